// job_arena_test.cpp -- the layout part of spray_amd/csrc/job_arena.h on the
// CPU (tests/test_job_arena.py compiles it with the sanitizers and runs it).
//
// Properties of takes, marks and the head, then the offsets of the build
// call's take sequence (build_device.cpp) against their closed form, a chain
// of aligned sizes, for 1 and 3 jobs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "job_arena.h"

using spray_rt::detail::align256;
using spray_rt::detail::HeadTake;
using spray_rt::detail::JobArena;
using spray_rt::detail::Take;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

namespace {

// Stand-ins of the table entries' sizes (build_kernels.h, refit_kernels.h,
// rt_common.h).
template <size_t N>
struct Bytes {
  char b[N];
};
using BuildJob = Bytes<128>;
using RefitJob = Bytes<144>;
using BuildRec = Bytes<160>;
using CopyJob = Bytes<24>;
using QGrid = Bytes<32>;
using BvhNode = Bytes<64>;
using QNode4 = Bytes<64>;
using Uint2 = Bytes<8>;
constexpr size_t kBuildParts = 64, kRefitLevels = 32;

struct Span {
  size_t off, bytes;
};

void test_takes() {
  JobArena A;
  std::vector<Span> spans;
  const size_t m0 = A.mark();
  CHECK(m0 == 0 && A.head == 0);
  const HeadTake<RefitJob> a = A.take_head<RefitJob>(3);
  spans.push_back({a.off, 3 * sizeof(RefitJob)});
  const size_t m1 = A.mark();
  CHECK(m1 == align256(3 * sizeof(RefitJob)));
  const HeadTake<uint32_t> b = A.take_head<uint32_t>(3);
  spans.push_back({b.off, 12});
  const size_t m2 = A.mark();
  CHECK(m2 == m1 + 256);
  CHECK(A.head == m2);  // the head ends where the last mirrored take ends
  const Take<QGrid> g = A.take<QGrid>(3);
  spans.push_back({g.off, 96});
  CHECK(A.head == m2 && A.mark() == m2 + 256);
  // a zero-count take: no bytes, the offset of the next take, still resolves
  const size_t before = A.mark();
  const Take<BvhNode> z = A.take<BvhNode>(0);
  CHECK(bool(z) && z.off == before && A.mark() == before);
  const Take<uint8_t> odd = A.take<uint8_t>(257);
  spans.push_back({odd.off, 257});
  CHECK(odd.off == z.off && A.mark() == before + 512);
  const Take<uint64_t> last = A.take<uint64_t>(1);
  spans.push_back({last.off, 8});
  CHECK(!Take<float>{});  // nothing taken
  size_t end = 0;
  for (const Span& s : spans) {  // aligned, monotone, non-overlapping
    CHECK(s.off % 256 == 0);
    CHECK(s.off >= end);
    end = s.off + s.bytes;
  }
  CHECK(end <= A.mark() && A.mark() % 256 == 0);
  // both sides resolve to base + offset
  std::vector<char> dev(A.used), host(A.head);
  A.d = dev.data();
  A.h = host.data();
  CHECK(reinterpret_cast<char*>(A.dev(a)) == dev.data());
  CHECK(reinterpret_cast<char*>(A.dev(b)) == dev.data() + m1);
  CHECK(reinterpret_cast<char*>(A.host(b)) == host.data() + m1);
  CHECK(reinterpret_cast<char*>(A.dev(z)) == dev.data() + before);
  CHECK(reinterpret_cast<char*>(A.dev(last)) == dev.data() + last.off);
  A.host(b)[2] = 7;  // inside the mirror (the sanitizer's business)
  A.dev(last)[0] = 9;
  A.reset();
  CHECK(A.mark() == 0 && A.head == 0 && A.d == dev.data());
}

// The build call: its takes in order, against the chain of aligned sizes.
void test_build_layout(const std::vector<size_t>& nfaces) {
  const size_t nj = nfaces.size();
  size_t total_tris = 0;
  for (size_t f : nfaces) total_tris += f;
  // ---- the chain ----
  const size_t o_bjobs = 0;
  const size_t o_rjobs = o_bjobs + align256(nj * 128);
  const size_t o_offsets = o_rjobs + align256(nj * 144);
  const size_t o_status = o_offsets + align256((nj + 1) * 4);
  const size_t o_rec = o_status + align256(nj * 4);
  const size_t o_jobs2 = o_rec + align256(nj * 160);
  const size_t o_copies = o_jobs2 + align256(nj * 144);
  const size_t head_bytes = o_copies + align256(6 * nj * 24);
  const size_t o_grid = head_bytes;
  const size_t o_keys = o_grid + align256(nj * 32);
  const size_t o_sorted = o_keys + align256(total_tris * 8);
  size_t total = o_sorted + align256(total_tris * 8);
  auto chain = [&](size_t bytes) {
    const size_t o = total;
    total += align256(bytes);
    return o;
  };
  // ---- the takes ----
  JobArena A;
  CHECK(A.take_head<BuildJob>(nj).off == o_bjobs);
  CHECK(A.take_head<RefitJob>(nj).off == o_rjobs);
  CHECK(A.take_head<uint32_t>(nj + 1).off == o_offsets);
  CHECK(A.mark() == o_status);
  CHECK(A.take_head<uint32_t>(nj).off == o_status);
  CHECK(A.mark() == o_rec);
  CHECK(A.take_head<BuildRec>(nj).off == o_rec);
  CHECK(A.mark() == o_jobs2);
  CHECK(A.take_head<RefitJob>(nj).off == o_jobs2);
  CHECK(A.take_head<CopyJob>(6 * nj).off == o_copies);
  CHECK(A.head == head_bytes);
  CHECK(A.take<QGrid>(nj).off == o_grid);
  CHECK(A.take<uint64_t>(total_tris).off == o_keys);
  CHECK(A.take<uint64_t>(total_tris).off == o_sorted);
  for (size_t nt : nfaces) {
    const size_t cap = nt > 1 ? nt - 1 : 1;
    CHECK(A.take<float>(kBuildParts * 6).off == chain(kBuildParts * 6 * 4));
    CHECK(A.take<uint32_t>(nt).off == chain(nt * 4));
    CHECK(A.take<char>(64 + cap * sizeof(QNode4)).off == chain(64 + cap * 64));
    CHECK(A.take<BvhNode>(cap).off == chain(cap * 64));
    CHECK(A.take<QNode4>(cap).off == chain(cap * 64));
    CHECK(A.take<Uint2>(cap).off == chain(cap * 8));
    CHECK(A.take<Uint2>(cap).off == chain(cap * 8));
    CHECK(A.take<uint8_t>(cap).off == chain(cap));
    CHECK(A.take<uint32_t>(cap).off == chain(cap * 4));
    CHECK(A.take<uint32_t>(kRefitLevels).off == chain(kRefitLevels * 4));
    CHECK(A.take<int32_t>(4 * cap).off == chain(4 * cap * 4));
  }
  CHECK(A.mark() == total && A.head == head_bytes);
}

#ifdef HOST_OF_A_PLAIN_TAKE  // must not compile: only head takes have a host side
void* host_of_a_plain_take(JobArena& A) { return A.host(A.take<int>(1)); }
#endif

}  // namespace

int main() {
  test_takes();
  test_build_layout({5480});          // one job
  test_build_layout({1, 12, 5480});   // three, the 1-triangle one with cap == 1
  test_build_layout({0, 0, 0});       // empty meshes: zero-count takes throughout
  std::printf("job_arena_test ok\n");
  return 0;
}
