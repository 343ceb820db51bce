// block_stream_host_check.cpp -- the host restatements of the multi-block
// streamline filter (spray_rt_block_streamlines_host,
// spray_rt_block_stream_tubes_host) as a stand-alone program, for a run under
// the host sanitizers: no GPU, no HIP runtime.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -DSPRAY_RT_STREAM_HOST_ONLY \
//       -I<rocm>/include -Iinclude -Ispray_amd/csrc spray_amd/csrc/streamlines.cpp \
//       spray_amd/csrc/block_streamlines.cpp tests/cpp/block_stream_host_check.cpp \
//       -o block_stream_host_check
//
// Every array is allocated at exactly the size the count call reports, so a
// store or a read past an end is the sanitizer's to find.
//
// Then the box of the miss path by brute force (block_stream_common.h): for the
// spacings, sizes and origins of the hard-box class of tests/block_stream_cases.py,
// inside(box_of(R), p) against strm::locate(grid_of(R), p) for every float p
// within 256 floats of either bound on each axis and for 2^20 floats spread over
// the whole float line on each axis with a spacing of its own, the bounds themselves against the division, and the
// float keys there and back.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "block_stream_common.h"
#include "spray_rt.h"

namespace {

namespace bstrm = spray_rt::bstrm;
namespace strm = spray_rt::strm;

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

struct Lines {
  std::vector<float> p;
  std::vector<uint32_t> off, info, blk;
};
struct Mesh {
  std::vector<float> v, n;
  std::vector<uint32_t> c, f;
};

// Counts, then traces into exact-size arrays.
Lines lines_of(const spray_rt_blockfield& S) {
  Lines L;
  size_t np = 0;
  expect(spray_rt_block_streamlines_host(&S, &np, nullptr, nullptr, nullptr, nullptr) ==
             SPRAY_RT_OK, "count call");
  L.p.resize(3 * np);
  L.blk.resize(np);
  L.off.resize(S.nseeds + 1);
  L.info.resize(2 * S.nseeds);
  expect(spray_rt_block_streamlines_host(&S, &np, L.p.data(), L.off.data(), L.info.data(),
                                         L.blk.data()) == SPRAY_RT_OK, "trace");
  expect(L.off[S.nseeds] == np, "the last offset is the point count");
  for (uint32_t b : L.blk) expect(b < uint32_t(S.nblocks), "point block in range");
  // single arrays
  expect(spray_rt_block_streamlines_host(&S, nullptr, nullptr, nullptr, nullptr, L.blk.data()) ==
             SPRAY_RT_OK, "point blocks alone");
  return L;
}

Mesh tubes_of(const spray_rt_blockfield& S, const spray_rt_tube& T, const spray_rt_block_color* bc) {
  Mesh M;
  size_t nv = 0, nf = 0;
  expect(spray_rt_block_stream_tubes_host(&S, &T, bc, &nv, &nf, nullptr, nullptr, nullptr, nullptr) ==
             SPRAY_RT_OK, "tube count call");
  M.v.resize(3 * nv), M.n.resize(3 * nv), M.c.resize(nv), M.f.resize(3 * nf);
  expect(spray_rt_block_stream_tubes_host(&S, &T, bc, &nv, &nf, M.v.data(), M.n.data(), M.c.data(),
                                          M.f.data()) == SPRAY_RT_OK, "tubes");
  for (uint32_t x : M.f) expect(x < nv, "face index in range");
  for (float x : M.v) expect(std::isfinite(x), "finite position");
  return M;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// An n^3 lattice of a swirl with a lift, [z][y][x][3].
std::vector<float> swirl(int n, float c) {
  std::vector<float> v(size_t(3) * n * n * n);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        float* s = &v[3 * (size_t(i) + size_t(n) * (size_t(j) + size_t(n) * size_t(k)))];
        s[0] = -(float(j) - c) * 0.25f;
        s[1] = (float(i) - c) * 0.25f;
        s[2] = 0.0625f * float(std::sin(0.5 * double(i + k)));
      }
  return v;
}

// ---- the box of the miss path ----

size_t box_checked = 0;

// p on axis a, the origin on the other two (d = 0 there: inside).
bool box_agrees(const bstrm::BlockRec& R, const bstrm::BlockBox& B, const strm::Grid& G, int a,
                float x) {
  float p[3] = {R.origin[0], R.origin[1], R.origin[2]};
  p[a] = x;
  strm::Cell c;
  ++box_checked;
  return bstrm::inside(B, p) == strm::locate(G, p, &c);
}

void check_box(const float spacing[3], int n, float origin, bool sweep) {
  bstrm::BlockRec R{};
  for (int a = 0; a < 3; ++a) {
    R.origin[a] = origin;
    R.spacing[a] = spacing[a];
    R.n[a] = n;
  }
  const bstrm::BlockBox B = bstrm::box_of(R);
  const strm::Grid G = bstrm::grid_of(R);
  for (int a = 0; a < 3; ++a) {
    const float s = spacing[a], top = float(n - 1);
    // the bounds are the outermost floats whose quotient is in range
    const uint32_t klo = bstrm::float_key(B.lo[a]), khi = bstrm::float_key(B.hi[a]);
    expect(B.lo[a] / s >= 0.0f && !(bstrm::key_float(klo - 1) / s >= 0.0f), "lo is the lowest float in range");
    expect(B.hi[a] / s <= top && !(bstrm::key_float(khi + 1) / s <= top), "hi is the highest float in range");
    expect(B.lo[a] <= -0.0f && B.hi[a] >= 0.0f, "both zeros are in range");
    // every p within 256 floats of origin + lo and of origin + hi
    bool ok = true;
    for (float at : {origin + B.lo[a], origin + B.hi[a]}) {
      if (!std::isfinite(at)) at = at > 0 ? 3.4028235e38f : -3.4028235e38f;
      const uint32_t k0 = bstrm::float_key(at);
      for (int64_t k = int64_t(k0) - 256; k <= int64_t(k0) + 256; ++k)
        if (k >= 0 && k <= int64_t(0xFFFFFFFFu)) ok = ok && box_agrees(R, B, G, a, bstrm::key_float(uint32_t(k)));
    }
    expect(ok, "box and division agree within 256 floats of the bounds");
    if (!sweep || (a > 0 && spacing[a] == spacing[0])) continue;  // equal spacings: equal axes
    ok = true;
    for (uint32_t j = 0; j < (1u << 20); ++j) {  // one key in every stratum of 4096
      const uint32_t k = j * 4096u + (j * 2654435761u >> 20);
      ok = ok && box_agrees(R, B, G, a, bstrm::key_float(k));
    }
    expect(ok, "box and division agree over the float line");
  }
}

void check_boxes() {
  const float third = 1.0f / 3.0f;
  const float spacings[8][3] = {{0.1f, 0.1f, 0.1f}, {third, third, third}, {0.7f, 0.7f, 0.7f},
                                {3e-5f, 3e-5f, 3e-5f}, {1e-38f, 1e-38f, 1e-38f},
                                {3e37f, 3e37f, 3e37f}, {0.1f, third, 0.7f}, {3e-5f, 0.7f, 1e-38f}};
  const float origins[5] = {0.0f, -0.0f, 1e6f, -123456.7f, 1e-30f};
  for (int s = 0; s < 8; ++s)
    for (int o = 0; o < 5; ++o)
      for (int n = 2; n <= 5; ++n) check_box(spacings[s], n, origins[o], n == 2 + (s + o) % 4);
  // a spacing so small that hi is subnormal, one so large that top * s overflows
  bstrm::BlockRec R{};
  for (int a = 0; a < 3; ++a) R.spacing[a] = a == 0 ? 1e-38f : 3e38f, R.n[a] = 5;
  const bstrm::BlockBox B = bstrm::box_of(R);
  expect(B.hi[0] > 0.0f && B.hi[0] < 1.17549435e-38f * 4.0f && std::fpclassify(1e-38f) == FP_SUBNORMAL,
         "a subnormal spacing has a tiny hi");
  expect(B.hi[1] == 3.4028235e38f, "top * spacing overflows: every finite float is in range");
  // the keys: order, and there and back bitwise
  const float specials[] = {0.0f, -0.0f, strm::pos_inf(), -strm::pos_inf(), 1e-45f, -1e-45f,
                            1.17549435e-38f, 3.4028235e38f, -3.4028235e38f, 1.0f, -1.0f, 0.1f};
  for (float x : specials)
    expect(strm::bits(bstrm::key_float(bstrm::float_key(x))) == strm::bits(x), "key there and back");
  expect(bstrm::float_key(-0.0f) + 1 == bstrm::float_key(0.0f), "-0 is the float below +0");
  expect(bstrm::float_key(-strm::pos_inf()) < bstrm::float_key(-3.4028235e38f) &&
             bstrm::float_key(3.4028235e38f) + 1 == bstrm::float_key(strm::pos_inf()),
         "the infinities are the ends of the finite floats");
  bool ok = true;
  uint32_t prev = 0;
  for (uint32_t j = 0; j < (1u << 20); ++j) {
    const uint32_t k = j * 4096u + (j * 2654435761u >> 20);
    const float x = bstrm::key_float(k);
    ok = ok && bstrm::float_key(x) == k;
    if (j && x == x && bstrm::key_float(prev) == bstrm::key_float(prev))
      ok = ok && bstrm::key_float(prev) <= x;  // the order of the keys is the order of the floats
    prev = k;
  }
  expect(ok, "keys there and back and in order over the float line");
}

}  // namespace

int main() {
  // ---- a 9^3 lattice at spacing 0.25, split 2 x 2 x 2 into 5^3 blocks sharing planes ----
  const int n = 9, m = 5;
  const std::vector<float> whole = swirl(n, 4.0f);
  std::vector<float> color(size_t(n) * n * n);
  for (size_t e = 0; e < color.size(); ++e) color[e] = float(std::cos(0.37 * double(e)));
  std::vector<std::vector<float>> bv(8), bc(8);
  std::vector<spray_rt_vecblock> blocks(8);
  for (int b = 0; b < 8; ++b) {
    const int lo[3] = {(b & 1) * 4, ((b >> 1) & 1) * 4, (b >> 2) * 4};
    bv[b].resize(size_t(3) * m * m * m);
    bc[b].resize(size_t(m) * m * m);
    for (int k = 0; k < m; ++k)
      for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
          const size_t src = size_t(lo[0] + i) + size_t(n) * (size_t(lo[1] + j) + size_t(n) * size_t(lo[2] + k));
          const size_t dst = size_t(i) + size_t(m) * (size_t(j) + size_t(m) * size_t(k));
          for (int a = 0; a < 3; ++a) bv[b][3 * dst + a] = whole[3 * src + a];
          bc[b][dst] = color[src];
        }
    blocks[b] = {bv[b].data(), bc[b].data(), {m, m, m},
                 {0.25f * float(lo[0]), 0.25f * float(lo[1]), 0.25f * float(lo[2])},
                 {0.25f, 0.25f, 0.25f}};
  }
  std::vector<float> seeds;
  for (int s = 0; s < 23; ++s)
    for (int a = 0; a < 3; ++a)
      seeds.push_back(1.0f + 0.9f * float(std::sin(1.0 + 2.3 * double(3 * s + a))));
  seeds.insert(seeds.end(), {1.0f, 1.0f, 1.0f, 1.0f, 0.3f, 0.3f, 2.5f, 1.0f, 1.0f});  // corner, plane, outside
  const uint32_t table[5] = {0x0000FF, 0x00FF00, 0xFF0000, 0x808080, 0xFFFFFF};
  const spray_rt_block_color map = {table, 5, -0.5f, 0.5f};
  const spray_rt_tube tube = {0.03125f, 5, 0x123456, 1};
  size_t crossing = 0;
  for (int direction = SPRAY_RT_STREAM_FORWARD; direction <= SPRAY_RT_STREAM_BOTH; ++direction) {
    const spray_rt_blockfield S = {blocks.data(), 8, seeds.data(), seeds.size() / 3, 0.125f, 40,
                                   direction, 1e-6f};
    const Lines L = lines_of(S);
    for (size_t s = 0; s + 1 < L.off.size(); ++s)
      for (uint32_t k = L.off[s]; k + 1 < L.off[s + 1]; ++k) crossing += L.blk[k] != L.blk[k + 1];
    expect(L.off[24] > L.off[23] && L.blk[L.off[23] + L.info[2 * 23]] == 0,
           "a seed at the corner of eight blocks is in block 0");
    expect(L.info[2 * 25 + 1] == (SPRAY_RT_LINE_END_SEED | SPRAY_RT_LINE_END_SEED << 8),
           "a seed outside every block");
    const Mesh M = tubes_of(S, tube, &map);
    expect(!M.v.empty(), "the split has tubes");
  }
  expect(crossing > 50, "lines cross from block to block");

  // ---- P1: a set of one block gives the single-grid forms' bytes ----
  {
    const spray_rt_vecblock one = {whole.data(), color.data(), {n, n, n}, {-0.5f, 0.25f, 1.0f},
                                   {0.25f, 0.5f, 0.125f}};
    std::vector<float> s1;
    for (size_t e = 0; e < seeds.size(); ++e)
      s1.push_back(one.origin[e % 3] + seeds[e] * 4.0f * one.spacing[e % 3]);
    const spray_rt_blockfield S = {&one, 1, s1.data(), s1.size() / 3, 0.0625f, 30,
                                   SPRAY_RT_STREAM_BOTH, 1e-6f};
    const spray_rt_vecfield F = {whole.data(), {n, n, n}, {-0.5f, 0.25f, 1.0f}, {0.25f, 0.5f, 0.125f},
                                 s1.data(), s1.size() / 3, 0.0625f, 30, SPRAY_RT_STREAM_BOTH, 1e-6f};
    const Lines L = lines_of(S);
    size_t np = 0;
    expect(spray_rt_streamlines_host(&F, &np, nullptr, nullptr, nullptr) == SPRAY_RT_OK, "grid count");
    Lines G;
    G.p.resize(3 * np), G.off.resize(F.nseeds + 1), G.info.resize(2 * F.nseeds);
    expect(spray_rt_streamlines_host(&F, &np, G.p.data(), G.off.data(), G.info.data()) == SPRAY_RT_OK,
           "grid trace");
    expect(np > 200 && same(L.p, G.p) && same(L.off, G.off) && same(L.info, G.info),
           "one block: the polylines of the grid");
    const Mesh M = tubes_of(S, tube, &map);
    const spray_rt_grid_color gc = {color.data(), table, 5, -0.5f, 0.5f};
    size_t nv = 0, nf = 0;
    expect(spray_rt_stream_tubes_host(&F, &tube, &gc, &nv, &nf, nullptr, nullptr, nullptr, nullptr) ==
               SPRAY_RT_OK, "grid tube count");
    Mesh R;
    R.v.resize(3 * nv), R.n.resize(3 * nv), R.c.resize(nv), R.f.resize(3 * nf);
    expect(spray_rt_stream_tubes_host(&F, &tube, &gc, &nv, &nf, R.v.data(), R.n.data(), R.c.data(),
                                      R.f.data()) == SPRAY_RT_OK, "grid tubes");
    expect(same(M.v, R.v) && same(M.n, R.n) && same(M.c, R.c) && same(M.f, R.f),
           "one block: the tubes of the grid");
  }

  // ---- two blocks with a gap ----
  {
    std::vector<float> u(size_t(3) * 27, 0.0f);
    for (size_t e = 0; e < 27; ++e) u[3 * e] = 1.0f;
    const spray_rt_vecblock two[2] = {{u.data(), nullptr, {3, 3, 3}, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}},
                                      {u.data(), nullptr, {3, 3, 3}, {3.f, 0.f, 0.f}, {1.f, 1.f, 1.f}}};
    const float gs[6] = {0.5f, 1.0f, 1.0f, 2.5f, 1.0f, 1.0f};
    const spray_rt_blockfield S = {two, 2, gs, 2, 0.5f, 40, SPRAY_RT_STREAM_FORWARD, 1e-6f};
    const Lines L = lines_of(S);
    expect(L.off[1] == 4 && L.off[2] == 4, "the line stops at the gap, the seed in it has no points");
    expect(L.info[1] == (SPRAY_RT_LINE_END_STEPS | SPRAY_RT_LINE_END_GRID << 8), "GRID at the gap");
    expect(L.info[3] == (SPRAY_RT_LINE_END_SEED | SPRAY_RT_LINE_END_SEED << 8), "SEED in the gap");
    tubes_of(S, tube, nullptr);
    // the argument errors that need no array
    size_t np = 0;
    spray_rt_blockfield bad = S;
    bad.nblocks = 0;
    expect(spray_rt_block_streamlines_host(&bad, &np, nullptr, nullptr, nullptr, nullptr) ==
               SPRAY_RT_ERR_ARG, "no blocks");
    bad = S;
    bad.blocks = nullptr;
    expect(spray_rt_block_streamlines_host(&bad, &np, nullptr, nullptr, nullptr, nullptr) ==
               SPRAY_RT_ERR_ARG, "null blocks");
    const spray_rt_block_color map2 = {table, 5, 0.0f, 1.0f};
    size_t nv = 0, nf = 0;
    expect(spray_rt_block_stream_tubes_host(&S, &tube, &map2, &nv, &nf, nullptr, nullptr, nullptr,
                                            nullptr) == SPRAY_RT_ERR_ARG,
           "a colour table without colour fields");
  }

  check_boxes();
  expect(box_checked > (size_t(60) << 20), "the box sweep ran");

  std::printf("block_stream_host_check: %zu crossings, %zu box tests, %d failures\n", crossing,
              box_checked, failures);
  return failures ? 1 : 0;
}
