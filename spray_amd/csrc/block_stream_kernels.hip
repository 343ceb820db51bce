// block_stream_kernels.hip -- gfx950 kernels of the multi-block streamline
// filter: sets of vector blocks and seeds to polylines that continue from block
// to block (block_stream_common.h holds the rule).
//
//   check      a grid-stride pass over every block's vector and colour samples
//              and over the seeds: finiteness, into the set's status words
//   count      one lane per half-line: fixed-step RK4 until the half ends, the
//              block rule deciding each sample's grid; the block scan of
//              stream_kernels.hip's count pass
//   integrate  one lane per half-line, the same arithmetic again: points, line
//              offsets and info, the block of every point; for tubes the frame,
//              tangent and colour of every point and the per-line tube sums
//
// The scan of the block sums and the tube expansion are stream_kernels.hip's
// launches on the set's StreamJob.  Output order, determinism, the bounds of
// stores and loops are as there; the miss path adds one loop, bounded by the
// set's block count.
//
// A lane's grid is its own: the current block's index, base pointer, dims,
// origin and spacing live in 12 VGPRs and change only in the miss path, so the
// in-block step has the dependent chain of the single-grid kernels (divide,
// floor, address, gather, lerp) with vector operands where those have scalar
// ones.  The miss path reads the set's table of boxes front to back (48 B a
// block, no division: block_stream_common.h); the lanes of a wave that miss
// together read the same addresses, and the block's record is read on a hit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "block_scan.h"
#include "block_stream_common.h"
#include "block_stream_kernels.h"
#include "color_common.h"
#include "spray_rt.h"

namespace spray_rt {
namespace {

using namespace strm;
using bstrm::Blocks;
using bstrm::BlockRec;
using bstrm::Cur;

constexpr int kCheckBlock = 256;
constexpr unsigned kCheckBlocks = 64;  // per set, grid-stride

__global__ __launch_bounds__(kCheckBlock) void block_stream_check_kernel(
    const StreamJob* __restrict__ jobs, const BlockJob* __restrict__ bjobs,
    uint32_t* __restrict__ status) {
  const StreamJob J = jobs[blockIdx.y];
  const BlockJob B = bjobs[blockIdx.y];
  const size_t t0 = size_t(blockIdx.x) * kCheckBlock + threadIdx.x;
  const size_t stride = size_t(kCheckBlocks) * kCheckBlock;
  uint32_t bad = 0, first = bstrm::kNoBlock;
  for (uint32_t b = 0; b < B.nvb; ++b) {
    const BlockRec& R = B.blocks[b];
    const size_t np = size_t(R.n[0]) * size_t(R.n[1]) * size_t(R.n[2]);
    const float* v = R.vectors;
    const float* g = R.cfield;
    uint32_t here = 0;
    for (size_t e = t0; e < 3 * np; e += stride)
      if (!refit::finite_f(v[e])) here |= kBadVector;
    if (g)
      for (size_t e = t0; e < np; e += stride)
        if (!refit::finite_f(g[e])) here |= kBadColor;
    if (here && first == bstrm::kNoBlock) first = b;
    bad |= here;
  }
  for (size_t e = t0; e < 3 * size_t(J.nseeds); e += stride)
    if (!refit::finite_f(J.seeds[e])) bad |= kBadSeed;
  if (bad) atomicOr(&status[2 * blockIdx.y], bad);
  if (first != bstrm::kNoBlock) atomicMin(&status[2 * blockIdx.y + 1], first);
}

// The half a lane integrates (stream_kernels.hip's lane order).
struct Lane {
  uint32_t seed;
  bool back, owner;
};
__device__ inline Lane lane_of(const StreamJob& J, uint32_t lane) {
  Lane L;
  if (J.direction == SPRAY_RT_STREAM_BOTH) {
    L.seed = lane >> 1;
    L.back = !(lane & 1u);
    L.owner = !L.back;
  } else {
    L.seed = lane;
    L.back = J.direction == SPRAY_RT_STREAM_BACKWARD;
    L.owner = true;
  }
  return L;
}

__global__ __launch_bounds__(kBlock) void block_stream_count_kernel(
    const StreamJob* __restrict__ jobs, const BlockJob* __restrict__ bjobs) {
  const StreamJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const BlockJob B = bjobs[blockIdx.y];
  __shared__ uint64_t s_scan[kBlock];
  __shared__ uint32_t s_cnt[kBlock];
  const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
  const bool live = lane < J.nlanes;
  uint32_t cnt = 0;
  int end = kEndSeed;
  Lane L{};
  if (live) {
    L = lane_of(J, lane);
    const Blocks S = {B.blocks, B.boxes, B.nvb};
    const float seed[3] = {J.seeds[3 * size_t(L.seed)], J.seeds[3 * size_t(L.seed) + 1],
                           J.seeds[3 * size_t(L.seed) + 2]};
    Cur cur;
    Cell c0;
    if (bstrm::locate_any(S, seed, &cur, &c0)) {
      const int steps = bstrm::trace_count(S, cur, seed, c0, L.back ? -J.step : J.step, J.msq,
                                           J.max_steps, &end);
      cnt = uint32_t(steps) + (L.owner ? 1u : 0u);
    }
  }
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  uint32_t line_pts = 0;  // in the lane that closes the line
  if (live && L.owner)
    line_pts = cnt + (J.direction == SPRAY_RT_STREAM_BOTH ? s_cnt[threadIdx.x - 1] : 0u);
  const uint64_t v = scan_word(cnt, line_pts);
  uint64_t total;
  const uint64_t excl = block_excl_scan<kBlock>(v, s_scan, &total);
  if (live) {
    J.word[lane] = lane_word(cnt, end);
    J.loc[lane] = excl;
  }
  if (threadIdx.x == 0)
    J.bbase[blockIdx.x] =
        make_uint4(scan_points(total), scan_tube_points(total), scan_tube_lines(total), 0u);
}

template <bool kTubes>
__global__ __launch_bounds__(kBlock) void block_stream_integrate_kernel(
    const StreamJob* __restrict__ jobs, const BlockJob* __restrict__ bjobs,
    const StreamOut* __restrict__ outs, const BlockOut* __restrict__ bouts) {
  const StreamJob J = jobs[blockIdx.y];
  const StreamOut O = outs[blockIdx.y];
  if (J.nseeds == 0 && blockIdx.x == 0 && threadIdx.x == 0) {  // the set's only offsets
    if (O.line_offsets) O.line_offsets[0] = 0;
    if (kTubes && O.tube_points) O.tube_points[0] = 0;
    if (kTubes && O.tube_lines) O.tube_lines[0] = 0;
  }
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
  if (lane >= J.nlanes) return;
  const BlockJob B = bjobs[blockIdx.y];
  uint32_t* const pblocks = bouts[blockIdx.y].point_blocks;
  const Lane L = lane_of(J, lane);
  const uint32_t w = J.word[lane], cnt = word_count(w);
  const uint64_t excl = J.loc[lane];
  const uint4 base = J.bbase[blockIdx.x];
  const uint32_t start = base.x + scan_points(excl);
  const bool both = J.direction == SPRAY_RT_STREAM_BOTH;

  // ---- the line's entries, by the lane that closes it ----
  if (L.owner) {
    const uint32_t wb = both ? J.word[lane - 1] : w;  // the backward half's word
    const uint32_t nback = both ? word_count(wb) : (L.back ? cnt - (cnt ? 1u : 0u) : 0u);
    const uint32_t line_start = both ? start - nback : start;
    const uint32_t m = both ? nback + cnt : cnt;
    const uint32_t tp = base.y + scan_tube_points(excl), tl = base.z + scan_tube_lines(excl);
    // a half the direction leaves out ends by STEPS; a seed outside by SEED
    const uint32_t end_here = word_end(w);
    uint32_t end_back = both ? word_end(wb) : (L.back ? end_here : uint32_t(kEndSteps));
    uint32_t end_fwd = L.back ? uint32_t(kEndSteps) : end_here;
    if (end_here == uint32_t(kEndSeed)) end_back = end_fwd = uint32_t(kEndSeed);
    if (O.line_offsets) O.line_offsets[L.seed] = line_start;
    if (O.line_info) {
      O.line_info[2 * size_t(L.seed)] = nback;
      O.line_info[2 * size_t(L.seed) + 1] = end_back | (end_fwd << 8);
    }
    if (kTubes && O.tube_points) O.tube_points[L.seed] = tp;
    if (kTubes && O.tube_lines) O.tube_lines[L.seed] = tl;
    if (L.seed + 1 == J.nseeds) {
      if (O.line_offsets) O.line_offsets[J.nseeds] = line_start + m;
      if (kTubes && O.tube_points) O.tube_points[J.nseeds] = tp + (m >= 2 ? m : 0u);
      if (kTubes && O.tube_lines) O.tube_lines[J.nseeds] = tl + (m >= 2 ? 1u : 0u);
    }
  }
  if (cnt == 0) return;  // a seed outside, or a backward half without a step

  // ---- the half-line's points ----
  const Blocks S = {B.blocks, B.boxes, B.nvb};
  const float h = L.back ? -J.step : J.step;
  const uint32_t nsteps = L.owner ? cnt - 1 : cnt;
  float p[3] = {J.seeds[3 * size_t(L.seed)], J.seeds[3 * size_t(L.seed) + 1],
                J.seeds[3 * size_t(L.seed) + 2]};
  Cur cur;
  Cell c;
  if (!bstrm::locate_any(S, p, &cur, &c)) return;  // not reached: cnt > 0
  Frame fr = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (uint32_t k = 0; k <= nsteps; ++k) {
    float k1[3];
    sample_vector(cur.G, c, k1);
    if (kTubes) frame_at(k1, J.msq, k == 0, &fr);
    const uint64_t idx = uint64_t(start) + (L.back ? nsteps - k : k);
    if ((k > 0 || L.owner) && idx < O.cap_points) {
      if (O.points)
        for (int a = 0; a < 3; ++a) O.points[3 * idx + a] = p[a];
      if (pblocks) pblocks[idx] = cur.b;
      if (kTubes) {
        for (int a = 0; a < 3; ++a) {
          O.pnormals[3 * idx + a] = fr.N[a];
          O.ptangents[3 * idx + a] = fr.T[a];
        }
        if (O.pcolors) {
          uint32_t col = J.color;
          if (B.has_color)
            col = J.ctable[cmap::bin(sample_scalar(cur.G, S.tab[cur.b].cfield, c), J.clo,
                                     J.cscale, J.ntable)];
          O.pcolors[idx] = col;
        }
      }
    }
    if (k == nsteps) break;
    float pn[3];
    Cell cn;
    if (bstrm::rk4(S, &cur, p, k1, h, pn, &cn) != kTaken) break;  // not reached: the count pass decided
    for (int a = 0; a < 3; ++a) p[a] = pn[a];
    c = cn;
  }
}

}  // namespace

hipError_t launch_block_stream_check(hipStream_t s, const StreamJob* jobs, const BlockJob* bjobs,
                                     int njobs, uint32_t* status) {
  hipLaunchKernelGGL(block_stream_check_kernel, dim3(kCheckBlocks, unsigned(njobs)),
                     dim3(kCheckBlock), 0, s, jobs, bjobs, status);
  return hipGetLastError();
}

hipError_t launch_block_stream_count(hipStream_t s, const StreamJob* jobs, const BlockJob* bjobs,
                                     int njobs, uint32_t max_blocks) {
  if (max_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(block_stream_count_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kBlock), 0,
                     s, jobs, bjobs);
  return hipGetLastError();
}

hipError_t launch_block_stream_integrate(hipStream_t s, const StreamJob* jobs,
                                         const BlockJob* bjobs, const StreamOut* outs,
                                         const BlockOut* bouts, int njobs, uint32_t max_blocks,
                                         bool tubes) {
  const dim3 grid(std::max(max_blocks, 1u), unsigned(njobs));  // block 0: sets without seeds
  if (tubes)
    hipLaunchKernelGGL(block_stream_integrate_kernel<true>, grid, dim3(kBlock), 0, s, jobs, bjobs,
                       outs, bouts);
  else
    hipLaunchKernelGGL(block_stream_integrate_kernel<false>, grid, dim3(kBlock), 0, s, jobs, bjobs,
                       outs, bouts);
  return hipGetLastError();
}

}  // namespace spray_rt
