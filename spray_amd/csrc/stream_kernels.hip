// stream_kernels.hip -- gfx950 kernels of the streamline filter: vector grids
// and seeds to polylines and to tubes (stream_common.h holds the rule).
//
//   check      a grid-stride pass over the vector samples, the colour samples
//              and the seeds: finiteness, into the field's status word
//   count      one lane per half-line: fixed-step RK4 until the half ends; a
//              block scan leaves the lane's word and exclusive sums and the
//              block's sums
//   scan       one workgroup per field: block sums to block bases, the totals
//   integrate  one lane per half-line, the same arithmetic again: points (the
//              backward half at descending indices), line offsets and info;
//              for tubes the frame normal, tangent and colour of every point
//              and the per-line tube sums
//   expand     one thread per output vertex and one per face: the line by a
//              bounded binary search of the per-line sums, then dense writes
//
// A lane's points start at bbase[block].x + its exclusive sum, so the output
// order is (line, point): no atomic decides an index and two runs write the
// same bytes.  Data moves between workgroups only across launch boundaries on
// one stream.  Every store is bounded by a capacity of the out table, every
// loop by max_steps, the lane count or 32 halvings.
//
// The integration is a chain of dependent gathers (32 corner loads of 12 B
// per step, each stage's address a function of the previous stage's value):
// latency-bound, so the kernels keep their state in registers, use no LDS
// beyond the scan, and rely on occupancy; the samples come through the vector
// L1 and L2 (a 33^3 grid of vectors is 431 KB: L2-resident).  Lanes whose
// half-lines end early idle until the wave's longest ends.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "block_scan.h"
#include "color_common.h"
#include "stream_common.h"
#include "stream_kernels.h"
#include "spray_rt.h"

namespace spray_rt {
namespace {

using namespace strm;

constexpr int kCheckBlock = 256;
constexpr unsigned kCheckBlocks = 64;  // per field, grid-stride
constexpr int kScanBlock = 256;

__device__ inline Grid grid_of(const StreamJob& J) {
  Grid G;
  G.vectors = J.vectors;
  for (int a = 0; a < 3; ++a) {
    G.n[a] = J.dims[a];
    G.origin[a] = J.origin[a];
    G.spacing[a] = J.spacing[a];
  }
  return G;
}

__global__ __launch_bounds__(kCheckBlock) void stream_check_kernel(
    const StreamJob* __restrict__ jobs, uint32_t* __restrict__ status) {
  const StreamJob J = jobs[blockIdx.y];
  const size_t np = size_t(J.dims[0]) * size_t(J.dims[1]) * size_t(J.dims[2]);
  const size_t t0 = size_t(blockIdx.x) * kCheckBlock + threadIdx.x;
  const size_t stride = size_t(kCheckBlocks) * kCheckBlock;
  uint32_t bad = 0;
  for (size_t e = t0; e < 3 * np; e += stride)
    if (!refit::finite_f(J.vectors[e])) bad |= kBadVector;
  if (J.cfield)
    for (size_t e = t0; e < np; e += stride)
      if (!refit::finite_f(J.cfield[e])) bad |= kBadColor;
  for (size_t e = t0; e < 3 * size_t(J.nseeds); e += stride)
    if (!refit::finite_f(J.seeds[e])) bad |= kBadSeed;
  if (bad) atomicOr(&status[blockIdx.y], bad);
}

// The half a lane integrates: its seed, whether it runs backward, whether it
// writes the seed point and closes the line.
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

__global__ __launch_bounds__(kBlock) void stream_count_kernel(const StreamJob* __restrict__ jobs) {
  const StreamJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint64_t s_scan[kBlock];
  __shared__ uint32_t s_cnt[kBlock];
  const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
  const bool live = lane < J.nlanes;
  uint32_t cnt = 0;
  int end = kEndSeed;
  Lane L{};
  if (live) {
    L = lane_of(J, lane);
    const Grid G = grid_of(J);
    const float seed[3] = {J.seeds[3 * size_t(L.seed)], J.seeds[3 * size_t(L.seed) + 1],
                           J.seeds[3 * size_t(L.seed) + 2]};
    Cell c0;
    if (locate(G, seed, &c0)) {
      const int steps = trace_count(G, seed, c0, L.back ? -J.step : J.step, J.msq, J.max_steps, &end);
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

__global__ __launch_bounds__(kScanBlock) void stream_scan_kernel(const StreamJob* __restrict__ jobs) {
  const StreamJob J = jobs[blockIdx.x];
  __shared__ uint64_t s_scan[kScanBlock];
  uint64_t c[3] = {0, 0, 0};  // the same in every thread
  for (uint32_t b0 = 0; b0 < J.nblocks; b0 += kScanBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const bool live = b < J.nblocks;
    const uint4 s = live ? J.bbase[b] : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t in[3] = {s.x, s.y, s.z};
    uint32_t base[3];
    for (int k = 0; k < 3; ++k) {
      uint64_t total;
      const uint64_t excl = block_excl_scan<kScanBlock>(uint64_t(in[k]), s_scan, &total);
      base[k] = uint32_t(c[k] + excl);  // wraps only in a field the host rejects by its totals
      c[k] += total;
    }
    if (live) J.bbase[b] = make_uint4(base[0], base[1], base[2], 0u);
  }
  if (threadIdx.x == 0) {
    J.rec->npoints = c[0];
    J.rec->tube_points = c[1];
    J.rec->tube_lines = c[2];
  }
}

template <bool kTubes>
__global__ __launch_bounds__(kBlock) void stream_integrate_kernel(
    const StreamJob* __restrict__ jobs, const StreamOut* __restrict__ outs) {
  const StreamJob J = jobs[blockIdx.y];
  const StreamOut O = outs[blockIdx.y];
  if (J.nseeds == 0 && blockIdx.x == 0 && threadIdx.x == 0) {  // the field's only offsets
    if (O.line_offsets) O.line_offsets[0] = 0;
    if (kTubes && O.tube_points) O.tube_points[0] = 0;
    if (kTubes && O.tube_lines) O.tube_lines[0] = 0;
  }
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
  if (lane >= J.nlanes) return;
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
  const Grid G = grid_of(J);
  const float h = L.back ? -J.step : J.step;
  const uint32_t nsteps = L.owner ? cnt - 1 : cnt;
  float p[3] = {J.seeds[3 * size_t(L.seed)], J.seeds[3 * size_t(L.seed) + 1],
                J.seeds[3 * size_t(L.seed) + 2]};
  Cell c;
  locate(G, p, &c);
  Frame fr = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (uint32_t k = 0; k <= nsteps; ++k) {
    float k1[3];
    sample_vector(G, c, k1);
    if (kTubes) frame_at(k1, J.msq, k == 0, &fr);
    const uint64_t idx = uint64_t(start) + (L.back ? nsteps - k : k);
    if ((k > 0 || L.owner) && idx < O.cap_points) {
      if (O.points)
        for (int a = 0; a < 3; ++a) O.points[3 * idx + a] = p[a];
      if (kTubes) {
        for (int a = 0; a < 3; ++a) {
          O.pnormals[3 * idx + a] = fr.N[a];
          O.ptangents[3 * idx + a] = fr.T[a];
        }
        if (O.pcolors)
          O.pcolors[idx] = J.cfield ? J.ctable[cmap::bin(sample_scalar(G, J.cfield, c), J.clo,
                                                         J.cscale, J.ntable)]
                                    : J.color;
      }
    }
    if (k == nsteps) break;
    float pn[3];
    Cell cn;
    rk4(G, p, k1, h, pn, &cn);  // taken: the count pass decided
    for (int a = 0; a < 3; ++a) p[a] = pn[a];
    c = cn;
  }
}

// The last line l of [0, nseeds) whose tube starts at or before item x, a
// line's start being tube_points[l] * per_point + tube_lines[l] * per_line.
__device__ inline uint32_t find_line(const StreamOut& O, uint32_t nseeds, uint64_t x,
                                     uint32_t per_point, uint32_t per_line, uint64_t* first) {
  uint32_t lo = 0, hi = nseeds;
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const uint64_t off =
        uint64_t(O.tube_points[mid]) * per_point + uint64_t(O.tube_lines[mid]) * per_line;
    if (off <= x)
      lo = mid;
    else
      hi = mid;
  }
  *first = uint64_t(O.tube_points[lo]) * per_point + uint64_t(O.tube_lines[lo]) * per_line;
  return lo;
}

__global__ __launch_bounds__(kBlock) void stream_expand_kernel(const StreamJob* __restrict__ jobs,
                                                              const StreamOut* __restrict__ outs) {
  const StreamJob J = jobs[blockIdx.y];
  if (J.nseeds == 0) return;
  const StreamOut O = outs[blockIdx.y];
  const uint32_t ns = uint32_t(J.nsides);
  const uint64_t tp = O.tube_points[J.nseeds], tl = O.tube_lines[J.nseeds];
  const uint64_t nverts = tp * ns + 2 * tl, nfaces = 2 * uint64_t(ns) * tp;
  const uint64_t x = uint64_t(blockIdx.x) * kBlock + threadIdx.x;

  // ---- one vertex ----
  if (x < nverts && x < O.cap_verts) {
    uint64_t first;
    const uint32_t l = find_line(O, J.nseeds, x, ns, 2u, &first);
    const uint32_t p0 = O.line_offsets[l], m = O.line_offsets[l + 1] - p0;
    const uint64_t r = x - first;
    if (m >= 2 && r < tube_verts(m, ns)) {
      const bool ring = r < uint64_t(m) * ns;
      const uint32_t j = ring ? uint32_t(r / ns) : (r == uint64_t(m) * ns ? 0u : m - 1);
      const uint32_t k = ring ? uint32_t(r - uint64_t(j) * ns) : 0u;
      const size_t pi = size_t(p0) + j;
      float P[3], N[3], T[3], pos[3], nrm[3];
      for (int a = 0; a < 3; ++a) {
        P[a] = O.points[3 * pi + a];
        N[a] = O.pnormals[3 * pi + a];
        T[a] = O.ptangents[3 * pi + a];
      }
      if (ring) {
        float B[3];
        cross3(T, N, B);
        // the row from the table in memory: the job's copy stays in registers
        const float* rg = jobs[blockIdx.y].ring[k];
        ring_vertex(P, N, B, rg[0], rg[1], J.radius, pos, nrm);
      } else {
        const bool last = j != 0;
        for (int a = 0; a < 3; ++a) {
          pos[a] = P[a];
          nrm[a] = last ? T[a] : -T[a];
        }
      }
      if (O.verts)
        for (int a = 0; a < 3; ++a) O.verts[3 * x + a] = pos[a];
      if (O.vnormals)
        for (int a = 0; a < 3; ++a) O.vnormals[3 * x + a] = nrm[a];
      if (O.colors) O.colors[x] = O.pcolors[pi];
    }
  }

  // ---- one face ----
  if (x < nfaces && x < O.cap_faces && O.faces) {
    uint64_t first;
    const uint32_t l = find_line(O, J.nseeds, x, 2 * ns, 0u, &first);
    const uint32_t m = O.line_offsets[l + 1] - O.line_offsets[l];
    const uint64_t r = x - first;
    if (m >= 2 && r < tube_faces(m, ns)) {
      const uint32_t v0 = uint32_t(uint64_t(O.tube_points[l]) * ns + 2 * uint64_t(O.tube_lines[l]));
      uint32_t f[3];
      tube_face(ns, m, uint32_t(r), f);
      for (int a = 0; a < 3; ++a) O.faces[3 * x + a] = v0 + f[a];
    }
  }
}

}  // namespace

hipError_t launch_stream_check(hipStream_t s, const StreamJob* jobs, int njobs, uint32_t* status) {
  hipLaunchKernelGGL(stream_check_kernel, dim3(kCheckBlocks, unsigned(njobs)), dim3(kCheckBlock),
                     0, s, jobs, status);
  return hipGetLastError();
}

hipError_t launch_stream_count(hipStream_t s, const StreamJob* jobs, int njobs,
                               uint32_t max_blocks) {
  if (max_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(stream_count_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kBlock), 0, s,
                     jobs);
  return hipGetLastError();
}

hipError_t launch_stream_scan(hipStream_t s, const StreamJob* jobs, int njobs) {
  hipLaunchKernelGGL(stream_scan_kernel, dim3(unsigned(njobs)), dim3(kScanBlock), 0, s, jobs);
  return hipGetLastError();
}

hipError_t launch_stream_integrate(hipStream_t s, const StreamJob* jobs, const StreamOut* outs,
                                   int njobs, uint32_t max_blocks, bool tubes) {
  const dim3 grid(std::max(max_blocks, 1u), unsigned(njobs));  // block 0: fields without seeds
  if (tubes)
    hipLaunchKernelGGL(stream_integrate_kernel<true>, grid, dim3(kBlock), 0, s, jobs, outs);
  else
    hipLaunchKernelGGL(stream_integrate_kernel<false>, grid, dim3(kBlock), 0, s, jobs, outs);
  return hipGetLastError();
}

hipError_t launch_stream_expand(hipStream_t s, const StreamJob* jobs, const StreamOut* outs,
                                int njobs, uint64_t max_items) {
  if (max_items == 0) return hipSuccess;
  const unsigned blocks = unsigned((max_items + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(stream_expand_kernel, dim3(blocks, unsigned(njobs)), dim3(kBlock), 0, s, jobs,
                     outs);
  return hipGetLastError();
}

}  // namespace spray_rt
