// glyph_kernels.hip -- gfx950 kernels of the glyph filter: point sets to
// spheres and arrows (glyph_common.h holds the rule).
//
//   check   a grid-stride pass over the arrays in use (a block per 1,024
//           coordinates of the largest set, 2,048 blocks at most): finiteness
//           and the scales' sign, into the set's status word
//   count   one lane per point: the keep rule; a block scan leaves the lane's
//           flag and exclusive rank and the block's sum
//   scan    one workgroup per set: block sums to block bases, the total
//   place   one lane per point: kept lanes write their record (point, factor,
//           tangent, frame normal, colour, id) at base + rank
//   expand  one thread per output vertex and one per face: the glyph is
//           t / V, a division by a per-set constant, then dense 12-B stores
//
// A glyph's index is its block's base plus its exclusive rank, so the output
// order is point order: no atomic decides an index and two runs write the same
// bytes.  Data moves between workgroups only across launch boundaries on one
// stream.  Every store is bounded by a count or a capacity of the out table,
// every loop by an array size.
//
// The expansion is a streaming store: 28 B per vertex and 12 B per face out,
// against 48 B of record per glyph in, which the V threads of a glyph share
// through the vector L1.  The sphere table (at most 7.7 KB of vertices and
// 15 KB of faces) is read from the arena: consecutive threads read consecutive
// rows, every block reads the same rows, so it stays in L1 / L2 and staging it
// in LDS would add a barrier and save nothing.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "block_scan.h"
#include "color_common.h"
#include "glyph_common.h"
#include "glyph_kernels.h"
#include "spray_rt.h"

namespace spray_rt {
namespace {

using namespace glyph;

constexpr int kCheckBlock = 256;
constexpr unsigned kCheckBlocksMax = 2048;  // per set, grid-stride
constexpr int kScanBlock = 256;

__device__ inline Keep keep_of(const GlyphJob& J) {
  Keep K;
  K.vectors = J.vectors;
  K.scales = J.scales;
  K.select = J.select;
  K.select_lo = J.select_lo;
  K.select_hi = J.select_hi;
  K.stride = J.stride;
  K.size = J.size;
  K.msq = J.msq;
  K.arrow = J.shape == SPRAY_RT_GLYPH_ARROW;
  K.scale_by_vector = J.scale_by_vector != 0;
  return K;
}

__global__ __launch_bounds__(kCheckBlock) void glyph_check_kernel(
    const GlyphJob* __restrict__ jobs, uint32_t* __restrict__ status) {
  const GlyphJob& J = jobs[blockIdx.y];
  const size_t np = J.npoints;
  const size_t t0 = size_t(blockIdx.x) * kCheckBlock + threadIdx.x;
  const size_t stride = size_t(gridDim.x) * kCheckBlock;
  const float *points = J.points, *vectors = J.vectors, *scales = J.scales, *select = J.select,
              *cfield = J.cfield;
  uint32_t bad = 0;
  for (size_t e = t0; e < 3 * np; e += stride)
    if (!refit::finite_f(points[e])) bad |= kBadPoint;
  if (vectors)
    for (size_t e = t0; e < 3 * np; e += stride)
      if (!refit::finite_f(vectors[e])) bad |= kBadVector;
  if (scales)
    for (size_t e = t0; e < np; e += stride) {
      const float x = scales[e];
      if (!refit::finite_f(x))
        bad |= kBadScale;
      else if (x < 0.0f)
        bad |= kNegScale;
    }
  if (select)
    for (size_t e = t0; e < np; e += stride)
      if (!refit::finite_f(select[e])) bad |= kBadSelect;
  if (cfield)
    for (size_t e = t0; e < np; e += stride)
      if (!refit::finite_f(cfield[e])) bad |= kBadColor;
  if (bad) atomicOr(&status[blockIdx.y], bad);
}

__global__ __launch_bounds__(kBlock) void glyph_count_kernel(const GlyphJob* __restrict__ jobs) {
  const GlyphJob& J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kBlock];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < J.npoints;
  uint32_t kept = 0;
  if (live) {
    float s, d;
    kept = keep(keep_of(J), i, &s, &d) ? 1u : 0u;
  }
  uint32_t total;
  const uint32_t excl = block_excl_scan<kBlock>(kept, s_scan, &total);
  if (live) J.word[i] = excl | (kept ? kKept : 0u);
  if (threadIdx.x == 0) J.bbase[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanBlock) void glyph_scan_kernel(const GlyphJob* __restrict__ jobs) {
  const GlyphJob& J = jobs[blockIdx.x];
  __shared__ uint32_t s_scan[kScanBlock];
  const uint32_t nblocks = J.nblocks;
  uint32_t* bbase = J.bbase;
  uint32_t c = 0;  // the same in every thread; npoints < 2^31, so no sum wraps
  for (uint32_t b0 = 0; b0 < nblocks; b0 += kScanBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const bool live = b < nblocks;
    uint32_t total;
    const uint32_t excl = block_excl_scan<kScanBlock>(live ? bbase[b] : 0u, s_scan, &total);
    if (live) bbase[b] = c + excl;
    c += total;
  }
  if (threadIdx.x == 0) J.count->kept = c;
}

__global__ __launch_bounds__(kBlock) void glyph_place_kernel(const GlyphJob* __restrict__ jobs,
                                                            const GlyphOut* __restrict__ outs) {
  const GlyphJob& J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= J.npoints) return;
  const uint32_t w = J.word[i];
  if (!(w & kKept)) return;
  const GlyphOut& O = outs[blockIdx.y];
  const uint64_t g = uint64_t(J.bbase[blockIdx.x]) + (w & ~kKept);
  if (g >= O.nglyphs) return;
  float s, d;
  keep(keep_of(J), i, &s, &d);  // the count pass's arithmetic again: s and d
  GlyphRec R{};
  for (int a = 0; a < 3; ++a) R.p[a] = J.points[3 * size_t(i) + a];
  R.s = s;
  R.id = i;
  if (J.shape == SPRAY_RT_GLYPH_ARROW) {
    const float l = sqrtf(d);
    for (int a = 0; a < 3; ++a) R.T[a] = J.vectors[3 * size_t(i) + a] / l;
    strm::axis_normal(R.T, R.N);
  }
  R.color = J.cfield ? J.ctable[cmap::bin(J.cfield[i], J.clo, J.cscale, J.ntable)] : J.color;
  if (O.recs) O.recs[g] = R;
  if (O.point_ids) O.point_ids[g] = i;
}

__global__ __launch_bounds__(kBlock) void glyph_expand_kernel(const GlyphJob* __restrict__ jobs,
                                                             const GlyphOut* __restrict__ outs) {
  const GlyphJob& J = jobs[blockIdx.y];
  const GlyphOut& O = outs[blockIdx.y];
  const uint32_t V = J.V, F = J.F;
  const uint64_t nglyphs = O.nglyphs;
  const uint64_t nverts = nglyphs * V, nfaces = nglyphs * F;  // < 2^32, < 2^29: the host checked
  const uint64_t x = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  const bool arrow = J.shape == SPRAY_RT_GLYPH_ARROW;

  // ---- one vertex ----
  if (O.recs && x < nverts && x < O.cap_verts) {
    const uint32_t g = uint32_t(x) / V, k = uint32_t(x) - g * V;
    const GlyphRec R = O.recs[g];
    float pos[3], nrm[3];
    if (arrow) {
      const uint32_t ns = uint32_t(J.nsides);
      float B[3];
      strm::cross3(R.T, R.N, B);
      // the row from the table in memory: no register copy of the table to index
      const uint32_t j = k / ns, kk = j < 4 ? k - j * ns : 0u;
      const float* rg = J.ring[kk];
      arrow_vertex(R.p, R.T, R.N, B, R.s, ns, k, rg[0], rg[1], J.cn, J.ct, pos, nrm);
    } else {
      const float* u = J.tverts + 3 * size_t(k);
      const float uk[3] = {u[0], u[1], u[2]};
      sphere_vertex(R.p, R.s, uk, pos, nrm);
    }
    if (O.verts)
      for (int a = 0; a < 3; ++a) O.verts[3 * x + a] = pos[a];
    if (O.vnormals)
      for (int a = 0; a < 3; ++a) O.vnormals[3 * x + a] = nrm[a];
    if (O.colors) O.colors[x] = R.color;
  }

  // ---- one face ----
  if (O.faces && x < nfaces && x < O.cap_faces) {
    const uint32_t g = uint32_t(x) / F, r = uint32_t(x) - g * F;
    uint32_t f[3];
    if (arrow) {
      arrow_face(uint32_t(J.nsides), r, f);
    } else {
      const uint32_t* tf = J.tfaces + 3 * size_t(r);
      for (int a = 0; a < 3; ++a) f[a] = tf[a];
    }
    for (int a = 0; a < 3; ++a) O.faces[3 * x + a] = g * V + f[a];
  }
}

}  // namespace

hipError_t launch_glyph_check(hipStream_t s, const GlyphJob* jobs, int njobs, uint32_t max_blocks,
                              uint32_t* status) {
  // four elements of the largest array (3 floats a point) per thread, 2048 blocks at most
  const unsigned blocks = std::min(std::max((3u * max_blocks + 3u) / 4u, 1u), kCheckBlocksMax);
  hipLaunchKernelGGL(glyph_check_kernel, dim3(blocks, unsigned(njobs)), dim3(kCheckBlock), 0,
                     s, jobs, status);
  return hipGetLastError();
}

hipError_t launch_glyph_count(hipStream_t s, const GlyphJob* jobs, int njobs, uint32_t max_blocks) {
  if (max_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(glyph_count_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kBlock), 0, s,
                     jobs);
  return hipGetLastError();
}

hipError_t launch_glyph_scan(hipStream_t s, const GlyphJob* jobs, int njobs) {
  hipLaunchKernelGGL(glyph_scan_kernel, dim3(unsigned(njobs)), dim3(kScanBlock), 0, s, jobs);
  return hipGetLastError();
}

hipError_t launch_glyph_place(hipStream_t s, const GlyphJob* jobs, const GlyphOut* outs, int njobs,
                              uint32_t max_blocks) {
  if (max_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(glyph_place_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kBlock), 0, s,
                     jobs, outs);
  return hipGetLastError();
}

hipError_t launch_glyph_expand(hipStream_t s, const GlyphJob* jobs, const GlyphOut* outs,
                               int njobs, uint64_t max_items) {
  if (max_items == 0) return hipSuccess;
  // Fewer than 2^29 items, so fewer than 2^21 blocks: the faces bound the
  // vertices (V < F for either shape), and the host rejects 2^29 faces.
  const unsigned blocks = unsigned((max_items + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(glyph_expand_kernel, dim3(blocks, unsigned(njobs)), dim3(kBlock), 0, s, jobs,
                     outs);
  return hipGetLastError();
}

}  // namespace spray_rt
