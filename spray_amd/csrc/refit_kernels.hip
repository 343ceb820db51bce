// refit_kernels.hip -- gfx950 kernels of spray_rt_domains_refit and
// spray_rt_slot_sah.
//
// A refit keeps a slot's topology (faces, prims, leaf ranges, child refs, the
// QNode4 collapse) and recomputes every number that depends on the vertex
// positions with the builder's own arithmetic (refit_common.h).  Two phases:
//   1. check_tris, fit_level x height, grid, quant: read the slot and the new
//      vertices, write scratch and one status word per slot;
//   2. commit: scratch -> slot, triangle records, normals, bounds.
// The host reads the status words between the two, so a rejected call has
// written no slot memory.
//
// Data moves between workgroups only across launch boundaries on one stream:
// the bottom-up fit is one launch per tree height (a node's inner children
// sit at lower heights, refit_order), batched over the slots of the call in
// blockIdx.y.  No atomics on the boxes, nothing depends on dispatch order.
// The traversal kernels fetch nodes through the scalar cache; the commit's
// vector stores reach them at the next launch boundary of the stream.
#include <hip/hip_runtime.h>

#include "refit_common.h"
#include "refit_kernels.h"

namespace spray_rt {
namespace {

using namespace refit;

constexpr int kRefitBlock = 256;
constexpr uint32_t kMaxGridX = 4096;  // grid-stride loops cover the rest

__device__ inline const float* side_lo(const BvhNode& n, int side) { return side ? n.r_lo : n.l_lo; }
__device__ inline const float* side_hi(const BvhNode& n, int side) { return side ? n.r_hi : n.l_hi; }
__device__ inline QNode4* slot_qnode(const RefitJob& J, uint32_t i) {
  return reinterpret_cast<QNode4*>(reinterpret_cast<char*>(J.nodes) - 64 -
                                   size_t(64) * (size_t(i) + 1));
}

// One thread per leaf-order triangle.  kCommit = false: flags a record that
// is not finite; kCommit = true: writes the 48-B record into the slot.
template <bool kCommit>
__global__ __launch_bounds__(kRefitBlock) void refit_tris_kernel(const RefitJob* __restrict__ jobs,
                                                                 uint32_t* __restrict__ status) {
  const RefitJob J = jobs[blockIdx.y];
  bool bad = false;
  for (uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x; i < J.ntris;
       i += gridDim.x * kRefitBlock) {
    const uint32_t* f = J.faces + 3 * size_t(J.prims[i]);
    float r[12];
    const bool ok = tri_record(J.verts + 3 * size_t(f[0]), J.verts + 3 * size_t(f[1]),
                               J.verts + 3 * size_t(f[2]), r);
    if (kCommit) {
      float4* out = reinterpret_cast<float4*>(J.tris + 12 * size_t(i));
      out[0] = make_float4(r[0], r[1], r[2], r[3]);
      out[1] = make_float4(r[4], r[5], r[6], r[7]);
      out[2] = make_float4(r[8], r[9], r[10], r[11]);
    } else {
      bad = bad || !ok;
    }
  }
  if (!kCommit && bad) atomicOr(&status[blockIdx.y], kBadVertex);
}

// The exact (unpadded) box of one child of slot node `node`, children of
// lower height read from scratch.
__device__ inline void fit_child(const RefitJob& J, const BvhNode& old, int side, float lo[3],
                                 float hi[3]) {
  const float* olo = side_lo(old, side);
  if (empty_box(olo)) {  // the never-hit box of a root that is a leaf: kept
    const float* ohi = side_hi(old, side);
    for (int j = 0; j < 3; ++j) {
      lo[j] = olo[j];
      hi[j] = ohi[j];
    }
    return;
  }
  for (int j = 0; j < 3; ++j) {
    lo[j] = pos_inf();
    hi[j] = -pos_inf();
  }
  const int32_t ref = side ? old.right : old.left;
  if (ref < 0) {
    uint32_t first, count;
    leaf_range(ref, &first, &count);
    for (uint32_t t = first; t < first + count && t < J.ntris; ++t) {
      const uint32_t* f = J.faces + 3 * size_t(J.prims[t]);
      for (int k = 0; k < 3; ++k) {
        const float* p = J.verts + 3 * size_t(f[k]);
        grow(lo, hi, p, p);
      }
    }
  } else if (uint32_t(ref) < J.nnodes) {
    const BvhNode& c = J.s_nodes[ref];
    if (!empty_box(c.l_lo)) grow(lo, hi, c.l_lo, c.l_hi);
    if (!empty_box(c.r_lo)) grow(lo, hi, c.r_lo, c.r_hi);
  }
}

__global__ __launch_bounds__(kRefitBlock) void refit_fit_level_kernel(
    const RefitJob* __restrict__ jobs, int h) {
  const RefitJob J = jobs[blockIdx.y];
  if (h > J.height) return;
  const uint32_t begin = J.level[h], end = J.level[h + 1];
  for (uint32_t k = begin + blockIdx.x * kRefitBlock + threadIdx.x; k < end;
       k += gridDim.x * kRefitBlock) {
    const uint32_t node = J.order[k];
    if (node >= J.nnodes) continue;
    const BvhNode old = J.nodes[node];
    BvhNode out = old;
    fit_child(J, old, 0, out.l_lo, out.l_hi);
    fit_child(J, old, 1, out.r_lo, out.r_hi);
    J.s_nodes[node] = out;
  }
}

// make_qgrid: min / max over the padded non-empty child boxes of the fitted
// nodes (one workgroup per slot, a fixed-shape reduction), then the grid's
// double arithmetic in one thread.
__global__ __launch_bounds__(kRefitBlock) void refit_grid_kernel(const RefitJob* __restrict__ jobs,
                                                                 uint32_t* __restrict__ status) {
  const RefitJob J = jobs[blockIdx.x];
  __shared__ float s_lo[3][kRefitBlock], s_hi[3][kRefitBlock];
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  float lo[3] = {pos_inf(), pos_inf(), pos_inf()}, hi[3] = {-pos_inf(), -pos_inf(), -pos_inf()};
  bool bad = false;
  for (uint32_t k = threadIdx.x; k < J.nnodes; k += kRefitBlock) {
    const BvhNode n = J.s_nodes[k];
    for (int side = 0; side < 2; ++side) {
      float bl[3], bh[3];
      for (int j = 0; j < 3; ++j) {
        bl[j] = side_lo(n, side)[j];
        bh[j] = side_hi(n, side)[j];
      }
      if (empty_box(bl)) continue;
      pad_box(bl, bh);
      for (int j = 0; j < 3; ++j) bad = bad || !finite_f(bl[j]) || !finite_f(bh[j]);
      grow(lo, hi, bl, bh);
    }
  }
  if (bad) s_bad = 1;
  for (int j = 0; j < 3; ++j) {
    s_lo[j][threadIdx.x] = lo[j];
    s_hi[j][threadIdx.x] = hi[j];
  }
  __syncthreads();
  for (int w = kRefitBlock / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w)
      for (int j = 0; j < 3; ++j) {
        s_lo[j][threadIdx.x] = fminf(s_lo[j][threadIdx.x], s_lo[j][threadIdx.x + w]);
        s_hi[j][threadIdx.x] = fmaxf(s_hi[j][threadIdx.x], s_hi[j][threadIdx.x + w]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    QGrid g{};
    bool ok = !s_bad;
    const bool any = s_lo[0][0] <= s_hi[0][0];
    for (int j = 0; j < 3; ++j)
      ok = qgrid_axis(s_lo[j][0], s_hi[j][0], any, &g.base[j], &g.scale[j]) && ok;
    *J.s_grid = g;
    if (!ok) atomicOr(&status[blockIdx.x], kBadGrid);
  }
}

// One thread per QNode4 child: quant_box of its source BVH2 child box (padded)
// on the new grid; the child refs are the slot's.
__global__ __launch_bounds__(kRefitBlock) void refit_quant_kernel(const RefitJob* __restrict__ jobs,
                                                                  uint32_t* __restrict__ status) {
  const RefitJob J = jobs[blockIdx.y];
  const QGrid g = *J.s_grid;
  bool bad = false;
  for (uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x; i < 4 * J.nq;
       i += gridDim.x * kRefitBlock) {
    const uint32_t qi = i >> 2, c = i & 3;
    const int32_t src = J.qsrc[i];
    QNode4* out = J.s_q + qi;
    out->child[c] = slot_qnode(J, qi)->child[c];
    uint16_t q[6] = {0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF};
    if (src >= 0 && uint32_t(src >> 1) < J.nnodes) {
      const BvhNode& n = J.s_nodes[src >> 1];
      float bl[3], bh[3];
      for (int j = 0; j < 3; ++j) {
        bl[j] = side_lo(n, src & 1)[j];
        bh[j] = side_hi(n, src & 1)[j];
      }
      pad_box(bl, bh);
      for (int j = 0; j < 3; ++j)
        if (!(g.scale[j] > 0.f) ||
            !quant_axis(g.base[j], g.scale[j], bl[j], bh[j], &q[j], &q[3 + j]))
          bad = true;
    }
    for (int j = 0; j < 6; ++j) out->q[6 * c + j] = q[j];
  }
  if (bad) atomicOr(&status[blockIdx.y], kBadQuant);
}

// scratch -> slot: padded nodes, QNode4s (stored backwards in front of the
// nodes), the grid, the normals and the exact bounds.
__global__ __launch_bounds__(kRefitBlock) void refit_commit_kernel(const RefitJob* __restrict__ jobs,
                                                                   float* __restrict__ bounds) {
  const RefitJob J = jobs[blockIdx.y];
  const uint32_t tid = blockIdx.x * kRefitBlock + threadIdx.x, stride = gridDim.x * kRefitBlock;
  for (uint32_t k = tid; k < J.nnodes; k += stride) {
    BvhNode n = J.s_nodes[k];
    pad_box(n.l_lo, n.l_hi);
    pad_box(n.r_lo, n.r_hi);
    J.nodes[k] = n;
  }
  for (uint32_t k = tid; k < J.nq; k += stride) *slot_qnode(J, k) = J.s_q[k];
  if (J.normals)
    for (size_t k = tid; k < 3 * size_t(J.nverts); k += stride) J.normals[k] = J.vnormals[k];
  if (tid == 0) {
    if (J.nq)
      *reinterpret_cast<QGrid*>(reinterpret_cast<char*>(J.nodes) - sizeof(QGrid)) = *J.s_grid;
    if (bounds) {
      float lo[3] = {pos_inf(), pos_inf(), pos_inf()};
      float hi[3] = {-pos_inf(), -pos_inf(), -pos_inf()};
      if (J.nnodes) {
        const BvhNode& r = J.s_nodes[0];
        if (!empty_box(r.l_lo)) grow(lo, hi, r.l_lo, r.l_hi);
        if (!empty_box(r.r_lo)) grow(lo, hi, r.r_lo, r.r_hi);
      }
      for (int j = 0; j < 3; ++j) {
        bounds[6 * blockIdx.y + j] = lo[j];
        bounds[6 * blockIdx.y + 3 + j] = hi[j];
      }
    }
  }
}

// spray_rt_slot_sah: per-node terms in double, thread t sums nodes t, t + 256,
// ... in that order, then a fixed-shape tree over the 256 partial sums.
__global__ __launch_bounds__(kRefitBlock) void slot_sah_kernel(const BvhNode* __restrict__ nodes,
                                                               uint32_t nnodes,
                                                               double* __restrict__ out) {
  __shared__ double s_sum[kRefitBlock];
  double sum = 0.0;
  for (uint32_t k = threadIdx.x; k < nnodes; k += kRefitBlock) {
    const BvhNode n = nodes[k];
    for (int side = 0; side < 2; ++side) {
      const float* lo = side_lo(n, side);
      if (empty_box(lo)) continue;
      const int32_t ref = side ? n.right : n.left;
      uint32_t first = 0, count = 1;
      if (ref < 0) leaf_range(ref, &first, &count);
      sum += double(half_area(lo, side_hi(n, side))) * double(count);
    }
  }
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (int w = kRefitBlock / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) s_sum[threadIdx.x] = s_sum[threadIdx.x] + s_sum[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float lo[3] = {pos_inf(), pos_inf(), pos_inf()}, hi[3] = {-pos_inf(), -pos_inf(), -pos_inf()};
    if (nnodes) {
      const BvhNode& r = nodes[0];
      if (!empty_box(r.l_lo)) grow(lo, hi, r.l_lo, r.l_hi);
      if (!empty_box(r.r_lo)) grow(lo, hi, r.r_lo, r.r_hi);
    }
    *out = nnodes ? s_sum[0] / double(half_area(lo, hi)) : 0.0;
  }
}

dim3 grid_for(uint32_t items, int njobs) {
  uint32_t gx = (items + kRefitBlock - 1) / kRefitBlock;
  if (gx < 1) gx = 1;
  if (gx > kMaxGridX) gx = kMaxGridX;
  return dim3(gx, unsigned(njobs), 1);
}

}  // namespace

hipError_t launch_refit_check_tris(hipStream_t s, const RefitJob* jobs, int njobs,
                                   uint32_t max_tris, uint32_t* status) {
  hipLaunchKernelGGL(refit_tris_kernel<false>, grid_for(max_tris, njobs), dim3(kRefitBlock), 0, s,
                     jobs, status);
  return hipGetLastError();
}

hipError_t launch_refit_fit_level(hipStream_t s, const RefitJob* jobs, int njobs, int h,
                                  uint32_t max_level_nodes) {
  hipLaunchKernelGGL(refit_fit_level_kernel, grid_for(max_level_nodes, njobs), dim3(kRefitBlock),
                     0, s, jobs, h);
  return hipGetLastError();
}

hipError_t launch_refit_grid(hipStream_t s, const RefitJob* jobs, int njobs, uint32_t* status) {
  hipLaunchKernelGGL(refit_grid_kernel, dim3(unsigned(njobs)), dim3(kRefitBlock), 0, s, jobs,
                     status);
  return hipGetLastError();
}

hipError_t launch_refit_quant(hipStream_t s, const RefitJob* jobs, int njobs, uint32_t max_nq,
                              uint32_t* status) {
  hipLaunchKernelGGL(refit_quant_kernel, grid_for(4 * max_nq, njobs), dim3(kRefitBlock), 0, s,
                     jobs, status);
  return hipGetLastError();
}

hipError_t launch_refit_commit(hipStream_t s, const RefitJob* jobs, int njobs,
                               uint32_t max_nodes, uint32_t max_tris, uint32_t max_verts,
                               float* bounds) {
  uint32_t items = max_nodes;
  const uint64_t nfloats = 3 * uint64_t(max_verts);
  if (nfloats > items) items = nfloats > (1u << 30) ? (1u << 30) : uint32_t(nfloats);
  hipLaunchKernelGGL(refit_commit_kernel, grid_for(items, njobs), dim3(kRefitBlock), 0, s, jobs,
                     bounds);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(refit_tris_kernel<true>, grid_for(max_tris, njobs), dim3(kRefitBlock), 0, s,
                     jobs, static_cast<uint32_t*>(nullptr));
  return hipGetLastError();
}

hipError_t launch_slot_sah(hipStream_t s, const BvhNode* nodes, uint32_t nnodes, double* out) {
  hipLaunchKernelGGL(slot_sah_kernel, dim3(1), dim3(kRefitBlock), 0, s, nodes, nnodes, out);
  return hipGetLastError();
}

}  // namespace spray_rt
