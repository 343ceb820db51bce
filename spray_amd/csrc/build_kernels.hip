// build_kernels.hip -- gfx950 kernels of spray_rt_domains_build: a slot's BVH
// built on the device from a triangle list that is already in HBM.
//
//   check     one thread per triangle: face indices, finiteness, centroid bounds
//   keys      one thread per triangle: (Morton code << 32) | face
//   sort      rocPRIM segmented radix sort, one segment per slot
//   topology  one workgroup per slot: ranges over the sorted triangles split
//             level by level, nodes numbered by a block scan in range order,
//             heights, the refit metadata
//   fit, grid, quant: the refit's kernels (refit_kernels.hip) on the scratch image
//   collapse  one workgroup per slot: the QNode4s level by level, the greedy
//             rule of the host collapse per node, indices by a block scan
//   copy      scratch / caller arrays -> the slot image
//
// Data moves between workgroups only across launch boundaries on one stream;
// inside topology and collapse a slot belongs to one workgroup and levels are
// separated by __syncthreads().  No atomic decides an index or an order: two
// builds of one mesh write the same bytes.  A domain of any size is built
// correctly; a large one only takes longer, its levels walked in strides by
// the one workgroup.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "block_scan.h"
#include "build_common.h"
#include "build_kernels.h"

namespace spray_rt {
namespace {

using namespace refit;
using namespace build;

constexpr int kCodeBlock = 256;
constexpr int kTreeBlock = 512;
constexpr int32_t kEmptyChild = INT32_MIN;  // bvh_build.h kNoChild

__global__ __launch_bounds__(kCodeBlock) void build_check_kernel(const BuildJob* __restrict__ jobs,
                                                                uint32_t* __restrict__ status) {
  const BuildJob J = jobs[blockIdx.y];
  __shared__ float s_lo[3][kCodeBlock], s_hi[3][kCodeBlock];
  float lo[3] = {pos_inf(), pos_inf(), pos_inf()}, hi[3] = {-pos_inf(), -pos_inf(), -pos_inf()};
  uint32_t flags = 0;
  for (uint32_t i = blockIdx.x * kCodeBlock + threadIdx.x; i < J.ntris;
       i += gridDim.x * kCodeBlock) {
    const uint32_t* f = J.faces + 3 * size_t(i);
    const uint32_t f0 = f[0], f1 = f[1], f2 = f[2];
    if (f0 >= J.nverts || f1 >= J.nverts || f2 >= J.nverts) {
      flags |= kBadFace;
      continue;
    }
    const float* a = J.verts + 3 * size_t(f0);
    const float* b = J.verts + 3 * size_t(f1);
    const float* c = J.verts + 3 * size_t(f2);
    float r[12], cen[3];
    if (!tri_record(a, b, c, r)) flags |= kBadVertex;
    tri_centroid(a, b, c, cen);
    grow(lo, hi, cen, cen);
  }
  for (int j = 0; j < 3; ++j) {
    s_lo[j][threadIdx.x] = lo[j];
    s_hi[j][threadIdx.x] = hi[j];
  }
  __syncthreads();
  for (int w = kCodeBlock / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w)
      for (int j = 0; j < 3; ++j) {
        const float l = s_lo[j][threadIdx.x + w], h = s_hi[j][threadIdx.x + w];
        if (l < s_lo[j][threadIdx.x]) s_lo[j][threadIdx.x] = l;
        if (h > s_hi[j][threadIdx.x]) s_hi[j][threadIdx.x] = h;
      }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    J.part[6 * blockIdx.x + threadIdx.x] = s_lo[threadIdx.x][0];
    J.part[6 * blockIdx.x + 3 + threadIdx.x] = s_hi[threadIdx.x][0];
  }
  if (flags) atomicOr(&status[blockIdx.y], flags);
}

// nparts = the check pass' gridDim.x
__global__ __launch_bounds__(kCodeBlock) void build_keys_kernel(const BuildJob* __restrict__ jobs,
                                                               const uint32_t* __restrict__ status,
                                                               uint32_t nparts) {
  const BuildJob J = jobs[blockIdx.y];
  __shared__ float s_cb[6];
  if (threadIdx.x < 6) {
    const bool is_hi = threadIdx.x >= 3;
    float v = is_hi ? -pos_inf() : pos_inf();
    for (uint32_t p = 0; p < nparts; ++p) {
      const float x = J.part[6 * p + threadIdx.x];
      if (is_hi ? x > v : x < v) v = x;
    }
    s_cb[threadIdx.x] = v;
  }
  __syncthreads();
  const bool dead = status[blockIdx.y] != 0;  // its keys are sorted and never read
  float cb[6];
  for (int j = 0; j < 6; ++j) cb[j] = s_cb[j];
  for (uint32_t i = blockIdx.x * kCodeBlock + threadIdx.x; i < J.ntris;
       i += gridDim.x * kCodeBlock) {
    uint64_t key = i;
    if (!dead) {
      const uint32_t* f = J.faces + 3 * size_t(i);
      float cen[3];
      tri_centroid(J.verts + 3 * size_t(f[0]), J.verts + 3 * size_t(f[1]),
                   J.verts + 3 * size_t(f[2]), cen);
      key = sort_key(cen, cb, i);
    }
    J.keys[i] = key;
  }
}

__device__ inline BvhNode zero_node() {
  BvhNode n;
  for (int j = 0; j < 3; ++j) n.l_lo[j] = n.l_hi[j] = n.r_lo[j] = n.r_hi[j] = 0.f;
  n.left = n.right = n.pad0 = n.pad1 = 0;
  return n;
}

__global__ __launch_bounds__(kTreeBlock) void build_topology_kernel(
    const BuildJob* __restrict__ jobs, RefitJob* __restrict__ rjobs,
    const uint32_t* __restrict__ status) {
  const BuildJob J = jobs[blockIdx.x];
  __shared__ uint32_t s_scan[kTreeBlock];
  __shared__ uint32_t s_lbase[kBuildLevels + 2];  // first node of each BFS level
  const uint32_t t = threadIdx.x;
  RefitJob* R = rjobs + blockIdx.x;
  if (status[blockIdx.x] != 0 || J.ntris == 0) {  // nothing to build: an empty slot
    if (t < uint32_t(kRefitLevels)) {
      J.level[t] = 0;
      J.rec->level[t] = 0;
    }
    if (t == 0) {
      J.rec->nnodes = J.rec->nq = 0;
      J.rec->depth = J.rec->height = J.rec->stack_bound = 0;
      R->nnodes = R->ntris = R->nq = 0;
      R->height = 0;
    }
    return;
  }
  for (uint32_t i = t; i < J.ntris; i += kTreeBlock) J.prims[i] = uint32_t(J.sorted[i]);

  int nlev;
  bool too_deep = false;
  if (J.ntris <= uint32_t(kLeafMax)) {
    // the root form of a mesh that is one leaf: left = the leaf, right never hit
    if (t == 0) {
      BvhNode n = zero_node();
      for (int j = 0; j < 3; ++j) n.r_lo[j] = n.r_hi[j] = pos_inf();
      n.left = leaf_ref(0, J.ntris);
      n.right = ~int32_t(0);
      J.nodes[0] = n;
      J.range[0] = make_uint2(0, J.ntris);
      s_lbase[0] = 0;
      s_lbase[1] = 1;
    }
    nlev = 1;
    __syncthreads();
  } else {
    if (t == 0) {
      J.range[0] = make_uint2(0, J.ntris);
      s_lbase[0] = 0;
      s_lbase[1] = 1;
    }
    __syncthreads();
    int L = 0;
    for (;;) {
      const uint32_t base = s_lbase[L], next_base = s_lbase[L + 1], cnt = next_base - base;
      uint32_t carry = 0;
      for (uint32_t k0 = 0; k0 < cnt; k0 += kTreeBlock) {
        const uint32_t k = k0 + t;
        const bool live = k < cnt;
        uint32_t b = 0, m = 0, e = 0, fl = 0, fr = 0;
        if (live) {
          const uint2 r = J.range[base + k];
          b = r.x;
          e = r.y;
          bool forced;
          m = split_range(J.sorted, b, e, L, &forced);
          fl = m - b > uint32_t(kLeafMax);
          fr = e - m > uint32_t(kLeafMax);
        }
        uint32_t total;
        const uint32_t pos =
            next_base + carry + block_excl_scan<kTreeBlock>(fl + fr, s_scan, &total);
        if (live && pos + fl + fr <= J.cap) {
          BvhNode n = zero_node();
          n.left = fl ? int32_t(pos) : leaf_ref(b, m - b);
          n.right = fr ? int32_t(pos + fl) : leaf_ref(m, e - m);
          J.nodes[base + k] = n;
          if (fl) J.range[pos] = make_uint2(b, m);
          if (fr) J.range[pos + fl] = make_uint2(m, e);
        }
        carry += total;
      }
      __syncthreads();
      if (t == 0) s_lbase[L + 2] = next_base + carry;
      __syncthreads();
      ++L;
      if (carry == 0) break;
      if (L >= kMaxDepth) {  // only a mesh of more than 4 * 2^kMaxDepth triangles gets here
        too_deep = true;
        break;
      }
    }
    nlev = L;
  }
  if (too_deep) {  // reported through rec->depth; the later launches see an empty slot
    if (t < uint32_t(kRefitLevels)) {
      J.level[t] = 0;
      J.rec->level[t] = 0;
    }
    if (t == 0) {
      J.rec->nnodes = J.rec->nq = 0;
      J.rec->depth = kMaxDepth + 1;
      J.rec->height = J.rec->stack_bound = 0;
      R->nnodes = R->ntris = R->nq = 0;
      R->height = 0;
    }
    return;
  }
  const uint32_t nn = s_lbase[nlev];

  // heights bottom up: the children of level L sit in level L + 1
  for (int L = nlev - 1; L >= 0; --L) {
    const uint32_t base = s_lbase[L], end = s_lbase[L + 1];
    for (uint32_t k = base + t; k < end; k += kTreeBlock) {
      const BvhNode& n = J.nodes[k];
      const int hl = n.left >= 0 ? J.hgt[n.left] : 0, hr = n.right >= 0 ? J.hgt[n.right] : 0;
      J.hgt[k] = uint8_t(1 + (hl > hr ? hl : hr));
    }
    __syncthreads();
  }

  // refit metadata: group h = the BFS level nlev - h (every inner child of a
  // node lies one level deeper, so in a lower group), nodes ascending within
  for (int L = 0; L < nlev; ++L) {
    const uint32_t base = s_lbase[L], end = s_lbase[L + 1], first = nn - end;
    for (uint32_t k = base + t; k < end; k += kTreeBlock) J.order[first + (k - base)] = k;
  }
  if (t < uint32_t(kRefitLevels)) {
    uint32_t lv = nn;
    if (t == 0)
      lv = 0;
    else if (int(t) <= nlev)
      lv = nn - s_lbase[nlev - int(t) + 1];
    J.level[t] = lv;
    J.rec->level[t] = lv;
  }
  if (t == 0) {
    J.rec->nnodes = nn;
    J.rec->depth = nlev;
    J.rec->height = nlev;
    R->nnodes = nn;
    R->height = nlev;
  }
}

__device__ inline QNode4* scratch_qnode(const BuildJob& J, uint32_t i) {
  return reinterpret_cast<QNode4*>(reinterpret_cast<char*>(J.nodes) - 64 -
                                   size_t(64) * (size_t(i) + 1));
}

__global__ __launch_bounds__(kTreeBlock) void build_collapse_kernel(
    const BuildJob* __restrict__ jobs, RefitJob* __restrict__ rjobs) {
  const BuildJob J = jobs[blockIdx.x];
  __shared__ uint32_t s_scan[kTreeBlock];
  __shared__ int s_bound;
  const uint32_t t = threadIdx.x;
  RefitJob* R = rjobs + blockIdx.x;
  const uint32_t nn = R->nnodes;  // the topology launch's
  if (nn == 0) {
    if (t == 0) {
      J.rec->nq = 0;
      J.rec->stack_bound = 0;
      R->nq = 0;
    }
    return;
  }
  if (t == 0) {
    J.qlist[0] = make_uint2(0, 0);
    s_bound = 0;
  }
  __syncthreads();
  uint32_t base = 0, cnt = 1;
  while (cnt > 0) {
    const uint32_t next_base = base + cnt;
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < cnt; k0 += kTreeBlock) {
      const uint32_t k = k0 + t;
      const bool live = k < cnt;
      Cand cs[4];
      int nc = 0, p2 = 0;
      uint32_t ninner = 0;
      if (live) {
        const uint2 q = J.qlist[base + k];
        nc = collapse_node(J.nodes, J.hgt, int32_t(q.x), int(q.y), cs);
        p2 = int(q.y) + (nc > 0 ? nc - 1 : 0);
        for (int c = 0; c < nc; ++c) ninner += cs[c].ref >= 0;
        atomicMax(&s_bound, p2);
      }
      uint32_t total;
      uint32_t pos = next_base + carry + block_excl_scan<kTreeBlock>(ninner, s_scan, &total);
      if (live && pos + ninner <= J.cap) {
        QNode4* out = scratch_qnode(J, base + k);
        for (int c = 0; c < 4; ++c) {
          int32_t ref = kEmptyChild, src = -1;
          if (c < nc) {
            ref = cs[c].ref;
            src = cs[c].src;
            if (ref >= 0) {
              J.qlist[pos] = make_uint2(uint32_t(ref), uint32_t(p2));
              ref = int32_t(pos++);
            }
          }
          out->child[c] = ref;
          J.qsrc[4 * size_t(base + k) + c] = src;
        }
      }
      carry += total;
    }
    __syncthreads();
    base = next_base;
    cnt = carry;
  }
  if (t == 0) {
    J.rec->nq = base;
    J.rec->stack_bound = s_bound;
    R->nq = base;
  }
}

__global__ __launch_bounds__(kCodeBlock) void build_copy_kernel(const CopyJob* __restrict__ copies) {
  const CopyJob c = copies[blockIdx.y];
  for (size_t k = size_t(blockIdx.x) * kCodeBlock + threadIdx.x; k < c.nwords;
       k += size_t(gridDim.x) * kCodeBlock)
    c.dst[k] = c.src[k];
}

uint32_t blocks_for(size_t items, uint32_t cap) {
  size_t gx = (items + kCodeBlock - 1) / kCodeBlock;
  if (gx < 1) gx = 1;
  if (gx > cap) gx = cap;
  return uint32_t(gx);
}

}  // namespace

hipError_t launch_build_check(hipStream_t s, const BuildJob* jobs, int njobs, uint32_t max_tris,
                              uint32_t* status) {
  hipLaunchKernelGGL(build_check_kernel, dim3(blocks_for(max_tris, kBuildParts), unsigned(njobs)),
                     dim3(kCodeBlock), 0, s, jobs, status);
  return hipGetLastError();
}

hipError_t launch_build_keys(hipStream_t s, const BuildJob* jobs, int njobs, uint32_t max_tris,
                             const uint32_t* status) {
  hipLaunchKernelGGL(build_keys_kernel, dim3(blocks_for(max_tris, 4096), unsigned(njobs)),
                     dim3(kCodeBlock), 0, s, jobs, status, blocks_for(max_tris, kBuildParts));
  return hipGetLastError();
}

hipError_t build_sort(hipStream_t s, void* tmp, size_t* tmp_bytes, const uint64_t* keys,
                      uint64_t* sorted, uint32_t total, int njobs, const uint32_t* offsets) {
  // 30 code bits above the 32 face bits
  return rocprim::segmented_radix_sort_keys(tmp, *tmp_bytes, keys, sorted, total,
                                            unsigned(njobs), offsets, offsets + 1, 0u,
                                            32u + 3u * kCodeBits, s);
}

hipError_t launch_build_topology(hipStream_t s, const BuildJob* jobs, RefitJob* rjobs, int njobs,
                                 const uint32_t* status) {
  hipLaunchKernelGGL(build_topology_kernel, dim3(unsigned(njobs)), dim3(kTreeBlock), 0, s, jobs,
                     rjobs, status);
  return hipGetLastError();
}

hipError_t launch_build_collapse(hipStream_t s, const BuildJob* jobs, RefitJob* rjobs, int njobs) {
  hipLaunchKernelGGL(build_collapse_kernel, dim3(unsigned(njobs)), dim3(kTreeBlock), 0, s, jobs,
                     rjobs);
  return hipGetLastError();
}

hipError_t launch_build_copy(hipStream_t s, const CopyJob* copies, int ncopies, size_t max_words) {
  hipLaunchKernelGGL(build_copy_kernel, dim3(blocks_for(max_words, 1024), unsigned(ncopies)),
                     dim3(kCodeBlock), 0, s, copies);
  return hipGetLastError();
}

}  // namespace spray_rt
