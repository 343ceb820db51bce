// tet_kernels.hip -- gfx950 kernels of the isosurface extraction from
// unstructured tetrahedral meshes: points, tets and samples to welded, indexed
// triangle meshes.
//
//   count   one thread per tet: the 4 indices (each < npoints), the 4 samples,
//           finiteness of what the call reads of the 4 points, the inside
//           bits, the parity from the geometry; a block scan of the
//           crossing-edge and triangle counts leaves the tet's word and the
//           block's sums
//   scan    one workgroup per mesh: block sums to block bases, the totals
//   keys    one thread per tet: (pair key, instance index) of every crossing
//           walk edge at the tet's scanned offset
//   sort    rocPRIM segmented radix sort of the pairs, one segment per mesh
//   unique  one thread per sorted instance: first-of-run flags, block-scanned
//   scan    ... of the distinct keys per block: the vertex counts
//   verts   one thread per sorted instance: its vertex id to vid[instance];
//           the first of a run writes position, normal and colour of its pair
//   faces   one thread per tet: iso::tet_triangles, each corner
//           vid[tet's offset + rank of the walk edge among its crossing edges]
//
// Equal keys all get the same id, so the sort's order among them does not
// matter; no atomic and no hash decides an index, and two runs write the same
// bytes.  Data moves between workgroups only across launch boundaries on one
// stream.  Every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "block_scan.h"
#include "tet_common.h"
#include "tet_kernels.h"

namespace spray_rt {
namespace {

using namespace tet;

constexpr int kScanBlock = 512;

__global__ __launch_bounds__(kTetBlock) void tet_count_kernel(const TetJob* __restrict__ jobs,
                                                             uint32_t* __restrict__ status) {
  const TetJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kTetBlock];
  const uint32_t t = blockIdx.x * kTetBlock + threadIdx.x;
  uint32_t signs = 0, odd = 0, ne = 0, nf = 0;
  if (t < J.ntets) {
    const Corner C =
        classify(J.points, J.tets, J.values, J.cfield, J.normals, J.npoints, t, J.isovalue);
    if (C.status) atomicOr(&status[blockIdx.y], C.status);
    signs = C.signs;
    odd = C.odd;
    ne = uint32_t(iso::popc(cross_mask(signs)));
    nf = uint32_t(iso::tet_tri_count(signs));
  }
  // both counts in one scan: a block holds at most 1024 instances and 512 faces
  uint32_t total;
  const uint32_t excl = block_excl_scan<kTetBlock>(ne | (nf << 16), s_scan, &total);
  if (t < J.ntets) J.word[t] = tet_word(signs, odd, excl & 0xFFFFu, excl >> 16);
  if (threadIdx.x == 0) {
    J.eblock[blockIdx.x] = total & 0xFFFFu;
    J.fblock[blockIdx.x] = total >> 16;
  }
}

// kUnique: the distinct keys per block of sorted instances (ublock) to first
// vertices and rec->nverts; else eblock / fblock to first instances / faces
// and rec->ninst / nfaces.
template <bool kUnique>
__global__ __launch_bounds__(kScanBlock) void tet_scan_kernel(const TetJob* __restrict__ jobs,
                                                             const TetInst* __restrict__ insts) {
  const TetJob J = jobs[blockIdx.x];
  __shared__ uint64_t s_scan[kScanBlock];
  uint32_t *lo = J.eblock, *hi = J.fblock;
  uint32_t nblocks = J.nblocks;
  if constexpr (kUnique) {
    const TetInst I = insts[blockIdx.x];
    lo = I.ublock;
    hi = nullptr;
    nblocks = I.niblocks;
  }
  uint64_t clo = 0, chi = 0;  // the same in every thread
  for (uint32_t b0 = 0; b0 < nblocks; b0 += kScanBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const bool live = b < nblocks;
    // a stride sums to less than 2^20 of either
    uint64_t v = live ? uint64_t(lo[b]) : 0;
    if (live && hi) v |= uint64_t(hi[b]) << 32;
    uint64_t total;
    const uint64_t excl = block_excl_scan<kScanBlock>(v, s_scan, &total);
    if (live) {  // bases wrap only in a call the host rejects by its totals
      lo[b] = uint32_t(clo + (excl & 0xFFFFFFFFu));
      if (hi) hi[b] = uint32_t(chi + (excl >> 32));
    }
    clo += total & 0xFFFFFFFFu;
    chi += total >> 32;
  }
  if (threadIdx.x == 0) {
    if constexpr (kUnique) {
      J.rec->nverts = clo;
    } else {
      J.rec->ninst = clo;
      J.rec->nfaces = chi;
    }
  }
}

__global__ __launch_bounds__(kTetBlock) void tet_keys_kernel(const TetJob* __restrict__ jobs,
                                                            const TetInst* __restrict__ insts) {
  const TetJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t t = blockIdx.x * kTetBlock + threadIdx.x;
  if (t >= J.ntets) return;
  const uint32_t word = J.word[t];
  const uint32_t mask = cross_mask(word_signs(word));
  if (!mask) return;
  const TetInst I = insts[blockIdx.y];
  uint32_t i = J.eblock[blockIdx.x] + word_eloc(word);
  uint32_t p[4];  // by elements: the caller's array may be 4-B aligned only
  for (int v = 0; v < 4; ++v) p[v] = J.tets[4 * size_t(t) + v];
  for (int k = 0; k < 6; ++k) {
    if (!((mask >> k) & 1u)) continue;
    // a select, not a dynamic index: p stays in registers
    uint32_t pu = p[0], pw = p[1];
    for (int v = 1; v < 4; ++v) {
      if (v == edge_u(k)) pu = p[v];
      if (v == edge_w(k)) pw = p[v];
    }
    if (i < I.ninst) {
      I.keys[i] = pair_key(pu < pw ? pu : pw, pu < pw ? pw : pu, J.shift);
      I.inst[i] = i;
    }
    ++i;
  }
}

__global__ __launch_bounds__(kTetBlock) void tet_unique_kernel(const TetInst* __restrict__ insts) {
  const TetInst I = insts[blockIdx.y];
  if (blockIdx.x >= I.niblocks) return;
  __shared__ uint32_t s_scan[kTetBlock];
  const uint32_t i = blockIdx.x * kTetBlock + threadIdx.x;
  uint32_t first = 0;
  if (i < I.ninst) first = (i == 0 || I.skeys[i] != I.skeys[i - 1]) ? 1u : 0u;
  uint32_t total;
  const uint32_t excl = block_excl_scan<kTetBlock>(first, s_scan, &total);
  // a run that started in an earlier block continues the vertex before the
  // block's first: excl + first - 1 wraps to -1 there, and the base undoes it
  if (i < I.ninst) I.loc[i] = excl + first - 1u;
  if (threadIdx.x == 0) I.ublock[blockIdx.x] = total;
}

__global__ __launch_bounds__(kTetBlock) void tet_verts_kernel(const TetJob* __restrict__ jobs,
                                                             const TetInst* __restrict__ insts,
                                                             const TetOut* __restrict__ outs) {
  const TetInst I = insts[blockIdx.y];
  if (blockIdx.x >= I.niblocks) return;
  const uint32_t i = blockIdx.x * kTetBlock + threadIdx.x;
  if (i >= I.ninst) return;
  const uint32_t id = I.ublock[blockIdx.x] + I.loc[i];
  const uint32_t from = I.sinst[i];
  if (from < I.ninst) I.vid[from] = id;
  const uint64_t key = I.skeys[i];
  if (i != 0 && I.skeys[i - 1] == key) return;
  const TetOut O = outs[blockIdx.y];
  if (id >= O.cap_verts) return;
  const TetJob J = jobs[blockIdx.y];
  const uint32_t a = key_a(key, J.shift), b = key_b(key, J.shift);
  const float t = pair_t(J.values, a, b, J.isovalue);
  if (O.verts) {
    float pos[3];
    pair_lerp3(J.points, a, b, t, pos);
    for (int ax = 0; ax < 3; ++ax) O.verts[3 * size_t(id) + ax] = pos[ax];
  }
  if (O.normals) {
    float nrm[3];
    pair_lerp3(J.normals, a, b, t, nrm);
    for (int ax = 0; ax < 3; ++ax) O.normals[3 * size_t(id) + ax] = nrm[ax];
  }
  if (O.colors) {
    uint32_t col = J.color;
    if (J.cfield)
      col = J.ctable[cmap::bin(iso::lerp(J.cfield[a], J.cfield[b], t), J.clo, J.cscale, J.ntable)];
    O.colors[id] = col;
  }
}

__global__ __launch_bounds__(kTetBlock) void tet_faces_kernel(const TetJob* __restrict__ jobs,
                                                             const TetInst* __restrict__ insts,
                                                             const TetOut* __restrict__ outs) {
  const TetJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t t = blockIdx.x * kTetBlock + threadIdx.x;
  if (t >= J.ntets) return;
  const uint32_t word = J.word[t];
  const uint32_t signs = word_signs(word);
  uint8_t e[2][3];
  const int nt = iso::tet_triangles(signs, word_odd(word), e);
  if (!nt) return;
  const TetOut O = outs[blockIdx.y];
  if (!O.faces) return;
  const TetInst I = insts[blockIdx.y];
  const uint32_t mask = cross_mask(signs);
  const uint32_t base = J.eblock[blockIdx.x] + word_eloc(word);
  uint64_t fid = uint64_t(J.fblock[blockIdx.x]) + word_floc(word);
  for (int n = 0; n < nt; ++n, ++fid) {
    if (fid >= O.cap_faces) continue;
    for (int v = 0; v < 3; ++v) {
      const int k = edge_index(e[n][v]);
      const uint32_t i = base + uint32_t(iso::popc(mask & ((1u << k) - 1u)));
      O.faces[3 * fid + v] = i < I.ninst ? I.vid[i] : 0u;
    }
  }
}

}  // namespace

hipError_t launch_tet_count(hipStream_t s, const TetJob* jobs, int njobs, uint32_t max_blocks,
                            uint32_t* status) {
  if (!max_blocks) return hipSuccess;
  hipLaunchKernelGGL(tet_count_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kTetBlock), 0, s,
                     jobs, status);
  return hipGetLastError();
}

hipError_t launch_tet_scan(hipStream_t s, const TetJob* jobs, const TetInst* insts, int njobs,
                           bool unique) {
  if (unique)
    hipLaunchKernelGGL(tet_scan_kernel<true>, dim3(unsigned(njobs)), dim3(kScanBlock), 0, s, jobs,
                       insts);
  else
    hipLaunchKernelGGL(tet_scan_kernel<false>, dim3(unsigned(njobs)), dim3(kScanBlock), 0, s, jobs,
                       insts);
  return hipGetLastError();
}

hipError_t launch_tet_keys(hipStream_t s, const TetJob* jobs, const TetInst* insts, int njobs,
                           uint32_t max_blocks) {
  if (!max_blocks) return hipSuccess;
  hipLaunchKernelGGL(tet_keys_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kTetBlock), 0, s,
                     jobs, insts);
  return hipGetLastError();
}

hipError_t tet_sort(hipStream_t s, void* tmp, size_t* tmp_bytes, const uint64_t* keys,
                    uint64_t* skeys, const uint32_t* inst, uint32_t* sinst, uint32_t total,
                    int njobs, const uint32_t* offsets, unsigned end_bit) {
  return rocprim::segmented_radix_sort_pairs(tmp, *tmp_bytes, keys, skeys, inst, sinst, total,
                                             unsigned(njobs), offsets, offsets + 1, 0u, end_bit,
                                             s);
}

hipError_t launch_tet_unique(hipStream_t s, const TetInst* insts, int njobs,
                             uint32_t max_iblocks) {
  if (!max_iblocks) return hipSuccess;
  hipLaunchKernelGGL(tet_unique_kernel, dim3(max_iblocks, unsigned(njobs)), dim3(kTetBlock), 0, s,
                     insts);
  return hipGetLastError();
}

hipError_t launch_tet_verts(hipStream_t s, const TetJob* jobs, const TetInst* insts,
                            const TetOut* outs, int njobs, uint32_t max_iblocks) {
  if (!max_iblocks) return hipSuccess;
  hipLaunchKernelGGL(tet_verts_kernel, dim3(max_iblocks, unsigned(njobs)), dim3(kTetBlock), 0, s,
                     jobs, insts, outs);
  return hipGetLastError();
}

hipError_t launch_tet_faces(hipStream_t s, const TetJob* jobs, const TetInst* insts,
                            const TetOut* outs, int njobs, uint32_t max_blocks) {
  if (!max_blocks) return hipSuccess;
  hipLaunchKernelGGL(tet_faces_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kTetBlock), 0, s,
                     jobs, insts, outs);
  return hipGetLastError();
}

}  // namespace spray_rt
