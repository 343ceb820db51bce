// surf_kernels.hip -- gfx950 kernels of the boundary-surface and threshold
// extraction from meshes of hexahedra, wedges, pyramids and tets: the faces of
// the kept cells that no other kept cell shares, as an indexed triangle mesh
// over the points they use.
//
//   count      one thread per cell: type and offsets against each other and
//              nconn, the indices (each < npoints), finiteness of what the
//              call reads of the cell's points, the select; a kept cell counts
//              its 4, 5 or 6 faces; a block scan leaves the cell's word and
//              the block's sum.  One thread per point clears its use flag.
//   scan       tet_scan over a TetJob view: block sums to block bases, the total
//   keys       one thread per kept cell: (face key, cell << 3 | face) of every
//              face at the cell's scanned offset
//   sort       tet_sort: rocPRIM segmented radix sort, one segment per mesh
//   unique     one thread per sorted instance: a key that differs from both
//              neighbours in its segment survives; that thread alone writes
//              the instance's alive byte, and sets the use flags of the face's
//              points (several threads may store the same 1 to a flag)
//   tri_count  one thread per cell: the mask of its surviving faces and their
//              triangle count, block-scanned; one thread per point: its use
//              flag block-scanned into a vertex id within the block
//   scan       tet_scan over two more views: triangles, vertices
//   verts      one thread per point: position, normal, colour and point index
//              of a used point at its vertex id
//   faces      one thread per cell: the triangles of its surviving faces,
//              turned outward, as vertex ids, at the cell's scanned offset
//
// No atomic and no hash decides an index; the sort's order among equal keys
// does not matter, because equal keys all drop.  Data moves between workgroups
// only across launch boundaries on one stream.  Every store is an ordinary
// vector store; the only atomic is the atomicOr of a status word.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "surf_common.h"
#include "surf_kernels.h"

namespace spray_rt {
namespace {

using namespace surf;

// A cell the count pass accepted, read again: its type and first listed index,
// false where the tables no longer say what the word says (never in a call
// whose status the host accepted).
__device__ inline bool sound_cell(const SurfJob& J, uint32_t i, uint32_t* type, uint32_t* o0) {
  const uint32_t t = J.types[i];
  const int np = cell::cell_points(t);
  if (!np) return false;
  const uint32_t o = J.offsets[i];
  if (uint64_t(o) + uint64_t(np) > J.nconn) return false;
  *type = t;
  *o0 = o;
  return true;
}

__global__ __launch_bounds__(kSurfBlock) void surf_clear_kernel(const SurfJob* __restrict__ jobs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.npblocks) return;
  const uint64_t p = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  if (p < J.npoints) J.pword[p] = 0u;
}

__global__ __launch_bounds__(kSurfBlock) void surf_count_kernel(const SurfJob* __restrict__ jobs,
                                                               uint32_t* __restrict__ status) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kSurfBlock];
  const uint32_t i = blockIdx.x * kSurfBlock + threadIdx.x;
  uint32_t nf = 0;
  if (i < J.ncells) {
    const Cell C = classify(J.points, J.types, J.offsets, J.conn, J.values, J.cell_values,
                            J.cfield, J.normals, J.npoints, J.nconn, i, J.mode, J.lo, J.hi);
    if (C.status) atomicOr(&status[blockIdx.y], C.status);
    nf = C.nfaces;
  }
  uint32_t total;
  const uint32_t excl = block_excl_scan<kSurfBlock>(nf, s_scan, &total);
  if (i < J.ncells) J.word[i] = cell_word(excl, nf);
  if (threadIdx.x == 0) J.iblock[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSurfBlock) void surf_keys_kernel(const SurfJob* __restrict__ jobs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t i = blockIdx.x * kSurfBlock + threadIdx.x;
  if (i >= J.ncells) return;
  const uint32_t word = J.word[i];
  const uint32_t nf = word_bits(word);
  if (!nf) return;
  uint32_t type, o0;
  if (!sound_cell(J, i, &type, &o0) || uint32_t(faces_of(type)) != nf) return;
  const uint64_t first = uint64_t(J.iblock[blockIdx.x]) + word_loc(word);
  if (first + nf > J.ninst) return;
  const uint32_t* P = J.conn + o0;
  for (int f = 0; f < 6; ++f) {
    if (uint32_t(f) >= nf) break;
    const Face F = face_points(face_of(type, f), P);
    J.keys[first + f] = face_key(F, J.shift);
    J.vals[first + f] = (i << 3) | uint32_t(f);
  }
}

__global__ __launch_bounds__(kSurfBlock) void surf_unique_kernel(const SurfJob* __restrict__ jobs) {
  const SurfJob J = jobs[blockIdx.y];
  const uint64_t k = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  if (k >= J.ninst) return;
  const uint64_t key = J.skeys[k];
  const bool once =
      (k == 0 || J.skeys[k - 1] != key) && (k + 1 == J.ninst || J.skeys[k + 1] != key);
  const uint32_t val = J.svals[k];
  const uint32_t i = val >> 3, f = val & 7u;
  if (i >= J.ncells) return;
  const uint32_t word = J.word[i];
  if (f >= word_bits(word)) return;
  const uint64_t at = uint64_t(J.iblock[i / kSurfBlock]) + word_loc(word) + f;
  if (at >= J.ninst) return;
  J.alive[at] = once ? uint8_t(1) : uint8_t(0);
  if (!once) return;
  uint32_t type, o0;
  if (!sound_cell(J, i, &type, &o0) || f >= uint32_t(faces_of(type))) return;
  const uint32_t face = face_of(type, int(f));
  const int nc = face_corners(face);
  for (int d = 0; d < 4; ++d) {
    if (d >= nc) break;
    const uint32_t p = J.conn[size_t(o0) + size_t(cell::face_q(face, d))];
    if (uint64_t(p) < J.npoints) J.pword[p] = 1u;
  }
}

// Cells: the surviving faces' mask and triangle count; the word now holds the
// triangles in front of the cell within its block.
__global__ __launch_bounds__(kSurfBlock) void surf_tri_count_kernel(
    const SurfJob* __restrict__ jobs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kSurfBlock];
  const uint32_t i = blockIdx.x * kSurfBlock + threadIdx.x;
  uint32_t mask = 0, nt = 0;
  if (i < J.ncells) {
    const uint32_t word = J.word[i];
    const uint32_t nf = word_bits(word);
    uint32_t type, o0;
    if (nf && sound_cell(J, i, &type, &o0) && uint32_t(faces_of(type)) == nf) {
      const uint64_t first = uint64_t(J.iblock[blockIdx.x]) + word_loc(word);
      for (int f = 0; f < 6; ++f) {
        if (uint32_t(f) >= nf || first + f >= J.ninst) break;
        if (!J.alive[first + f]) continue;
        mask |= 1u << f;
        nt += uint32_t(face_corners(face_of(type, f)) - 2);
      }
    }
  }
  uint32_t total;
  const uint32_t excl = block_excl_scan<kSurfBlock>(nt, s_scan, &total);
  if (i < J.ncells) J.word[i] = cell_word(excl, mask);
  if (threadIdx.x == 0) J.tblock[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSurfBlock) void surf_point_count_kernel(
    const SurfJob* __restrict__ jobs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.npblocks) return;
  __shared__ uint32_t s_scan[kSurfBlock];
  const uint64_t p = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  const uint32_t used = p < J.npoints && J.pword[p] ? 1u : 0u;
  uint32_t total;
  const uint32_t excl = block_excl_scan<kSurfBlock>(used, s_scan, &total);
  if (p < J.npoints) J.pword[p] = point_word(excl, used);
  if (threadIdx.x == 0) J.pblock[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSurfBlock) void surf_verts_kernel(const SurfJob* __restrict__ jobs,
                                                               const SurfOut* __restrict__ outs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.npblocks) return;
  const uint64_t p = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  if (p >= J.npoints) return;
  const uint32_t w = J.pword[p];
  if (!pword_used(w)) return;
  const SurfOut O = outs[blockIdx.y];
  const uint64_t id = uint64_t(J.pblock[blockIdx.x]) + pword_loc(w);
  if (id >= O.cap_verts) return;
  if (O.verts)
    for (int ax = 0; ax < 3; ++ax) O.verts[3 * id + ax] = J.points[3 * p + ax];
  if (O.normals)
    for (int ax = 0; ax < 3; ++ax) O.normals[3 * id + ax] = J.normals[3 * p + ax];
  if (O.colors)
    O.colors[id] = point_color(J.cfield, J.ctable, J.clo, J.cscale, J.ntable, J.color, p);
  if (O.ids) O.ids[id] = uint32_t(p);
}

__global__ __launch_bounds__(kSurfBlock) void surf_faces_kernel(const SurfJob* __restrict__ jobs,
                                                               const SurfOut* __restrict__ outs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t i = blockIdx.x * kSurfBlock + threadIdx.x;
  if (i >= J.ncells) return;
  const uint32_t word = J.word[i];
  const uint32_t mask = word_bits(word);
  if (!mask) return;
  const SurfOut O = outs[blockIdx.y];
  if (!O.faces) return;
  uint32_t type, o0;
  if (!sound_cell(J, i, &type, &o0)) return;
  const uint32_t* P = J.conn + o0;
  uint64_t fid = uint64_t(J.tblock[blockIdx.x]) + word_loc(word);
  const int nf = faces_of(type);
  for (int f = 0; f < 6; ++f) {
    if (f >= nf) break;
    if (!((mask >> f) & 1u)) continue;
    const uint32_t face = face_of(type, f);
    const Face F = face_points(face, P);
    const uint32_t pref = P[face_ref(face)];
    // a cell of a call whose status the host accepted lists points < npoints
    bool inside = uint64_t(pref) < J.npoints;
    for (int d = 0; d < 4; ++d) inside = inside && (d >= F.n || uint64_t(F.c[d]) < J.npoints);
    if (!inside) return;
    uint32_t tri[6];
    const int nt = face_triangles(F, J.points, J.points + 3 * size_t(pref), tri);
    for (int t = 0; t < 2; ++t) {
      if (t >= nt) break;
      if (fid < O.cap_faces)
        for (int v = 0; v < 3; ++v) {
          const uint32_t p = tri[3 * t + v];
          O.faces[3 * fid + v] = J.pblock[p / kSurfBlock] + pword_loc(J.pword[p]);
        }
      ++fid;
    }
  }
}

template <class K, class... Args>
hipError_t launch(K kernel, hipStream_t s, uint32_t blocks, int njobs, Args... args) {
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(blocks, unsigned(njobs)), dim3(kSurfBlock), 0, s, args...);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_surf_count(hipStream_t s, const SurfJob* jobs, int njobs, uint32_t max_blocks,
                             uint32_t max_pblocks, uint32_t* status) {
  const hipError_t e = launch(surf_clear_kernel, s, max_pblocks, njobs, jobs);
  if (e != hipSuccess) return e;
  return launch(surf_count_kernel, s, max_blocks, njobs, jobs, status);
}

hipError_t launch_surf_keys(hipStream_t s, const SurfJob* jobs, int njobs, uint32_t max_blocks) {
  return launch(surf_keys_kernel, s, max_blocks, njobs, jobs);
}

hipError_t launch_surf_unique(hipStream_t s, const SurfJob* jobs, int njobs,
                              uint32_t max_iblocks) {
  return launch(surf_unique_kernel, s, max_iblocks, njobs, jobs);
}

hipError_t launch_surf_tri_count(hipStream_t s, const SurfJob* jobs, int njobs,
                                 uint32_t max_blocks, uint32_t max_pblocks) {
  const hipError_t e = launch(surf_tri_count_kernel, s, max_blocks, njobs, jobs);
  if (e != hipSuccess) return e;
  return launch(surf_point_count_kernel, s, max_pblocks, njobs, jobs);
}

hipError_t launch_surf_emit(hipStream_t s, const SurfJob* jobs, const SurfOut* outs, int njobs,
                            uint32_t max_blocks, uint32_t max_pblocks) {
  const hipError_t e = launch(surf_verts_kernel, s, max_pblocks, njobs, jobs, outs);
  if (e != hipSuccess) return e;
  return launch(surf_faces_kernel, s, max_blocks, njobs, jobs, outs);
}

}  // namespace spray_rt
