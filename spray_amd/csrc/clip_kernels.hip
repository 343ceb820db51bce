// clip_kernels.hip -- gfx950 kernels of the clip of meshes of hexahedra,
// wedges, pyramids and tets by a level of their scalar field: the surface of
// the kept side of the linear interpolant over the tet split, cap and skin, as
// one indexed triangle mesh.
//
// The cap runs first and whole (cell_kernels.hip, tet_kernels.hip); its sorted
// instance keys, block bases and in-block ids stay where they are.  Then
//
//   count       one thread per cell: surf_count's checks with the values among
//               them; a cell with a kept point counts its faces; block scan.
//               One thread per point clears its use flag.
//   scan, keys, sort, unique   surf_kernels.hip's and tet_kernels.hip's, as
//               they are: alive[] of every face instance, the use flags of the
//               surviving faces' points
//   skin_count  one thread per cell: the mask of its surviving faces and the
//               pieces their triangles give under the kept bits, block-scanned;
//               every cut edge is looked up among the cap's keys, a miss sets
//               a status bit.  One thread per point: flagged and kept, block-
//               scanned into a vertex id within the block
//   scan        tet_scan over two views: pieces, kept points
//   cap         one thread per sorted instance: the first of a run writes pair
//               and t of its vertex
//   swap        one thread per cap face of an inverted mesh: corners 1 and 2
//   verts       one thread per point: position, normal, colour, (p, p) and 0
//               of a used point behind the cap's vertices
//   faces       one thread per cell: the pieces of its surviving faces behind
//               the cap's faces; a corner on a cut edge is the cap vertex a
//               bounded binary search of the pair key finds in skeys
//
// No atomic and no hash decides an index.  Data moves between workgroups only
// across launch boundaries on one stream.  Every store is an ordinary vector
// store bounded by the job tables' capacities; the only atomic is the atomicOr
// of a status word.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "clip_common.h"
#include "clip_kernels.h"

namespace spray_rt {
namespace {

using namespace surf;

// A cell the count pass accepted, read again (surf_kernels.hip's sound_cell).
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

// x[i], i in 0..2, by selects on values read at constant positions: x stays in
// registers
__device__ inline uint32_t pick3(const uint32_t* x, int i) {
  const uint32_t x0 = x[0], x1 = x[1], x2 = x[2];
  return i == 0 ? x0 : i == 1 ? x1 : x2;
}

// The triangles of face f of a sound cell as point indices, false where an
// index is out of range (never in a call whose status the host accepted).
__device__ inline bool face_tris(const SurfJob& J, uint32_t type, const uint32_t* P, int f,
                                 uint32_t* tri, int* nt) {
  const uint32_t face = face_of(type, f);
  const Face F = face_points(face, P);
  const uint32_t pref = P[face_ref(face)];
  bool inside = uint64_t(pref) < J.npoints;
  for (int d = 0; d < 4; ++d) inside = inside && (d >= F.n || uint64_t(F.c[d]) < J.npoints);
  if (!inside) return false;
  *nt = face_triangles(F, J.points, J.points + 3 * size_t(pref), tri);
  return true;
}

// The kept bits of a triangle's three corners.
__device__ inline uint32_t tri_bits(const SurfJob& J, const ClipJob& K, const uint32_t* tri) {
  uint32_t bits = 0;
  for (int v = 0; v < 3; ++v)
    if (clip::kept(J.values[tri[v]], K.isovalue, K.invert)) bits |= 1u << v;
  return bits;
}

// The cap vertex of the pair of points pi != pj: false on a miss.
__device__ inline bool cap_vertex(const SurfJob& J, const TetInst& I, uint32_t pi, uint32_t pj,
                                  uint32_t* id) {
  const uint64_t key = tet::pair_key(pi < pj ? pi : pj, pi < pj ? pj : pi, J.shift);
  const uint32_t at = clip::find_key(I.skeys, I.ninst, key);
  if (at >= I.ninst) return false;
  *id = I.ublock[at / tet::kTetBlock] + I.loc[at];
  return true;
}

__global__ __launch_bounds__(kSurfBlock) void clip_clear_kernel(const SurfJob* __restrict__ jobs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.npblocks) return;
  const uint64_t p = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  if (p < J.npoints) J.pword[p] = 0u;
}

__global__ __launch_bounds__(kSurfBlock) void clip_count_kernel(const SurfJob* __restrict__ jobs,
                                                               const ClipJob* __restrict__ cjobs,
                                                               uint32_t* __restrict__ status) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kSurfBlock];
  const ClipJob K = cjobs[blockIdx.y];
  const uint32_t i = blockIdx.x * kSurfBlock + threadIdx.x;
  uint32_t nf = 0;
  if (i < J.ncells) {
    const Cell C = clip::classify(J.points, J.types, J.offsets, J.conn, J.values, J.cfield,
                                  J.normals, J.npoints, J.nconn, i, K.isovalue, K.invert);
    if (C.status) atomicOr(&status[blockIdx.y], C.status);
    nf = C.nfaces;
  }
  uint32_t total;
  const uint32_t excl = block_excl_scan<kSurfBlock>(nf, s_scan, &total);
  if (i < J.ncells) J.word[i] = cell_word(excl, nf);
  if (threadIdx.x == 0) J.iblock[blockIdx.x] = total;
}

// Cells: the surviving faces' mask and their piece count; the word now holds
// the pieces in front of the cell within its block.
__global__ __launch_bounds__(kSurfBlock) void clip_skin_count_kernel(
    const SurfJob* __restrict__ jobs, const ClipJob* __restrict__ cjobs,
    const TetInst* __restrict__ insts, uint32_t* __restrict__ status) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kSurfBlock];
  const uint32_t i = blockIdx.x * kSurfBlock + threadIdx.x;
  uint32_t mask = 0, np = 0;
  bool miss = false;
  if (i < J.ncells) {
    const uint32_t word = J.word[i];
    const uint32_t nf = word_bits(word);
    uint32_t type, o0;
    if (nf && sound_cell(J, i, &type, &o0) && uint32_t(faces_of(type)) == nf) {
      const ClipJob K = cjobs[blockIdx.y];
      const TetInst I = insts[blockIdx.y];
      const uint32_t* P = J.conn + o0;
      const uint64_t first = uint64_t(J.iblock[blockIdx.x]) + word_loc(word);
      for (int f = 0; f < 6; ++f) {
        if (uint32_t(f) >= nf || first + f >= J.ninst) break;
        if (!J.alive[first + f]) continue;
        uint32_t tri[6];
        int nt;
        if (!face_tris(J, type, P, f, tri, &nt)) break;
        mask |= 1u << f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (t >= nt) break;
          const uint32_t bits = tri_bits(J, K, tri + 3 * t);
          np += uint32_t(clip::piece_count(bits));
          if (bits == 0u || bits == 7u) continue;
          for (int e = 0; e < 3; ++e) {
            const int e1 = e == 2 ? 0 : e + 1;
            if (!(((bits >> e) ^ (bits >> e1)) & 1u)) continue;
            uint32_t id;
            if (!cap_vertex(J, I, pick3(tri + 3 * t, e), pick3(tri + 3 * t, e1), &id)) miss = true;
          }
        }
      }
    }
  }
  if (miss) atomicOr(&status[blockIdx.y], clip::kMiss);
  uint32_t total;
  const uint32_t excl = block_excl_scan<kSurfBlock>(np, s_scan, &total);
  if (i < J.ncells) J.word[i] = clip::skin_word(excl, mask);
  if (threadIdx.x == 0) J.tblock[blockIdx.x] = total;
}

// Points: a vertex of the skin is a kept point of a surviving face.
__global__ __launch_bounds__(kSurfBlock) void clip_point_count_kernel(
    const SurfJob* __restrict__ jobs, const ClipJob* __restrict__ cjobs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.npblocks) return;
  __shared__ uint32_t s_scan[kSurfBlock];
  const ClipJob K = cjobs[blockIdx.y];
  const uint64_t p = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  const uint32_t used =
      p < J.npoints && J.pword[p] && clip::kept(J.values[p], K.isovalue, K.invert) ? 1u : 0u;
  uint32_t total;
  const uint32_t excl = block_excl_scan<kSurfBlock>(used, s_scan, &total);
  if (p < J.npoints) J.pword[p] = point_word(excl, used);
  if (threadIdx.x == 0) J.pblock[blockIdx.x] = total;
}

__global__ __launch_bounds__(tet::kTetBlock) void clip_cap_kernel(
    const SurfJob* __restrict__ jobs, const ClipJob* __restrict__ cjobs,
    const TetInst* __restrict__ insts, const ClipOut* __restrict__ outs) {
  const TetInst I = insts[blockIdx.y];
  if (blockIdx.x >= I.niblocks) return;
  const uint32_t i = blockIdx.x * tet::kTetBlock + threadIdx.x;
  if (i >= I.ninst) return;
  const uint64_t key = I.skeys[i];
  if (i != 0 && I.skeys[i - 1] == key) return;
  const ClipOut O = outs[blockIdx.y];
  const uint64_t id = I.ublock[blockIdx.x] + I.loc[i];
  if (id >= O.ncap_verts || id >= O.cap_verts) return;
  const SurfJob J = jobs[blockIdx.y];
  const uint32_t a = tet::key_a(key, J.shift), b = tet::key_b(key, J.shift);
  if (uint64_t(a) >= J.npoints || uint64_t(b) >= J.npoints) return;
  if (O.pairs) {
    O.pairs[2 * id] = a;
    O.pairs[2 * id + 1] = b;
  }
  if (O.vt) O.vt[id] = tet::pair_t(J.values, a, b, cjobs[blockIdx.y].isovalue);
}

__global__ __launch_bounds__(kSurfBlock) void clip_swap_kernel(const ClipJob* __restrict__ cjobs,
                                                              const ClipOut* __restrict__ outs) {
  if (!cjobs[blockIdx.y].invert) return;
  const ClipOut O = outs[blockIdx.y];
  const uint64_t f = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  if (!O.faces || f >= O.ncap_faces || f >= O.cap_faces) return;
  const uint32_t v1 = O.faces[3 * f + 1], v2 = O.faces[3 * f + 2];
  O.faces[3 * f + 1] = v2;
  O.faces[3 * f + 2] = v1;
}

__global__ __launch_bounds__(kSurfBlock) void clip_verts_kernel(const SurfJob* __restrict__ jobs,
                                                               const ClipOut* __restrict__ outs) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.npblocks) return;
  const uint64_t p = uint64_t(blockIdx.x) * kSurfBlock + threadIdx.x;
  if (p >= J.npoints) return;
  const uint32_t w = J.pword[p];
  if (!pword_used(w)) return;
  const ClipOut O = outs[blockIdx.y];
  const uint64_t id = O.ncap_verts + uint64_t(J.pblock[blockIdx.x]) + pword_loc(w);
  if (id >= O.cap_verts) return;
  if (O.verts)
    for (int ax = 0; ax < 3; ++ax) O.verts[3 * id + ax] = J.points[3 * p + ax];
  if (O.normals)
    for (int ax = 0; ax < 3; ++ax) O.normals[3 * id + ax] = J.normals[3 * p + ax];
  if (O.colors)
    O.colors[id] = point_color(J.cfield, J.ctable, J.clo, J.cscale, J.ntable, J.color, p);
  if (O.pairs) O.pairs[2 * id] = O.pairs[2 * id + 1] = uint32_t(p);
  if (O.vt) O.vt[id] = 0.0f;
}

__global__ __launch_bounds__(kSurfBlock) void clip_faces_kernel(
    const SurfJob* __restrict__ jobs, const ClipJob* __restrict__ cjobs,
    const TetInst* __restrict__ insts, const ClipOut* __restrict__ outs,
    uint32_t* __restrict__ status) {
  const SurfJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t i = blockIdx.x * kSurfBlock + threadIdx.x;
  if (i >= J.ncells) return;
  const uint32_t word = J.word[i];
  const uint32_t mask = clip::skin_mask(word);
  if (!mask) return;
  const ClipOut O = outs[blockIdx.y];
  if (!O.faces) return;
  uint32_t type, o0;
  if (!sound_cell(J, i, &type, &o0)) return;
  const ClipJob K = cjobs[blockIdx.y];
  const TetInst I = insts[blockIdx.y];
  const uint32_t* P = J.conn + o0;
  uint64_t fid = O.ncap_faces + uint64_t(J.tblock[blockIdx.x]) + clip::skin_loc(word);
  const int nf = faces_of(type);
  for (int f = 0; f < 6; ++f) {
    if (f >= nf) break;
    if (!((mask >> f) & 1u)) continue;
    uint32_t tri[6];
    int nt;
    if (!face_tris(J, type, P, f, tri, &nt)) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t >= nt) continue;
      const uint32_t bits = tri_bits(J, K, tri + 3 * t);
      const int np = clip::piece_count(bits);
#pragma unroll
      for (int piece = 0; piece < 2; ++piece) {
        if (piece >= np) continue;
        if (fid < O.cap_faces)
#pragma unroll
          for (int v = 0; v < 3; ++v) {
            int ci, cj;
            clip::piece_corner(bits, piece, v, &ci, &cj);
            const uint32_t pi = pick3(tri + 3 * t, ci), pj = pick3(tri + 3 * t, cj);
            uint32_t id = 0;
            if (ci == cj) {
              id = uint32_t(O.ncap_verts) + J.pblock[pi / kSurfBlock] + pword_loc(J.pword[pi]);
            } else if (!cap_vertex(J, I, pi, pj, &id)) {
              // never after a skin count the host accepted; the miss indexes nothing
              atomicOr(&status[blockIdx.y], clip::kMiss);
              id = 0;
            }
            O.faces[3 * fid + v] = id;
          }
        ++fid;
      }
    }
  }
}

__global__ __launch_bounds__(256) void plane_values_kernel(const float* __restrict__ points,
                                                          uint64_t npoints, Plane plane,
                                                          float* __restrict__ values) {
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  for (uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < npoints; p += stride) {
    const float q[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
    values[p] = clip::plane_value(q, plane.origin, plane.normal);
  }
}

template <int kBlock = kSurfBlock, class K, class... Args>
hipError_t launch(K kernel, hipStream_t s, uint32_t blocks, int njobs, Args... args) {
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(blocks, unsigned(njobs)), dim3(kBlock), 0, s, args...);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_clip_count(hipStream_t s, const SurfJob* jobs, const ClipJob* cjobs, int njobs,
                             uint32_t max_blocks, uint32_t max_pblocks, uint32_t* status) {
  const hipError_t e = launch(clip_clear_kernel, s, max_pblocks, njobs, jobs);
  if (e != hipSuccess) return e;
  return launch(clip_count_kernel, s, max_blocks, njobs, jobs, cjobs, status);
}

hipError_t launch_clip_skin_count(hipStream_t s, const SurfJob* jobs, const ClipJob* cjobs,
                                  const TetInst* insts, int njobs, uint32_t max_blocks,
                                  uint32_t max_pblocks, uint32_t* status) {
  const hipError_t e =
      launch(clip_skin_count_kernel, s, max_blocks, njobs, jobs, cjobs, insts, status);
  if (e != hipSuccess) return e;
  return launch(clip_point_count_kernel, s, max_pblocks, njobs, jobs, cjobs);
}

hipError_t launch_clip_emit(hipStream_t s, const SurfJob* jobs, const ClipJob* cjobs,
                            const TetInst* insts, const ClipOut* outs, int njobs,
                            uint32_t max_blocks, uint32_t max_pblocks, uint32_t max_iblocks,
                            uint32_t max_fblocks, uint32_t* status) {
  hipError_t e =
      launch<tet::kTetBlock>(clip_cap_kernel, s, max_iblocks, njobs, jobs, cjobs, insts, outs);
  if (e != hipSuccess) return e;
  e = launch(clip_swap_kernel, s, max_fblocks, njobs, cjobs, outs);
  if (e != hipSuccess) return e;
  e = launch(clip_verts_kernel, s, max_pblocks, njobs, jobs, outs);
  if (e != hipSuccess) return e;
  return launch(clip_faces_kernel, s, max_blocks, njobs, jobs, cjobs, insts, outs, status);
}

hipError_t launch_plane_values(hipStream_t s, const float* points, uint64_t npoints, Plane plane,
                               float* values) {
  if (!npoints) return hipSuccess;
  const uint64_t want = (npoints + 255) / 256;
  const unsigned blocks = unsigned(want < 16384 ? want : 16384);
  hipLaunchKernelGGL(plane_values_kernel, dim3(blocks), dim3(256), 0, s, points, npoints, plane,
                     values);
  return hipGetLastError();
}

}  // namespace spray_rt
