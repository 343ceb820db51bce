// iso_kernels.hip -- gfx950 kernels of the isosurface extraction: per-domain
// structured grids of scalars to welded, indexed triangle meshes.
//
//   count  one thread per lattice point: the 8 samples of the cell whose
//          minimum corner the point is, the inside mask, the crossing-edge
//          mask, the cell's triangle count, finiteness of the point's sample;
//          a block scan leaves the point's code word and the block's sums
//   scan   one workgroup per grid: block sums to block bases, the totals
//   emit   one thread per lattice point: a vertex (position, normal, color)
//          per crossing edge, the cell's faces; a mapped grid's colour is
//          table[bin(lerp(g[p], g[q], t))] of its colour field g
//          (color_common.h).  The colours-only instantiation does the colour
//          work alone: the two samples of a crossing edge, no cell, no faces
//   colormap_apply, recolor: the per-element map and the batched copy into
//          slots (the bottom of this file)
//
// A point's vertices start at vblock[block] + vloc, its cell's faces at
// fblock[block] + floc; the id of the vertex on an edge is its smaller
// endpoint's first vertex plus the crossing edges of lower type there.  No
// atomic and no hash decides an index: two runs write the same bytes.  Data
// moves between workgroups only across launch boundaries on one stream.
//
// The 8 samples of a thread come through the vector L1 and L2, not an LDS
// tile: blocks are runs of consecutive points (the scan order is the vertex
// order), so a wave's loads are two to four contiguous row segments per
// corner, the +x corner is the neighbouring lane's line, and a 3-D tile with
// a halo would break the linear numbering that makes the block scan the
// ordering.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "block_scan.h"
#include "color_common.h"
#include "iso_common.h"
#include "iso_kernels.h"

namespace spray_rt {
namespace {

using namespace iso;

constexpr int kScanBlock = 512;

struct Point {
  int i, j, k;
  uint32_t valid;
  float f[8];
};

// The cell whose minimum corner is point p: its valid corners' samples.
__device__ inline Point load_point(const IsoJob& J, uint32_t p) {
  Point P;
  const uint32_t nx = uint32_t(J.nx), ny = uint32_t(J.ny);
  const uint32_t row = p / nx;
  P.i = int(p - row * nx);
  P.k = int(row / ny);
  P.j = int(row - uint32_t(P.k) * ny);
  P.valid = valid_corners(P.i, P.j, P.k, J.nx, J.ny, J.nz);
  const size_t sy = nx, sz = size_t(nx) * ny;
  for (int c = 0; c < 8; ++c) {
    P.f[c] = 0.0f;
    if ((P.valid >> c) & 1u)
      P.f[c] = J.values[size_t(p) + size_t(c & 1) + sy * size_t((c >> 1) & 1) + sz * size_t(c >> 2)];
  }
  return P;
}

__global__ __launch_bounds__(kIsoBlock) void iso_count_kernel(const IsoJob* __restrict__ jobs,
                                                             uint32_t* __restrict__ status) {
  const IsoJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kIsoBlock];
  const uint32_t p = blockIdx.x * kIsoBlock + threadIdx.x;
  uint32_t emask = 0, nv = 0, nf = 0;
  if (p < J.npoints) {
    const Point P = load_point(J, p);
    if (!refit::finite_f(P.f[0])) atomicOr(&status[blockIdx.y], kBadSample);
    if (J.cfield && !refit::finite_f(J.cfield[p])) atomicOr(&status[blockIdx.y], kBadColor);
    const uint32_t ins = inside_mask(P.f, P.valid, J.isovalue);
    emask = edge_mask(ins, P.valid);
    nv = uint32_t(popc(emask));
    if (P.valid == 0xFFu) nf = cell_tri_count(ins);
  }
  // both counts in one scan: a block holds at most 1792 vertices and 3072 faces
  uint32_t total;
  const uint32_t excl = block_excl_scan<kIsoBlock>(nv | (nf << 16), s_scan, &total);
  if (p < J.npoints) J.code[p] = code_word(emask, excl & 0xFFFFu, excl >> 16);
  if (threadIdx.x == 0) {
    J.vblock[blockIdx.x] = total & 0xFFFFu;
    J.fblock[blockIdx.x] = total >> 16;
  }
}

__global__ __launch_bounds__(kScanBlock) void iso_scan_kernel(const IsoJob* __restrict__ jobs) {
  const IsoJob J = jobs[blockIdx.x];
  __shared__ uint64_t s_scan[kScanBlock];
  uint64_t cv = 0, cf = 0;  // the same in every thread
  for (uint32_t b0 = 0; b0 < J.nblocks; b0 += kScanBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const bool live = b < J.nblocks;
    // a stride sums to less than 2^20 vertices and 2^21 faces
    const uint64_t v = live ? (uint64_t(J.vblock[b]) | (uint64_t(J.fblock[b]) << 32)) : 0;
    uint64_t total;
    const uint64_t excl = block_excl_scan<kScanBlock>(v, s_scan, &total);
    if (live) {  // bases wrap only in a grid the host rejects by its totals
      J.vblock[b] = uint32_t(cv + (excl & 0xFFFFFFFFu));
      J.fblock[b] = uint32_t(cf + (excl >> 32));
    }
    cv += total & 0xFFFFFFFFu;
    cf += total >> 32;
  }
  if (threadIdx.x == 0) {
    J.rec->nverts = cv;
    J.rec->nfaces = cf;
  }
}

// Corner c of the cell whose minimum corner is point p.
__device__ inline uint32_t corner_point(uint32_t p, int c, uint32_t nx, uint32_t ny) {
  return p + uint32_t(c & 1) + nx * (uint32_t((c >> 1) & 1) + ny * uint32_t(c >> 2));
}

// The mapped colour of the vertex at parameter t of the edge from a point with
// colour sample gp to point q.
__device__ inline uint32_t edge_color(const IsoJob& J, float gp, uint32_t q, float t) {
  return J.ctable[cmap::bin(lerp(gp, J.cfield[q], t), J.clo, J.cscale, J.ntable)];
}

template <bool kColorsOnly>
__global__ __launch_bounds__(kIsoBlock) void iso_emit_kernel(const IsoJob* __restrict__ jobs,
                                                            const IsoOut* __restrict__ outs) {
  const IsoJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t p = blockIdx.x * kIsoBlock + threadIdx.x;
  if (p >= J.npoints) return;
  const uint32_t code = J.code[p];
  const uint32_t emask = code_emask(code);
  const IsoOut O = outs[blockIdx.y];
  const uint32_t nx = uint32_t(J.nx), ny = uint32_t(J.ny);

  if constexpr (kColorsOnly) {
    // ---- a colour per crossing edge: its two samples of either field ----
    if (!emask || !O.colors) return;
    uint64_t vid = uint64_t(J.vblock[blockIdx.x]) + code_vloc(code);
    float f0 = 0.f, g0 = 0.f;
    if (J.cfield) {
      f0 = J.values[p];
      g0 = J.cfield[p];
    }
    for (int type = 0; type < 7; ++type) {
      if (!((emask >> type) & 1u)) continue;
      if (vid < O.cap_verts) {
        uint32_t col = J.color;
        if (J.cfield) {
          const uint32_t q = corner_point(p, type_corner(type), nx, ny);
          col = edge_color(J, g0, q, edge_t(f0, J.values[q], J.isovalue));
        }
        O.colors[vid] = col;
      }
      ++vid;
    }
    return;
  }
  const Point P = load_point(J, p);

  // ---- a vertex per crossing edge ----
  if (emask) {
    uint64_t vid = uint64_t(J.vblock[blockIdx.x]) + code_vloc(code);
    float ga[3] = {0.f, 0.f, 0.f};
    if (O.normals) neg_gradient(J.values, J.nx, J.ny, J.nz, P.i, P.j, P.k, J.spacing, ga);
    const bool mapped = O.colors && J.cfield;
    const float g0 = mapped ? J.cfield[p] : 0.f;
    for (int type = 0; type < 7; ++type) {
      if (!((emask >> type) & 1u)) continue;
      const int c = type_corner(type);
      const float t = edge_t(P.f[0], P.f[c], J.isovalue);
      if (vid < O.cap_verts) {
        if (O.verts) {
          float pos[3];
          edge_vertex(J.origin, J.spacing, P.i, P.j, P.k, type, t, pos);
          for (int ax = 0; ax < 3; ++ax) O.verts[3 * vid + ax] = pos[ax];
        }
        if (O.normals) {
          float gb[3];
          neg_gradient(J.values, J.nx, J.ny, J.nz, P.i + (c & 1), P.j + ((c >> 1) & 1),
                       P.k + (c >> 2), J.spacing, gb);
          for (int ax = 0; ax < 3; ++ax) O.normals[3 * vid + ax] = lerp(ga[ax], gb[ax], t);
        }
        if (O.colors)
          O.colors[vid] = mapped ? edge_color(J, g0, corner_point(p, c, nx, ny), t) : J.color;
      }
      ++vid;
    }
  }

  // ---- the cell's faces ----
  if (P.valid != 0xFFu || !O.faces) return;
  const uint32_t ins = inside_mask(P.f, P.valid, J.isovalue);
  if (ins == 0 || ins == 0xFFu) return;
  // first vertex and crossing mask of corners 0..6 (corner 7 starts no edge of the cell)
  uint32_t vb[7], em[7];
  for (int c = 0; c < 7; ++c) {
    const uint32_t q = corner_point(p, c, nx, ny);
    const uint32_t cq = c ? J.code[q] : code;
    vb[c] = J.vblock[q / kIsoBlock] + code_vloc(cq);
    em[c] = code_emask(cq);
  }
  uint64_t fid = uint64_t(J.fblock[blockIdx.x]) + code_floc(code);
  for (int tet = 0; tet < 6; ++tet) {
    int T[4];
    tet_corners(tet, T);
    uint8_t e[2][3];
    const int nt = tet_triangles(tet_signs(T, ins), tet_odd(tet), e);
    for (int n = 0; n < nt; ++n) {
      if (fid < O.cap_faces)
        for (int v = 0; v < 3; ++v) {
          const int cu = T[e[n][v] >> 2], cv = T[e[n][v] & 3];
          const int type = diff_type(cu ^ cv);
          // a select, not a dynamic index: vb and em stay in registers
          uint32_t base = vb[0], mask = em[0];
          for (int c = 1; c < 7; ++c)
            if (c == cu) {
              base = vb[c];
              mask = em[c];
            }
          O.faces[3 * fid + v] = base + uint32_t(popc(mask & ((1u << type) - 1u)));
        }
      ++fid;
    }
  }
}

// ---- colour maps over per-vertex data, new colours for resident slots ----

constexpr int kApplyBlock = 256;

__device__ inline uint32_t map_one(float g, const uint32_t* __restrict__ table, int ntable,
                                   float lo, float scale, uint32_t* bad) {
  if (!refit::finite_f(g)) *bad = 1;
  return table[cmap::bin(g, lo, scale, ntable)];
}

// Elements [head, head + 4 nvec) as 16-B vectors (both arrays are 16-B aligned
// there), the head and the tail by elements: thread t takes vector t and the
// four rest elements 4 t .. 4 t + 3 (the rest: head, then tail).
__global__ __launch_bounds__(kApplyBlock) void colormap_apply_kernel(
    const float* __restrict__ scalars, size_t n, size_t head, size_t nvec,
    const uint32_t* __restrict__ table, int ntable, float lo, float scale,
    uint32_t* __restrict__ colors, uint32_t* __restrict__ status) {
  const size_t t = size_t(blockIdx.x) * kApplyBlock + threadIdx.x;
  uint32_t bad = 0;
  if (t < nvec) {
    const float4 g = *reinterpret_cast<const float4*>(scalars + head + 4 * t);
    uint4 c;
    c.x = map_one(g.x, table, ntable, lo, scale, &bad);
    c.y = map_one(g.y, table, ntable, lo, scale, &bad);
    c.z = map_one(g.z, table, ntable, lo, scale, &bad);
    c.w = map_one(g.w, table, ntable, lo, scale, &bad);
    *reinterpret_cast<uint4*>(colors + head + 4 * t) = c;
  }
  const size_t rest = n - 4 * nvec;
  for (int k = 0; k < 4; ++k) {
    const size_t r = 4 * t + size_t(k);
    if (r >= rest) break;
    const size_t e = r < head ? r : r + 4 * nvec;
    colors[e] = map_one(scalars[e], table, ntable, lo, scale, &bad);
  }
  if (bad) atomicOr(status, cmap::kBadScalar);
}

// Four colours per thread, block (x, job); the slots' arrays are 256-B
// aligned, the sources the caller's: by elements.
__global__ __launch_bounds__(kApplyBlock) void recolor_kernel(const RecolorJob* __restrict__ jobs) {
  const RecolorJob J = jobs[blockIdx.y];
  const uint32_t base = blockIdx.x * (4 * kApplyBlock) + threadIdx.x;
  for (int k = 0; k < 4; ++k) {
    const uint32_t i = base + uint32_t(k) * kApplyBlock;
    if (i < J.n) J.dst[i] = J.src[i];
  }
}

}  // namespace

hipError_t launch_iso_count(hipStream_t s, const IsoJob* jobs, int njobs, uint32_t max_blocks,
                            uint32_t* status) {
  hipLaunchKernelGGL(iso_count_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kIsoBlock), 0, s,
                     jobs, status);
  return hipGetLastError();
}

hipError_t launch_iso_scan(hipStream_t s, const IsoJob* jobs, int njobs) {
  hipLaunchKernelGGL(iso_scan_kernel, dim3(unsigned(njobs)), dim3(kScanBlock), 0, s, jobs);
  return hipGetLastError();
}

hipError_t launch_iso_emit(hipStream_t s, const IsoJob* jobs, const IsoOut* outs, int njobs,
                           uint32_t max_blocks, bool colors_only) {
  const dim3 grid(max_blocks, unsigned(njobs));
  if (colors_only)
    hipLaunchKernelGGL(iso_emit_kernel<true>, grid, dim3(kIsoBlock), 0, s, jobs, outs);
  else
    hipLaunchKernelGGL(iso_emit_kernel<false>, grid, dim3(kIsoBlock), 0, s, jobs, outs);
  return hipGetLastError();
}

hipError_t launch_colormap_apply(hipStream_t s, const float* scalars, size_t n,
                                 const uint32_t* table, int ntable, float lo, float scale,
                                 uint32_t* colors, uint32_t* status) {
  if (n == 0) return hipSuccess;
  // 16-B accesses where both arrays reach 16-B alignment at the same element
  const uintptr_t a = reinterpret_cast<uintptr_t>(scalars), b = reinterpret_cast<uintptr_t>(colors);
  const bool vec = ((a ^ b) & 15u) == 0 && (a & 3u) == 0;
  size_t head = n, nvec = 0;
  if (vec) {
    head = std::min<size_t>(n, ((16 - (a & 15u)) & 15u) / 4);
    nvec = (n - head) / 4;
  }
  // threads: one per vector, and one per four elements of the scalar rest
  const size_t rest = n - 4 * nvec, threads = std::max(nvec, (rest + 3) / 4);
  const unsigned blocks = unsigned((threads + kApplyBlock - 1) / kApplyBlock);
  hipLaunchKernelGGL(colormap_apply_kernel, dim3(blocks), dim3(kApplyBlock), 0, s, scalars, n,
                     head, nvec, table, ntable, lo, scale, colors, status);
  return hipGetLastError();
}

hipError_t launch_recolor(hipStream_t s, const RecolorJob* jobs, int njobs, uint32_t max_n) {
  if (max_n == 0) return hipSuccess;
  const unsigned blocks = (max_n + 4 * kApplyBlock - 1) / (4 * kApplyBlock);
  hipLaunchKernelGGL(recolor_kernel, dim3(blocks, unsigned(njobs)), dim3(kApplyBlock), 0, s, jobs);
  return hipGetLastError();
}

}  // namespace spray_rt
