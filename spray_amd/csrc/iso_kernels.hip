// iso_kernels.hip -- gfx950 kernels of the isosurface extraction: per-domain
// structured grids of scalars to welded, indexed triangle meshes.
//
//   count  one thread per lattice point: the 8 samples of the cell whose
//          minimum corner the point is, the inside mask, the crossing-edge
//          mask, the cell's triangle count, finiteness of the point's sample;
//          a block scan leaves the point's code word and the block's sums
//   scan   one workgroup per grid: block sums to block bases, the totals
//   emit   one thread per lattice point: a vertex (position, normal, color)
//          per crossing edge, the cell's faces
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

#include "block_scan.h"
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

__global__ __launch_bounds__(kIsoBlock) void iso_emit_kernel(const IsoJob* __restrict__ jobs,
                                                            const IsoOut* __restrict__ outs) {
  const IsoJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t p = blockIdx.x * kIsoBlock + threadIdx.x;
  if (p >= J.npoints) return;
  const uint32_t code = J.code[p];
  const uint32_t emask = code_emask(code);
  const IsoOut O = outs[blockIdx.y];
  const Point P = load_point(J, p);
  const uint32_t nx = uint32_t(J.nx), ny = uint32_t(J.ny);

  // ---- a vertex per crossing edge ----
  if (emask) {
    uint64_t vid = uint64_t(J.vblock[blockIdx.x]) + code_vloc(code);
    float ga[3] = {0.f, 0.f, 0.f};
    if (O.normals) neg_gradient(J.values, J.nx, J.ny, J.nz, P.i, P.j, P.k, J.spacing, ga);
    for (int type = 0; type < 7; ++type) {
      if (!((emask >> type) & 1u)) continue;
      const int c = type_corner(type);
      const float t = edge_t(P.f[0], P.f[c], J.isovalue);
      if (vid < O.cap_verts) {
        float pos[3];
        edge_vertex(J.origin, J.spacing, P.i, P.j, P.k, type, t, pos);
        for (int ax = 0; ax < 3; ++ax) O.verts[3 * vid + ax] = pos[ax];
        if (O.normals) {
          float gb[3];
          neg_gradient(J.values, J.nx, J.ny, J.nz, P.i + (c & 1), P.j + ((c >> 1) & 1),
                       P.k + (c >> 2), J.spacing, gb);
          for (int ax = 0; ax < 3; ++ax) O.normals[3 * vid + ax] = lerp(ga[ax], gb[ax], t);
        }
        if (O.colors) O.colors[vid] = J.color;
      }
      ++vid;
    }
  }

  // ---- the cell's faces ----
  if (P.valid != 0xFFu) return;
  const uint32_t ins = inside_mask(P.f, P.valid, J.isovalue);
  if (ins == 0 || ins == 0xFFu) return;
  // first vertex and crossing mask of corners 0..6 (corner 7 starts no edge of the cell)
  uint32_t vb[7], em[7];
  for (int c = 0; c < 7; ++c) {
    const uint32_t q = p + uint32_t(c & 1) + nx * (uint32_t((c >> 1) & 1) + ny * uint32_t(c >> 2));
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
                           uint32_t max_blocks) {
  hipLaunchKernelGGL(iso_emit_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kIsoBlock), 0, s,
                     jobs, outs);
  return hipGetLastError();
}

}  // namespace spray_rt
