// cell_common.h -- the split of hexahedral, wedge and pyramid cells into
// tetrahedra and the per-cell checks of spray_rt_cell_isosurface /
// spray_rt_domains_cell_isosurface, shared by the host restatement
// (cell_isosurface.cpp) and the gfx950 kernels (cell_kernels.hip).
//
// Cell types and local point order are VTK's.  A tet is its four points as
// listed.  Any other cell is the cone from its apex -- the local position m of
// its smallest point index, the lowest position on ties -- over the faces that
// do not contain m, in face-table order: a triangle (q0, q1, q2) gives the tet
// (P[m], P[q0], P[q1], P[q2]); a quad, rotated to start at the position j of
// its smallest point index (lowest j on ties), r_d = q[(j + d) mod 4], gives
// (P[m], P[r0], P[r1], P[r2]) then (P[m], P[r0], P[r2], P[r3]).  Every quad of
// the mesh is therefore cut through its smallest point index from both sides.
// The surface is tet_common.h's rule on that tet list.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tet_common.h"

namespace spray_rt {
namespace cell {

constexpr uint32_t kTet = 10, kHex = 12, kWedge = 13, kPyramid = 14;

// status bits of one mesh of a call, above tet_common.h's
constexpr uint32_t kBadType = 32;     // an unknown cell type
constexpr uint32_t kBadOffsets = 64;  // offsets[i + 1] - offsets[i] is not the type's point count
constexpr uint32_t kBadConn = 128;    // offsets[i + 1] > nconn

// The extraction numbers per block of kCellBlock consecutive cells; a cell's
// word holds its exclusive tet count within the block and its own tet count:
// loc | ntets << 12 (255 * 6 < 2^12).
constexpr int kCellBlock = 256;
SPRAY_HD uint32_t cell_word(uint32_t loc, uint32_t ntets) { return loc | (ntets << 12); }
SPRAY_HD uint32_t word_loc(uint32_t w) { return w & 4095u; }
SPRAY_HD uint32_t word_ntets(uint32_t w) { return w >> 12; }

// Points, tets and faces of a type; 0 points: unknown.
SPRAY_HD int cell_points(uint32_t type) {
  return type == kHex ? 8 : type == kWedge ? 6 : type == kPyramid ? 5 : type == kTet ? 4 : 0;
}
SPRAY_HD int cell_tets(uint32_t type) {
  return type == kHex ? 6 : type == kWedge ? 3 : type == kPyramid ? 2 : type == kTet ? 1 : 0;
}
SPRAY_HD int cell_faces(uint32_t type) { return type == kHex ? 6 : 5; }

// Face f of a hex, wedge or pyramid: local position q_d in nibble d, quads in
// cyclic order, nibble 3 of a triangle 0xF.
//   hex      (0,1,2,3) (4,5,6,7) (0,1,5,4) (1,2,6,5) (2,3,7,6) (3,0,4,7)
//   wedge    (0,1,2) (3,4,5) (0,1,4,3) (1,2,5,4) (2,0,3,5)
//   pyramid  (0,1,2,3) (0,1,4) (1,2,4) (2,3,4) (3,0,4)
SPRAY_HD uint32_t cell_face(uint32_t type, int f) {
  const uint64_t lo = type == kHex     ? 0x5621451076543210ull
                      : type == kWedge ? 0x45213410F543F210ull
                                       : 0xF432F421F4103210ull;
  const uint32_t hi = type == kHex ? 0x74036732u : type == kWedge ? 0x5302u : 0xF403u;
  return f < 4 ? uint32_t(lo >> (16 * f)) & 0xFFFFu : (hi >> (16 * (f - 4))) & 0xFFFFu;
}
SPRAY_HD int face_q(uint32_t face, int d) { return int((face >> (4 * d)) & 15u); }

// The tets of one cell of a known type, P its cell_points(type) point indices:
// 4 * cell_tets(type) indices to dst, in the rule's order.
SPRAY_HD void split(uint32_t type, const uint32_t* P, uint32_t* dst) {
  if (type == kTet) {
    for (int v = 0; v < 4; ++v) dst[v] = P[v];
    return;
  }
  const int np = cell_points(type);
  int m = 0;
  uint32_t pm = P[0];
  for (int v = 1; v < 8; ++v)
    if (v < np && P[v] < pm) {
      pm = P[v];
      m = v;
    }
  const int nf = cell_faces(type);
  for (int f = 0; f < 6; ++f) {
    if (f >= nf) break;
    const uint32_t q = cell_face(type, f);
    const bool tri = face_q(q, 3) == 15;
    bool has = false;
    for (int d = 0; d < (tri ? 3 : 4); ++d) has = has || face_q(q, d) == m;
    if (has) continue;
    if (tri) {
      dst[0] = pm;
      for (int d = 0; d < 3; ++d) dst[1 + d] = P[face_q(q, d)];
      dst += 4;
      continue;
    }
    int j = 0;
    uint32_t best = P[face_q(q, 0)];
    for (int d = 1; d < 4; ++d) {
      const uint32_t p = P[face_q(q, d)];
      if (p < best) {
        best = p;
        j = d;
      }
    }
    const uint32_t r1 = P[face_q(q, (j + 1) & 3)], r2 = P[face_q(q, (j + 2) & 3)],
                   r3 = P[face_q(q, (j + 3) & 3)];
    dst[0] = pm, dst[1] = best, dst[2] = r1, dst[3] = r2;
    dst[4] = pm, dst[5] = best, dst[6] = r2, dst[7] = r3;
    dst += 8;
  }
}

// What is wrong with the listing of one cell (status bits; 0: nothing): its
// type, its offsets against the type and nconn, its indices against npoints.
// *type_out / *first = the type and offsets[cell] of a sound cell.
SPRAY_HD uint32_t check_cell(const uint8_t* types, const uint32_t* offsets, const uint32_t* conn,
                             uint64_t npoints, uint64_t nconn, size_t cell, uint32_t* type_out,
                             uint32_t* first) {
  const uint32_t type = types[cell];
  const int np = cell_points(type);
  if (!np) return kBadType;
  const uint32_t o0 = offsets[cell], o1 = offsets[cell + 1];
  if (o1 < o0 || o1 - o0 != uint32_t(np)) return kBadOffsets;
  if (uint64_t(o1) > nconn) return kBadConn;
  uint32_t status = 0;
  for (int v = 0; v < 8; ++v)
    if (v < np && uint64_t(conn[size_t(o0) + size_t(v)]) >= npoints) status |= tet::kBadIndex;
  *type_out = type;
  *first = o0;
  return status;
}

// What one cell contributes: its tet count where its points are not all on one
// side of the isovalue (else 0), or the status bits of what is wrong with it.
// Every point of the cell is checked, whatever the isovalue.
struct Cell {
  uint32_t ntets, status;
};
SPRAY_HD Cell classify(const float* points, const uint8_t* types, const uint32_t* offsets,
                       const uint32_t* conn, const float* values, const float* cfield,
                       const float* normals, uint64_t npoints, uint64_t nconn, size_t cell,
                       float isovalue) {
  Cell C{0u, 0u};
  uint32_t type = 0, o0 = 0;
  C.status = check_cell(types, offsets, conn, npoints, nconn, cell, &type, &o0);
  if (C.status) return C;
  const int np = cell_points(type);
  uint32_t signs = 0;
  for (int v = 0; v < 8; ++v) {
    if (v >= np) break;
    const size_t p = conn[size_t(o0) + size_t(v)];
    const float f = values[p];
    if (!refit::finite_f(f)) C.status |= tet::kBadSample;
    for (int ax = 0; ax < 3; ++ax) {
      if (!refit::finite_f(points[3 * p + size_t(ax)])) C.status |= tet::kBadPoint;
      if (normals && !refit::finite_f(normals[3 * p + size_t(ax)])) C.status |= tet::kBadNormal;
    }
    if (cfield && !refit::finite_f(cfield[p])) C.status |= tet::kBadColor;
    if (iso::inside(f, isovalue)) signs |= 1u << v;
  }
  if (C.status) return C;
  if (signs != 0 && signs != (1u << np) - 1u) C.ntets = uint32_t(cell_tets(type));
  return C;
}

}  // namespace cell
}  // namespace spray_rt
