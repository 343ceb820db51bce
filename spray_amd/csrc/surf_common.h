// surf_common.h -- the rule of the boundary-surface and threshold extraction
// from meshes of hexahedra, wedges, pyramids and tets (spray_rt_cell_surface,
// spray_rt_domains_cell_surface), shared by the host restatement
// (cell_surface.cpp) and the gfx950 kernels (surf_kernels.hip).
//
// A select keeps cells (all; those whose points all lie in [lo, hi]; those
// whose cell value does).  A kept cell has the faces of cell_common.h's tables
// in table order, a tet (0,1,2) (0,1,3) (1,2,3) (2,0,3).  With c[i] the point
// indices of a face and j the position of the smallest (lowest j on ties), the
// face's key is (corner count, c[j], min(a, b), max(a, b)), a and b the face's
// corners next to c[j] on either side.  A face whose key occurs once among the
// kept cells' faces of its mesh is on the surface.  Vertices are the points such faces use,
// ascending by point index; triangles come by cell, then face: a triangle as
// listed, a quad cut through its smallest index (cell_common.h's diagonal),
// turned outward by the sign of a float determinant against a point of the
// cell that is not on the face.  Both translation units are compiled with
// -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cell_common.h"
#include "tet_common.h"

namespace spray_rt {
namespace surf {

// SPRAY_RT_SELECT_*; cell_surface.cpp asserts that they agree
constexpr int32_t kAll = 0, kPoints = 1, kCells = 2;

// status bit of one mesh of a call, above cell_common.h's
constexpr uint32_t kBadCellValue = 256;  // a non-finite cell_values[i] (mode kCells)

// The largest mesh whose key, three indices and the quad bit, fits 64 bits.
constexpr uint64_t kMaxPoints = uint64_t(1) << 21;

// The extraction numbers per block of kSurfBlock consecutive cells or points.
// A cell's word holds an exclusive count within its block and six bits beside
// it: first the face instances in front of the cell and its own instance
// count (255 * 6 < 2^12), later the triangles in front of it and the mask of
// its surviving faces (255 * 12 < 2^12).  A point's word holds the vertices in
// front of it within its block and whether it is one itself.
constexpr int kSurfBlock = 256;
SPRAY_HD uint32_t cell_word(uint32_t loc, uint32_t bits) { return loc | (bits << 12); }
SPRAY_HD uint32_t word_loc(uint32_t w) { return w & 4095u; }
SPRAY_HD uint32_t word_bits(uint32_t w) { return w >> 12; }
SPRAY_HD uint32_t point_word(uint32_t loc, uint32_t used) { return loc | (used << 16); }
SPRAY_HD uint32_t pword_loc(uint32_t w) { return w & 0xFFFFu; }
SPRAY_HD uint32_t pword_used(uint32_t w) { return w >> 16; }

// Faces of a type and face f as cell::cell_face's nibbles.
SPRAY_HD int faces_of(uint32_t type) { return type == cell::kTet ? 4 : cell::cell_faces(type); }
SPRAY_HD uint32_t face_of(uint32_t type, int f) {
  if (type == cell::kTet) return (0xF302F321F310F210ull >> (16 * f)) & 0xFFFFu;
  return cell::cell_face(type, f);
}
SPRAY_HD int face_corners(uint32_t face) { return cell::face_q(face, 3) == 15 ? 3 : 4; }

// The lowest local position of the cell that is not on the face.
SPRAY_HD int face_ref(uint32_t face) {
  const int nc = face_corners(face);
  uint32_t on = 0;
  for (int d = 0; d < nc; ++d) on |= 1u << cell::face_q(face, d);
  int v = 0;
  while ((on >> v) & 1u) ++v;
  return v;
}

// A face of a cell, P the cell's listed point indices: the corners rotated to
// start at the smallest index (r[0]; a triangle keeps its listed order in c).
struct Face {
  uint32_t c[4];  // as listed
  uint32_t r[4];  // from the smallest on; r[3] of a triangle is unused
  int n;          // 3 or 4 corners
};
SPRAY_HD Face face_points(uint32_t face, const uint32_t* P) {
  Face F;
  F.n = face_corners(face);
  int j = 0;
  uint32_t best = 0;
  for (int d = 0; d < 4; ++d) {
    F.c[d] = d < F.n ? P[cell::face_q(face, d)] : 0u;
    if (d < F.n && (d == 0 || F.c[d] < best)) {
      best = F.c[d];
      j = d;
    }
  }
  // P[q] again from memory, not c[] by a computed index: c stays in registers
  for (int d = 0; d < 4; ++d) {
    const int at = j + d < F.n ? j + d : j + d - F.n;
    F.r[d] = d < F.n ? P[cell::face_q(face, at)] : 0u;
  }
  return F;
}

// The sort key of a face: (quad << 3w) | (m << 2w) | (lo << w) | hi, w the bit
// width of the mesh's largest point index (tet::index_bits, at most 21, so the
// key has at most 64 bits).  quad is 1 for a face of four corners: a quad and
// the triangle on its smallest corner and that corner's two neighbours have
// the same triple and must not match.
SPRAY_HD int key_bits(int w) { return 3 * w + 1; }
SPRAY_HD uint64_t face_key(const Face& F, int w) {
  const uint32_t a = F.r[1], b = F.n == 3 ? F.r[2] : F.r[3];
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return (uint64_t(F.n == 4 ? 1u : 0u) << (3 * w)) | (uint64_t(F.r[0]) << (2 * w)) |
         (uint64_t(lo) << w) | uint64_t(hi);
}

// The triangles of a face as point indices to tri[6] (a triangle face fills
// the first three and leaves the rest unspecified), turned away from pref (a
// point's three coordinates): the sign of det = dot(cross(p1 - p0, p2 - p0),
// pref - p0) on the first triangle decides for the whole face; det == 0 and
// NaN leave the listed order.  -> the triangle count.
SPRAY_HD int face_triangles(const Face& F, const float* points, const float* pref,
                            uint32_t* tri) {
  const bool quad = F.n == 4;
  const uint32_t v0 = quad ? F.r[0] : F.c[0], v1 = quad ? F.r[1] : F.c[1],
                 v2 = quad ? F.r[2] : F.c[2], v3 = F.r[3];
  const bool flip = tet::orient_odd(points + 3 * size_t(v0), points + 3 * size_t(v1),
                                    points + 3 * size_t(v2), pref) != 0;
  tri[0] = v0, tri[1] = flip ? v2 : v1, tri[2] = flip ? v1 : v2;
  tri[3] = v0, tri[4] = flip ? v3 : v2, tri[5] = flip ? v2 : v3;
  return quad ? 2 : 1;
}

// What one cell contributes: its face count where the select keeps it (else
// 0), or the status bits of what is wrong with it.  Every point of the cell is
// checked, kept or not.
struct Cell {
  uint32_t nfaces, status;
};
SPRAY_HD bool in_range(float v, float lo, float hi) { return lo <= v && v <= hi; }
SPRAY_HD Cell classify(const float* points, const uint8_t* types, const uint32_t* offsets,
                       const uint32_t* conn, const float* values, const float* cell_values,
                       const float* cfield, const float* normals, uint64_t npoints,
                       uint64_t nconn, size_t cell, int32_t mode, float lo, float hi) {
  Cell C{0u, 0u};
  uint32_t type = 0, o0 = 0;
  C.status = cell::check_cell(types, offsets, conn, npoints, nconn, cell, &type, &o0);
  if (C.status) return C;
  const int np = cell::cell_points(type);
  bool keep = true;
  for (int v = 0; v < 8; ++v) {
    if (v >= np) break;
    const size_t p = conn[size_t(o0) + size_t(v)];
    for (int ax = 0; ax < 3; ++ax) {
      if (!refit::finite_f(points[3 * p + size_t(ax)])) C.status |= tet::kBadPoint;
      if (normals && !refit::finite_f(normals[3 * p + size_t(ax)])) C.status |= tet::kBadNormal;
    }
    if (cfield && !refit::finite_f(cfield[p])) C.status |= tet::kBadColor;
    if (mode == kPoints) {
      const float f = values[p];
      if (!refit::finite_f(f)) C.status |= tet::kBadSample;
      keep = keep && in_range(f, lo, hi);
    }
  }
  if (mode == kCells) {
    const float f = cell_values[cell];
    if (!refit::finite_f(f)) C.status |= kBadCellValue;
    keep = in_range(f, lo, hi);
  }
  if (C.status) return C;
  if (keep) C.nfaces = uint32_t(faces_of(type));
  return C;
}

// The colour of point p: the table entry of its colour sample, or the mesh's.
SPRAY_HD uint32_t point_color(const float* cfield, const uint32_t* ctable, float clo, float cscale,
                              int ntable, uint32_t color, size_t p) {
  return cfield ? ctable[cmap::bin(cfield[p], clo, cscale, ntable)] : color;
}

}  // namespace surf
}  // namespace spray_rt
