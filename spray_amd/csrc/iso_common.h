// iso_common.h -- the arithmetic and the case logic of the isosurface
// extraction (spray_rt_isosurface, spray_rt_domains_isosurface), shared by the
// host restatement (isosurface.cpp) and the gfx950 kernels (iso_kernels.hip).
//
// Marching tetrahedra over the Kuhn split of each cell: six tetrahedra, one
// per permutation of the axes in lexicographic order, each walking from the
// cell's corner (0,0,0) to (1,1,1) and adding the axes in the permutation's
// order.  Every mesh vertex lies on a lattice edge that starts at its
// componentwise-smaller endpoint and has one of 7 types (+x +y +z +xy +xz +yz
// +xyz); vertices are ordered by (point, type), faces by (cell, tetrahedron,
// triangle).  The mesh is a function of the grid alone.  A sample equal to
// the isovalue puts vertices on lattice points and may give zero-area
// triangles: they are kept (tri_record accepts them, and dropping them would
// break the numbering).  Both translation units are compiled with
// -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "refit_common.h"

namespace spray_rt {
namespace iso {

constexpr uint32_t kBadSample = 1;  // status bit of a grid: a non-finite sample
constexpr uint32_t kBadColor = 2;   // ... a non-finite sample of its colour field

// The extraction numbers per block of kIsoBlock consecutive points; a point's
// code word holds its crossing-edge mask and its exclusive vertex / face
// counts within the block: mask | vloc << 7 | floc << 18 (255 * 7 < 2^11,
// 255 * 12 < 2^12).
constexpr int kIsoBlock = 256;
SPRAY_HD uint32_t code_word(uint32_t emask, uint32_t vloc, uint32_t floc) {
  return emask | (vloc << 7) | (floc << 18);
}
SPRAY_HD uint32_t code_emask(uint32_t c) { return c & 127u; }
SPRAY_HD uint32_t code_vloc(uint32_t c) { return (c >> 7) & 2047u; }
SPRAY_HD uint32_t code_floc(uint32_t c) { return c >> 18; }

SPRAY_HD int popc(uint32_t x) { return __builtin_popcount(x); }

SPRAY_HD bool inside(float f, float isovalue) { return f >= isovalue; }

// Corner c of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z.  The partner of a
// point along edge type t is corner type_corner(t) of the cell whose minimum
// corner the point is: 1 2 4 3 5 6 7.
SPRAY_HD int type_corner(int type) { return int((0x7653421u >> (4 * type)) & 7u); }
// and back: the type of the edge between corners cu < cv, d = cu ^ cv
SPRAY_HD int diff_type(int d) { return int((0x65423100u >> (4 * d)) & 7u); }

// Corners of the cell at (i, j, k) that are grid points (bit c).
SPRAY_HD uint32_t valid_corners(int i, int j, int k, int nx, int ny, int nz) {
  uint32_t v = 0xFFu;
  if (i + 1 >= nx) v &= 0x55u;
  if (j + 1 >= ny) v &= 0x33u;
  if (k + 1 >= nz) v &= 0x0Fu;
  return v;
}

// Inside bits of the valid corners; f[c] is read for those only.
SPRAY_HD uint32_t inside_mask(const float f[8], uint32_t valid, float isovalue) {
  uint32_t m = 0;
  for (int c = 0; c < 8; ++c)
    if (((valid >> c) & 1u) && inside(f[c], isovalue)) m |= 1u << c;
  return m;
}

// Edge types of the point that cross: exactly one endpoint is inside.
SPRAY_HD uint32_t edge_mask(uint32_t ins, uint32_t valid) {
  uint32_t m = 0;
  for (int t = 0; t < 7; ++t) {
    const int c = type_corner(t);
    if (((valid >> c) & 1u) && (((ins >> c) ^ ins) & 1u)) m |= 1u << t;
  }
  return m;
}

// Tetrahedron tet (0..5: xyz xzy yxz yzx zxy zyx) of the Kuhn split: the
// cell corners of its walk, and whether the permutation is odd.
SPRAY_HD void tet_corners(int tet, int T[4]) {
  const int a = tet >> 1, b = (0x489 >> (2 * tet)) & 3;
  T[0] = 0;
  T[1] = 1 << a;
  T[2] = T[1] | (1 << b);
  T[3] = 7;
}
SPRAY_HD int tet_odd(int tet) { return (0x26 >> tet) & 1; }

// Inside bits of the walk's four vertices.
SPRAY_HD uint32_t tet_signs(const int T[4], uint32_t ins) {
  return ((ins >> T[0]) & 1u) | (((ins >> T[1]) & 1u) << 1) | (((ins >> T[2]) & 1u) << 2) |
         (((ins >> T[3]) & 1u) << 3);
}

SPRAY_HD int tet_tri_count(uint32_t s) {
  const int n = popc(s);
  return n == 0 || n == 4 ? 0 : (n == 2 ? 2 : 1);
}

// Triangles of a full cell with these inside bits: at most 12.
SPRAY_HD uint32_t cell_tri_count(uint32_t ins) {
  if (ins == 0 || ins == 0xFFu) return 0;
  uint32_t n = 0;
  for (int tet = 0; tet < 6; ++tet) {
    int T[4];
    tet_corners(tet, T);
    n += uint32_t(tet_tri_count(tet_signs(T, ins)));
  }
  return n;
}

// The triangles of one tetrahedron: signs s of its walk, odd its permutation's
// parity.  e[n][v] is vertex v of triangle n as a walk edge (u << 2 | w, u < w).
// Ng = (p0 - p1) x (p2 - p0) leaves the region f >= isovalue: the walk of an
// even permutation is positively oriented, so the orientation of a triangle
// follows from the parity of its arrangement (a, b, c, d) of the walk.
SPRAY_HD int tet_triangles(uint32_t s, int odd, uint8_t e[2][3]) {
  const int n = popc(s);
  if (n == 0 || n == 4) return 0;
  auto edge = [](int u, int w) { return uint8_t(u < w ? (u << 2 | w) : (w << 2 | u)); };
  if (n != 2) {
    // one vertex a apart from b < c < d: (a, b, c, d) is odd iff a is
    const uint32_t lone = n == 1 ? s : (~s & 15u);
    const int a = lone == 1 ? 0 : lone == 2 ? 1 : lone == 4 ? 2 : 3;
    int o[3], k = 0;
    for (int v = 0; v < 4; ++v)
      if (v != a) o[k++] = v;
    const bool positive = ((a & 1) ^ odd) == 0;
    const bool keep = positive == (n == 3);
    e[0][0] = edge(a, o[0]);
    e[0][1] = edge(a, keep ? o[1] : o[2]);
    e[0][2] = edge(a, keep ? o[2] : o[1]);
    return 1;
  }
  // two inside a < b, two outside c < d: the quad ac ad bd bc
  int in2[2], out2[2], ni = 0, no = 0;
  for (int v = 0; v < 4; ++v) {
    if ((s >> v) & 1u)
      in2[ni++] = v;
    else
      out2[no++] = v;
  }
  const int a = in2[0], b = in2[1], c = out2[0], d = out2[1];
  const int inv = (a > c) + (a > d) + (b > c) + (b > d);
  const bool positive = ((inv & 1) ^ odd) == 0;
  const uint8_t q0 = edge(a, c), q1 = edge(a, d), q2 = edge(b, d), q3 = edge(b, c);
  e[0][0] = q0;
  e[0][1] = positive ? q2 : q1;
  e[0][2] = positive ? q1 : q2;
  e[1][0] = q0;
  e[1][1] = positive ? q3 : q2;
  e[1][2] = positive ? q2 : q3;
  return 2;
}

// Point index `idx` of an axis.
SPRAY_HD float coord(float origin, int idx, float spacing) { return origin + float(idx) * spacing; }

// Where edge (a, b), a the smaller endpoint, meets the isovalue.
SPRAY_HD float edge_t(float fa, float fb, float isovalue) { return (isovalue - fa) / (fb - fa); }
SPRAY_HD float lerp(float a, float b, float t) { return a + t * (b - a); }

// The vertex on the edge of type `type` at point (i, j, k).
SPRAY_HD void edge_vertex(const float origin[3], const float spacing[3], int i, int j, int k,
                          int type, float t, float p[3]) {
  const int c = type_corner(type);
  const int idx[3] = {i, j, k};
  for (int ax = 0; ax < 3; ++ax) {
    const float pa = coord(origin[ax], idx[ax], spacing[ax]);
    const float pb = coord(origin[ax], idx[ax] + ((c >> ax) & 1), spacing[ax]);
    p[ax] = lerp(pa, pb, t);
  }
}

// Negated gradient at a grid point: central differences (times 0.5),
// one-sided on the grid boundary, divided by the spacing.
SPRAY_HD void neg_gradient(const float* values, int nx, int ny, int nz, int i, int j, int k,
                           const float spacing[3], float g[3]) {
  const size_t sx = 1, sy = size_t(nx), sz = size_t(nx) * size_t(ny);
  const size_t p = size_t(i) + sy * size_t(j) + sz * size_t(k);
  const int idx[3] = {i, j, k}, dim[3] = {nx, ny, nz};
  const size_t stride[3] = {sx, sy, sz};
  for (int ax = 0; ax < 3; ++ax) {
    const bool lo = idx[ax] > 0, hi = idx[ax] + 1 < dim[ax];
    const float fm = values[lo ? p - stride[ax] : p], fp = values[hi ? p + stride[ax] : p];
    float d = fp - fm;
    if (lo && hi) d = d * 0.5f;
    g[ax] = -(d / spacing[ax]);
  }
}

}  // namespace iso
}  // namespace spray_rt
