// clip_common.h -- the rule of the clip of meshes of hexahedra, wedges,
// pyramids and tets by a level of their scalar field (spray_rt_cell_clip,
// spray_rt_domains_cell_clip), shared by the host restatement (cell_clip.cpp)
// and the gfx950 kernels (clip_kernels.hip).
//
// A point is kept when iso::inside(values[p], isovalue), with invert when it
// is not.  The solid is the kept side of the linear interpolant over
// cell_common.h's tet split; its surface is the cap, tet_common.h's
// isosurface of that split, and the skin: the triangles of surf_common.h's
// boundary over the cells with a kept point, each cut by the kept bits of its
// three corners into 0, 1 or 2 pieces whose corners are kept points or cap
// vertices of a pair of corners.  Vertices are the cap's, then the kept points
// the skin uses ascending by index; faces are the cap's (corners 1 and 2
// swapped with invert), then the skin's by cell, face, triangle, piece.  Both
// translation units are compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cell_common.h"
#include "surf_common.h"
#include "tet_common.h"

namespace spray_rt {
namespace clip {

// status bit of one mesh of a call, above surf_common.h's: a cut edge of the
// skin whose pair is not among the cap's (never on input that passed the checks).
// A guard, not a reachable error: a cut edge of a boundary triangle is an edge
// of the cell's own tet split, which cuts a quad by the same smallest-index
// rule.  tests/test_mesh_cases.py::test_collapsed_family_clips_and_surfaces
// clips every single-position collapse of each cell type on the host (which
// raises on any status) and tests/test_gpu_mesh_cases.py::test_many_segments
// the same family on the device; none sets it.
constexpr uint32_t kMiss = 512;

SPRAY_HD bool kept(float f, float isovalue, uint32_t invert) {
  return iso::inside(f, isovalue) != (invert != 0u);
}

// A cell's word after the skin count: the pieces in front of it within its
// block and the mask of its surviving faces (255 * 24 < 2^16).
SPRAY_HD uint32_t skin_word(uint32_t loc, uint32_t mask) { return loc | (mask << 16); }
SPRAY_HD uint32_t skin_loc(uint32_t w) { return w & 0xFFFFu; }
SPRAY_HD uint32_t skin_mask(uint32_t w) { return w >> 16; }

// What one cell contributes: its face count where it takes part, that is where
// one of its listed points is kept (else 0), or the status bits of what is
// wrong with it.  Every point of the cell is checked, kept or not.
SPRAY_HD surf::Cell classify(const float* points, const uint8_t* types, const uint32_t* offsets,
                             const uint32_t* conn, const float* values, const float* cfield,
                             const float* normals, uint64_t npoints, uint64_t nconn, size_t cell,
                             float isovalue, uint32_t invert) {
  surf::Cell C{0u, 0u};
  uint32_t type = 0, o0 = 0;
  C.status = cell::check_cell(types, offsets, conn, npoints, nconn, cell, &type, &o0);
  if (C.status) return C;
  const int np = cell::cell_points(type);
  bool any = false;
  for (int v = 0; v < 8; ++v) {
    if (v >= np) break;
    const size_t p = conn[size_t(o0) + size_t(v)];
    for (int ax = 0; ax < 3; ++ax) {
      if (!refit::finite_f(points[3 * p + size_t(ax)])) C.status |= tet::kBadPoint;
      if (normals && !refit::finite_f(normals[3 * p + size_t(ax)])) C.status |= tet::kBadNormal;
    }
    if (cfield && !refit::finite_f(cfield[p])) C.status |= tet::kBadColor;
    const float f = values[p];
    if (!refit::finite_f(f)) C.status |= tet::kBadSample;
    any = any || kept(f, isovalue, invert);
  }
  if (C.status) return C;
  if (any) C.nfaces = uint32_t(surf::faces_of(type));
  return C;
}

// The pieces of a triangle whose corner i is kept where bit i of bits is set.
SPRAY_HD int piece_count(uint32_t bits) {
  const int n = iso::popc(bits & 7u);
  return n == 3 ? 1 : n;
}

// Corner v of piece `piece`: the triangle's corners *i and *j; i == j is the
// kept point itself, else the cap vertex of the pair of corners i and j.
//   3 kept        (0, 1, 2)
//   only k        (k, X(k,k+1), X(k,k+2))
//   all but k     (k+1, k+2, X(k+2,k)) then (k+1, X(k+2,k), X(k,k+1))
SPRAY_HD void piece_corner(uint32_t bits, int piece, int v, int* i, int* j) {
  bits &= 7u;
  const int n = iso::popc(bits);
  if (n == 3) {
    *i = *j = v;
    return;
  }
  if (n == 1) {
    const int k = bits == 1u ? 0 : bits == 2u ? 1 : 2;
    *i = k;
    *j = (k + v) % 3;
    return;
  }
  const int k = bits == 6u ? 0 : bits == 5u ? 1 : 2;  // the dropped corner
  const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
  if (piece == 0) {
    *i = v == 0 ? k1 : k2;
    *j = v == 0 ? k1 : v == 1 ? k2 : k;
  } else {
    *i = v == 0 ? k1 : v == 1 ? k2 : k;
    *j = v == 0 ? k1 : v == 1 ? k : k1;
  }
}

// The index of the first of the sorted keys skeys[0, n) equal to key, n where
// there is none; at most 33 probes.
SPRAY_HD uint32_t find_key(const uint64_t* skeys, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  for (int step = 0; step < 33 && lo < hi; ++step) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (skeys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && skeys[lo] == key ? lo : n;
}

// values[p] of the plane through origin with normal nrm: term by term in float.
SPRAY_HD float plane_value(const float* p, const float* origin, const float* nrm) {
  return ((p[0] - origin[0]) * nrm[0] + (p[1] - origin[1]) * nrm[1]) +
         (p[2] - origin[2]) * nrm[2];
}

}  // namespace clip
}  // namespace spray_rt
