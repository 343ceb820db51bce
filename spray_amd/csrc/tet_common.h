// tet_common.h -- the arithmetic and the case logic of the isosurface
// extraction from unstructured tetrahedral meshes (spray_rt_tet_isosurface,
// spray_rt_domains_tet_isosurface), shared by the host restatement
// (tet_isosurface.cpp) and the gfx950 kernels (tet_kernels.hip).
//
// Marching tetrahedra over explicit tets: iso::tet_triangles with the tet's
// four listed points as the walk 0..3 and the parity from the geometry
// (orient_odd).  A mesh vertex belongs to a distinct unordered point pair
// {a, b}, a < b by point index, whose samples differ in sign; everything about
// it (t, position, normal, colour) is a function of the pair alone.  Vertices
// are ordered by the pair (a, b), faces by (tet, triangle).  Both translation
// units are compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "color_common.h"
#include "iso_common.h"

namespace spray_rt {
namespace tet {

// status bits of one mesh of a call
constexpr uint32_t kBadIndex = 1;   // a point index >= npoints
constexpr uint32_t kBadPoint = 2;   // a non-finite coordinate of a referenced point
constexpr uint32_t kBadSample = 4;  // ... a non-finite sample
constexpr uint32_t kBadColor = 8;   // ... a non-finite sample of the colour field
constexpr uint32_t kBadNormal = 16; // ... a non-finite normal (where normals are wanted)

// The extraction numbers per block of kTetBlock consecutive tets; a tet's word
// holds its inside bits, its parity and its exclusive crossing-edge / face
// counts within the block: signs | odd << 4 | eloc << 5 | floc << 16
// (255 * 4 < 2^11, 255 * 2 < 2^9).
constexpr int kTetBlock = 256;
SPRAY_HD uint32_t tet_word(uint32_t signs, uint32_t odd, uint32_t eloc, uint32_t floc) {
  return signs | (odd << 4) | (eloc << 5) | (floc << 16);
}
SPRAY_HD uint32_t word_signs(uint32_t w) { return w & 15u; }
SPRAY_HD int word_odd(uint32_t w) { return int((w >> 4) & 1u); }
SPRAY_HD uint32_t word_eloc(uint32_t w) { return (w >> 5) & 2047u; }
SPRAY_HD uint32_t word_floc(uint32_t w) { return w >> 16; }

// Walk edge k = 0..5: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).
SPRAY_HD int edge_u(int k) { return int((0x211000u >> (4 * k)) & 3u); }
SPRAY_HD int edge_w(int k) { return int((0x332321u >> (4 * k)) & 3u); }
// and back, from iso::tet_triangles' edge u << 2 | w, u < w
SPRAY_HD int edge_index(int e) { return e < 4 ? e - 1 : (e < 8 ? e - 3 : 5); }

// Walk edges whose endpoints differ in sign (bit k): none, 3 or 4 of them.  A
// tet that lists a point twice has equal signs there and never crosses on it.
SPRAY_HD uint32_t cross_mask(uint32_t s) {
  uint32_t m = 0;
  for (int k = 0; k < 6; ++k)
    if (((s >> edge_u(k)) ^ (s >> edge_w(k))) & 1u) m |= 1u << k;
  return m;
}

// Whether the walk p0 p1 p2 p3 is negatively oriented: det = dot(cross(p1 -
// p0, p2 - p0), p3 - p0) term by term in float, left to right; det == 0 and a
// NaN det count as even.  A sliver whose float det has the wrong sign flips
// its one or two triangles.
SPRAY_HD int orient_odd(const float* p0, const float* p1, const float* p2, const float* p3) {
  const float a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
  const float b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
  const float c0 = p3[0] - p0[0], c1 = p3[1] - p0[1], c2 = p3[2] - p0[2];
  const float x = a1 * b2 - a2 * b1;
  const float y = a2 * b0 - a0 * b2;
  const float z = a0 * b1 - a1 * b0;
  const float det = x * c0 + y * c1 + z * c2;
  return det < 0.0f ? 1 : 0;
}

// The sort key of the pair (a, b), a < b: a above b's `shift` bits, shift the
// bit width of the mesh's largest point index.  Ascending keys are ascending
// (a << 32) | b.
SPRAY_HD int index_bits(uint64_t npoints) {
  int w = 1;
  while (w < 32 && (uint64_t(1) << w) < npoints) ++w;
  return w;
}
SPRAY_HD uint64_t pair_key(uint32_t a, uint32_t b, int shift) {
  return (uint64_t(a) << shift) | uint64_t(b);
}
SPRAY_HD uint32_t key_a(uint64_t key, int shift) { return uint32_t(key >> shift); }
SPRAY_HD uint32_t key_b(uint64_t key, int shift) {
  return uint32_t(key & ((uint64_t(1) << shift) - 1u));
}

// What one tet contributes: its inside bits and parity, or the status bits of
// what is wrong with it (then signs and odd are 0: it contributes nothing).
struct Corner {
  uint32_t signs, odd, status;
};
SPRAY_HD Corner classify(const float* points, const uint32_t* tets, const float* values,
                         const float* cfield, const float* normals, uint64_t npoints, size_t t,
                         float isovalue) {
  Corner C{0u, 0u, 0u};
  uint32_t idx[4];
  for (int v = 0; v < 4; ++v) {
    idx[v] = tets[4 * t + size_t(v)];
    if (uint64_t(idx[v]) >= npoints) C.status |= kBadIndex;
  }
  if (C.status) return C;
  for (int v = 0; v < 4; ++v) {
    const size_t p = idx[v];
    const float f = values[p];
    if (!refit::finite_f(f)) C.status |= kBadSample;
    for (int ax = 0; ax < 3; ++ax) {
      if (!refit::finite_f(points[3 * p + size_t(ax)])) C.status |= kBadPoint;
      if (normals && !refit::finite_f(normals[3 * p + size_t(ax)])) C.status |= kBadNormal;
    }
    if (cfield && !refit::finite_f(cfield[p])) C.status |= kBadColor;
    if (iso::inside(f, isovalue)) C.signs |= 1u << v;
  }
  if (C.status) {
    C.signs = 0;
    return C;
  }
  C.odd = uint32_t(orient_odd(points + 3 * size_t(idx[0]), points + 3 * size_t(idx[1]),
                              points + 3 * size_t(idx[2]), points + 3 * size_t(idx[3])));
  return C;
}

// The vertex of the pair (a, b), a < b: t, then position, normal and colour
// scalar with it; null outputs are skipped.
SPRAY_HD float pair_t(const float* values, uint32_t a, uint32_t b, float isovalue) {
  return iso::edge_t(values[a], values[b], isovalue);
}
SPRAY_HD void pair_lerp3(const float* arr, uint32_t a, uint32_t b, float t, float out[3]) {
  for (int ax = 0; ax < 3; ++ax)
    out[ax] = iso::lerp(arr[3 * size_t(a) + size_t(ax)], arr[3 * size_t(b) + size_t(ax)], t);
}

}  // namespace tet
}  // namespace spray_rt
