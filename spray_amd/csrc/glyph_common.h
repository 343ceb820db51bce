// glyph_common.h -- the rule of the glyph filter (spray_rt_glyphs,
// spray_rt_domains_glyphs), stated once and shared by the host restatement
// (glyphs.cpp) and the gfx950 kernels (glyph_kernels.hip): which points of a
// set are kept and at what factor, the sphere's and the arrow's vertices and
// faces (include/spray_rt.h).  dot3, usable, cross3 and
// axis_normal are the streamline filter's (stream_common.h).  Both translation
// units are compiled with -ffp-contract=off; division and square root are
// correctly rounded on either side.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "refit_common.h"
#include "stream_common.h"

namespace spray_rt {
namespace glyph {

// status bits of one set of a call (the check pass), in the order they are reported
constexpr uint32_t kBadPoint = 1;    // a non-finite point coordinate
constexpr uint32_t kBadVector = 2;   // a non-finite vector component (arrows)
constexpr uint32_t kBadScale = 4;    // a non-finite scale
constexpr uint32_t kNegScale = 8;    // a negative scale
constexpr uint32_t kBadSelect = 16;  // a non-finite select value
constexpr uint32_t kBadColor = 32;   // a non-finite sample of the colour field

constexpr int kBlock = 256;  // lanes (points) per block of the count and place passes
constexpr int kMaxLevel = 3;
constexpr int kMaxSides = strm::kMaxSides;
constexpr uint32_t kKept = 0x80000000u;  // a lane's word: kept | its exclusive rank in the block

SPRAY_HD uint32_t sphere_verts(int level) { return 10u * (1u << (2 * level)) + 2u; }
SPRAY_HD uint32_t sphere_faces(int level) { return 20u * (1u << (2 * level)); }
SPRAY_HD uint32_t arrow_verts(uint32_t ns) { return 4u * ns + 1u; }
SPRAY_HD uint32_t arrow_faces(uint32_t ns) { return 6u * ns; }

// How a set keeps its points (the arrays may be null as in spray_rt_pointset).
struct Keep {
  const float* vectors;  // read for arrows only
  const float* scales;
  const float* select;
  float select_lo, select_hi;
  uint32_t stride;
  float size, msq;
  bool arrow, scale_by_vector;
};

// Whether point i is kept; *s = its factor, *d = the square of its speed (arrows).
SPRAY_HD bool keep(const Keep& K, uint32_t i, float* s, float* d) {
  *s = 0.0f;
  *d = 0.0f;
  if (i % K.stride != 0) return false;
  if (K.select) {
    const float v = K.select[i];
    if (!(K.select_lo <= v && v <= K.select_hi)) return false;
  }
  float f = K.scales ? K.size * K.scales[i] : K.size;
  bool fast = true;
  if (K.arrow) {
    const float v[3] = {K.vectors[3 * size_t(i)], K.vectors[3 * size_t(i) + 1],
                        K.vectors[3 * size_t(i) + 2]};
    fast = strm::usable(v, K.msq, d);
    if (K.scale_by_vector) f = f * sqrtf(*d);
  }
  *s = f;
  return 0.0f < f && f < strm::pos_inf() && fast;
}

// ---- sphere: vertex k of the table u, V and F from the table ----
SPRAY_HD void sphere_vertex(const float p[3], float s, const float u[3], float pos[3],
                            float nrm[3]) {
  for (int a = 0; a < 3; ++a) {
    pos[a] = p[a] + s * u[a];
    nrm[a] = u[a];
  }
}

// ---- arrow of length L from p along T, frame N, B = T x N, ns sides ----
// Vertices: ring j * ns + k for j = 0 (at p, shaft radius), 1 (shaft end, shaft
// radius), 2 (shaft end, head radius), 3 (the tip, ns times); then the tail
// centre 4 * ns.  (c, s) is row k of the ring table; cn, ct the cone normal's
// constants.
SPRAY_HD void arrow_vertex(const float p[3], const float T[3], const float N[3],
                           const float B[3], float L, uint32_t ns, uint32_t r, float c, float s,
                           float cn, float ct, float pos[3], float nrm[3]) {
  const uint32_t j = r / ns;  // 4: the tail centre
  const float rs = 0.03f * L, rh = 0.1f * L, hl = 0.35f * L, ls = L - hl;
  const float rad = j == 2 ? rh : rs;  // rings 0 .. 2
  for (int a = 0; a < 3; ++a) {
    const float off = c * N[a] + s * B[a];
    const float cone = cn * off + ct * T[a];
    const float end = p[a] + ls * T[a], tip = p[a] + L * T[a];
    const float ring = (j == 0 ? p[a] : end) + rad * off;
    pos[a] = j >= 4 ? p[a] : (j == 3 ? tip : ring);
    nrm[a] = j >= 4 ? -T[a] : (j >= 2 ? cone : off);
  }
}

// Face r of the arrow, as vertex numbers within the arrow: the shaft (two per
// side, the tube's (a, c, b), (b, c, d) between rings 0 and 1), the annulus
// (the same between rings 1 and 2), the cone (ring 2 k, tip k, ring 2 k + 1),
// the tail fan (centre, ring 0 k, ring 0 k + 1).
SPRAY_HD void arrow_face(uint32_t ns, uint32_t r, uint32_t f[3]) {
  if (r < 4 * ns) {
    const uint32_t j = r >= 2 * ns ? 1u : 0u, q = (r - 2 * ns * j) >> 1;
    const uint32_t k1 = q + 1 == ns ? 0 : q + 1;
    const uint32_t a = j * ns + q, b = j * ns + k1, c = a + ns, d = b + ns;
    f[0] = (r & 1u) ? b : a;
    f[1] = c;
    f[2] = (r & 1u) ? d : b;
    return;
  }
  const uint32_t e = r - 4 * ns, tail = e >= ns ? 1u : 0u, k = e - tail * ns;
  const uint32_t k1 = k + 1 == ns ? 0 : k + 1;
  f[0] = tail ? 4 * ns : 2 * ns + k;
  f[1] = tail ? k : 3 * ns + k;
  f[2] = tail ? k1 : 2 * ns + k1;
}

}  // namespace glyph
}  // namespace spray_rt
