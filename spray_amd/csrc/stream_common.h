// stream_common.h -- the rule of the streamline filter (spray_rt_streamlines,
// spray_rt_stream_tubes, spray_rt_domains_stream_tubes), stated once and shared
// by the host restatement (streamlines.cpp) and the gfx950 kernels
// (stream_kernels.hip): the trilinear sample, the fixed-step RK4 step and the
// reasons a half-line ends, the tangent and the transported frame, the tube's
// vertices and faces (include/spray_rt.h).  Both
// translation units are compiled with -ffp-contract=off; division and square
// root are correctly rounded on either side.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "iso_common.h"
#include "refit_common.h"

namespace spray_rt {
namespace strm {

// status bits of one field of a call (the check pass)
constexpr uint32_t kBadSeed = 1;    // a non-finite seed coordinate
constexpr uint32_t kBadVector = 2;  // a non-finite vector sample
constexpr uint32_t kBadColor = 4;   // a non-finite sample of the colour field

constexpr int kBlock = 256;    // lanes (half-lines) per block of the integration
constexpr int kMaxSteps = 65535;
constexpr int kMaxSides = 16;
constexpr int kTaken = -1;  // advance(): the step is taken (else a SPRAY_RT_LINE_END_*)
// the end reasons of include/spray_rt.h
constexpr int kEndGrid = 0, kEndSteps = 1, kEndSpeed = 2, kEndSeed = 3;

// A lane's word: the points it writes (at most kMaxSteps + 1) | end << 24.
SPRAY_HD uint32_t lane_word(uint32_t cnt, int end) { return cnt | (uint32_t(end) << 24); }
SPRAY_HD uint32_t word_count(uint32_t w) { return w & 0xFFFFFFu; }
SPRAY_HD uint32_t word_end(uint32_t w) { return w >> 24; }
// What the block scan sums per lane: its points (a block holds at most 2^24),
// and for the lane that closes a line the line's tube points (its points where
// it has two or more) and whether it has a tube: cnt | tube_pts << 25 | tube << 50.
constexpr uint64_t kMask25 = (uint64_t(1) << 25) - 1;
SPRAY_HD uint64_t scan_word(uint32_t cnt, uint32_t line_pts) {
  const uint64_t tube = line_pts >= 2 ? 1 : 0;
  return uint64_t(cnt) | ((tube ? uint64_t(line_pts) : 0) << 25) | (tube << 50);
}
SPRAY_HD uint32_t scan_points(uint64_t v) { return uint32_t(v & kMask25); }
SPRAY_HD uint32_t scan_tube_points(uint64_t v) { return uint32_t((v >> 25) & kMask25); }
SPRAY_HD uint32_t scan_tube_lines(uint64_t v) { return uint32_t(v >> 50); }

struct Grid {
  const float* vectors;  // [nz][ny][nx][3]
  int32_t n[3];
  float origin[3], spacing[3];
};

// The cell a point is sampled in: its minimum corner's point index and the
// fractions.  The index is that of a cell of the grid whatever the point.
struct Cell {
  size_t base;
  float f[3];
};

SPRAY_HD uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }
SPRAY_HD float pos_inf() { return __builtin_huge_valf(); }

// Whether p is inside the grid; *c = its cell (cell 0 on an axis p is outside on).
SPRAY_HD bool locate(const Grid& G, const float p[3], Cell* c) {
  bool in = true;
  size_t idx[3];
  for (int a = 0; a < 3; ++a) {
    const float g = (p[a] - G.origin[a]) / G.spacing[a];
    const bool ina = g >= 0.0f && g <= float(G.n[a] - 1);
    int i = ina ? int(floorf(g)) : 0;
    if (i > G.n[a] - 2) i = G.n[a] - 2;
    c->f[a] = g - float(i);
    idx[a] = size_t(i);
    in = in && ina;
  }
  c->base = idx[0] + size_t(G.n[0]) * (idx[1] + size_t(G.n[1]) * idx[2]);
  return in;
}

// Corner k of a cell (bit 0 +x, bit 1 +y, bit 2 +z) as a point offset.
SPRAY_HD size_t corner_offset(const Grid& G, int k) {
  return size_t(k & 1) + size_t(G.n[0]) * (size_t((k >> 1) & 1) + size_t(G.n[1]) * size_t(k >> 2));
}

// The four x-lerps, the two y-lerps, the z-lerp.
SPRAY_HD float trilerp(const float c[8], const float f[3]) {
  const float x00 = iso::lerp(c[0], c[1], f[0]), x10 = iso::lerp(c[2], c[3], f[0]);
  const float x01 = iso::lerp(c[4], c[5], f[0]), x11 = iso::lerp(c[6], c[7], f[0]);
  const float y0 = iso::lerp(x00, x10, f[1]), y1 = iso::lerp(x01, x11, f[1]);
  return iso::lerp(y0, y1, f[2]);
}

SPRAY_HD void sample_vector(const Grid& G, const Cell& c, float v[3]) {
  float cx[8], cy[8], cz[8];
  for (int k = 0; k < 8; ++k) {
    const float* s = G.vectors + 3 * (c.base + corner_offset(G, k));
    cx[k] = s[0];
    cy[k] = s[1];
    cz[k] = s[2];
  }
  v[0] = trilerp(cx, c.f);
  v[1] = trilerp(cy, c.f);
  v[2] = trilerp(cz, c.f);
}

SPRAY_HD float sample_scalar(const Grid& G, const float* field, const Cell& c) {
  float s[8];
  for (int k = 0; k < 8; ++k) s[k] = field[c.base + corner_offset(G, k)];
  return trilerp(s, c.f);
}

SPRAY_HD float dot3(const float a[3], const float b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// Whether the speed of k1 is usable; *d = its square.
SPRAY_HD bool usable(const float k1[3], float msq, float* d) {
  *d = dot3(k1, k1);
  return msq <= *d && *d < pos_inf();
}

// The RK4 arithmetic from p with k1 = v(p): kTaken with pn and its cell, or
// kEndGrid where a stage point or pn is outside the grid.
SPRAY_HD int rk4(const Grid& G, const float p[3], const float k1[3], float h, float pn[3],
                 Cell* cn) {
  const float hh = 0.5f * h, h6 = h / 6.0f;
  float q[3], k2[3], k3[3], k4[3];
  Cell c;
  for (int a = 0; a < 3; ++a) q[a] = p[a] + hh * k1[a];
  if (!locate(G, q, &c)) return kEndGrid;
  sample_vector(G, c, k2);
  for (int a = 0; a < 3; ++a) q[a] = p[a] + hh * k2[a];
  if (!locate(G, q, &c)) return kEndGrid;
  sample_vector(G, c, k3);
  for (int a = 0; a < 3; ++a) q[a] = p[a] + h * k3[a];
  if (!locate(G, q, &c)) return kEndGrid;
  sample_vector(G, c, k4);
  for (int a = 0; a < 3; ++a)
    pn[a] = p[a] + h6 * (((k1[a] + 2.0f * k2[a]) + 2.0f * k3[a]) + k4[a]);
  return locate(G, pn, cn) ? kTaken : kEndGrid;
}

// One step of a half-line that has taken `steps`: kTaken, or the first reason
// that applies of SPEED, GRID, SPEED (the step moved nothing), STEPS.
SPRAY_HD int advance(const Grid& G, const float p[3], const float k1[3], float h, float msq,
                     int steps, int max_steps, float pn[3], Cell* cn) {
  float d;
  if (!usable(k1, msq, &d)) return kEndSpeed;
  const int r = rk4(G, p, k1, h, pn, cn);
  if (r != kTaken) return r;
  if (bits(pn[0]) == bits(p[0]) && bits(pn[1]) == bits(p[1]) && bits(pn[2]) == bits(p[2]))
    return kEndSpeed;
  if (steps >= max_steps) return kEndSteps;
  return kTaken;
}

// The steps a half-line from an inside seed takes (its cell c0); *end = why it ends.
SPRAY_HD int trace_count(const Grid& G, const float seed[3], const Cell& c0, float h, float msq,
                         int max_steps, int* end) {
  float p[3] = {seed[0], seed[1], seed[2]};
  Cell c = c0;
  *end = kEndSteps;
  int steps = 0;
  for (; steps <= max_steps; ++steps) {  // the step after max_steps is never taken
    float k1[3], pn[3];
    Cell cn;
    sample_vector(G, c, k1);
    const int r = advance(G, p, k1, h, msq, steps, max_steps, pn, &cn);
    if (r != kTaken) {
      *end = r;
      break;
    }
    for (int a = 0; a < 3; ++a) p[a] = pn[a];
    c = cn;
  }
  return steps;
}

// ---- tangent and frame ----

struct Frame {
  float T[3], N[3];
};

SPRAY_HD void normalize3(const float x[3], float out[3]) {
  const float l = sqrtf(dot3(x, x));
  for (int a = 0; a < 3; ++a) out[a] = x[a] / l;
}

// N from the axis with the smallest |T_a| (the lowest on a tie): normalised e - T_a T.
SPRAY_HD void axis_normal(const float T[3], float N[3]) {
  int e = 0;
  if (fabsf(T[1]) < fabsf(T[e])) e = 1;
  if (fabsf(T[2]) < fabsf(T[e])) e = 2;
  const float te = e == 0 ? T[0] : (e == 1 ? T[1] : T[2]);
  float w[3];
  for (int a = 0; a < 3; ++a) w[a] = (a == e ? 1.0f : 0.0f) - te * T[a];
  normalize3(w, N);
}

// The frame at a point with k1 = v(point): at the seed from the axis rule,
// else carried from the neighbour nearer the seed (fr on entry).
SPRAY_HD void frame_at(const float k1[3], float msq, bool seed, Frame* fr) {
  float d;
  if (usable(k1, msq, &d)) {
    const float s = sqrtf(d);
    for (int a = 0; a < 3; ++a) fr->T[a] = k1[a] / s;
  }
  if (seed) {
    axis_normal(fr->T, fr->N);
    return;
  }
  const float dt = dot3(fr->N, fr->T);
  float w[3];
  for (int a = 0; a < 3; ++a) w[a] = fr->N[a] - dt * fr->T[a];
  if (dot3(w, w) >= 0.25f)
    normalize3(w, fr->N);
  else
    axis_normal(fr->T, fr->N);
}

SPRAY_HD void cross3(const float a[3], const float b[3], float out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- the tube of a line of m >= 2 points, nsides sides ----
// Vertices: ring j * nsides + k of point j, then the cap centres m * nsides
// (first point) and m * nsides + 1 (last point).  Faces: per segment j and
// side k the triangles (a, c, b) and (b, c, d) of the quad a = (j, k),
// b = (j, k + 1), c = (j + 1, k), d = (j + 1, k + 1); then the fan of the first
// cap (centre, k, k + 1) and of the last cap (centre, k + 1, k) on its ring.

SPRAY_HD uint64_t tube_verts(uint64_t m, uint32_t ns) { return m * ns + 2; }
SPRAY_HD uint64_t tube_faces(uint64_t m, uint32_t ns) { return 2 * uint64_t(ns) * m; }

// Ring vertex: off = c N + s B, the position p + radius off.
SPRAY_HD void ring_vertex(const float p[3], const float N[3], const float B[3], float c, float s,
                          float radius, float pos[3], float off[3]) {
  for (int a = 0; a < 3; ++a) {
    off[a] = c * N[a] + s * B[a];
    pos[a] = p[a] + radius * off[a];
  }
}

// Face r of the tube, as vertex numbers within the tube.
SPRAY_HD void tube_face(uint32_t ns, uint32_t m, uint32_t r, uint32_t f[3]) {
  const uint32_t nside = 2 * ns * (m - 1);
  if (r < nside) {
    const uint32_t q = r >> 1, j = q / ns, k = q - j * ns, k1 = k + 1 == ns ? 0 : k + 1;
    const uint32_t a = j * ns + k, b = j * ns + k1, c = a + ns, d = b + ns;
    f[0] = (r & 1u) ? b : a;
    f[1] = c;
    f[2] = (r & 1u) ? d : b;
    return;
  }
  const uint32_t e = r - nside, last = e >= ns ? 1u : 0u, k = e - last * ns;
  const uint32_t k1 = k + 1 == ns ? 0 : k + 1, ring = last ? (m - 1) * ns : 0;
  f[0] = m * ns + last;
  f[1] = ring + (last ? k1 : k);
  f[2] = ring + (last ? k : k1);
}

}  // namespace strm
}  // namespace spray_rt
