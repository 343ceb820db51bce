// refit_common.h -- the arithmetic of a BVH refit, shared by the host
// restatement (refit.cpp) and the gfx950 kernels (refit_kernels.hip).
//
// Each function restates one rule of bvh_build.cpp operation for operation
// (pad, the triangle record of build_bvh, make_qgrid, quant_box), so a refit
// with the vertices a slot was built from reproduces the built bytes.  Both
// translation units are compiled with -ffp-contract=off; the only fused
// operations are the explicit fma calls.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rt_common.h"

namespace spray_rt {
namespace refit {

#define SPRAY_HD __host__ __device__ inline

// status bits of one slot of a refit call
constexpr uint32_t kBadVertex = 1;  // non-finite coordinate of a referenced vertex
constexpr uint32_t kBadGrid = 2;    // make_qgrid's failure
constexpr uint32_t kBadQuant = 4;   // quant_box's failure

SPRAY_HD float pos_inf() { return __builtin_huge_valf(); }
SPRAY_HD bool finite_f(float x) { return x - x == 0.0f; }
// the builder's never-hit box (a root that is itself a leaf has one)
SPRAY_HD bool empty_box(const float* lo) { return lo[0] == pos_inf(); }

// Box::grow_point / Box::grow: strict comparisons, the first value seen stays
SPRAY_HD void grow(float lo[3], float hi[3], const float* plo, const float* phi) {
  for (int j = 0; j < 3; ++j) {
    if (plo[j] < lo[j]) lo[j] = plo[j];
    if (phi[j] > hi[j]) hi[j] = phi[j];
  }
}

// pad(): each bound of a finite box moves out by kBoxPad x max(|lo|, |hi|, extent)
SPRAY_HD void pad_box(float lo[3], float hi[3]) {
  if (!(finite_f(lo[0]) && finite_f(hi[0]))) return;
  for (int j = 0; j < 3; ++j) {
    const float e = hi[j] - lo[j];
    const float m = fmaxf(fmaxf(fabsf(lo[j]), fabsf(hi[j])), e);
    const float p = m * kBoxPad;
    lo[j] = lo[j] - p;
    hi[j] = hi[j] + p;
  }
}

// build_bvh's record: v0, e1 = v0 - v1, e2 = v2 - v0, Ng = e1 x e2 in the
// kernels' explicit FMA form.  Returns whether v0, e1, e2 are finite (the
// check of a slot upload).
SPRAY_HD bool tri_record(const float* a, const float* b, const float* c, float r[12]) {
  r[0] = a[0];
  r[1] = a[1];
  r[2] = a[2];
  r[3] = a[0] - b[0];
  r[4] = a[1] - b[1];
  r[5] = a[2] - b[2];
  r[6] = c[0] - a[0];
  r[7] = c[1] - a[1];
  r[8] = c[2] - a[2];
  r[9] = fmaf(r[4], r[8], -(r[5] * r[7]));
  r[10] = fmaf(r[5], r[6], -(r[3] * r[8]));
  r[11] = fmaf(r[3], r[7], -(r[4] * r[6]));
  bool ok = true;
  for (int k = 0; k < 9; ++k) ok = ok && finite_f(r[k]);
  return ok;
}

// make_qgrid, one axis, from the min / max over the padded finite child boxes
// (lo > hi: there was none).  False: the axis has no representable grid.
SPRAY_HD bool qgrid_axis(float lo, float hi, bool any, float* base, float* scale) {
  if (!any) lo = hi = 0.f;
  double ext = double(hi) - double(lo);
  if (!(ext > 0)) ext = fmax(fabs(double(lo)), 1.0) * 1e-3;
  const double mag = fmax(fabs(double(lo)), fabs(double(hi)));
  *scale = float(fmax(ext / 64000.0, ldexp(mag, -19)));
  *base = float(double(lo) - 700.0 * double(*scale));
  return finite_f(*base) && *scale > 0.f;
}

// quant_box, one axis of a non-empty box: grid coordinates rounded outward
// with one extra step.
SPRAY_HD bool quant_axis(float base, float scale, float bl, float bh, uint16_t* q_lo,
                         uint16_t* q_hi) {
  const double s = scale;
  const double fl = floor((double(bl) - base) / s), fh = ceil((double(bh) - base) / s);
  // outside the grid by far (or NaN): quant_box's final test fails as well
  if (!(fl >= -16.0 && fl <= 70000.0 && fh >= -16.0 && fh <= 70000.0)) return false;
  long ql = long(fl) - 2;
  while (ql > 0 && !(double(fmaf(float(ql), scale, base)) + s <= double(bl))) --ql;
  long qh = long(fh) + 2;
  while (qh < 0xFFFF && !(double(fmaf(float(qh), scale, base)) - s >= double(bh))) ++qh;
  if (ql < 0 || qh > 0xFFFF || !(double(fmaf(float(ql), scale, base)) + s <= double(bl)) ||
      !(double(fmaf(float(qh), scale, base)) - s >= double(bh)))
    return false;
  *q_lo = uint16_t(ql);
  *q_hi = uint16_t(qh);
  return true;
}

// half surface area as the builder and the collapse evaluate it
SPRAY_HD float half_area(const float* lo, const float* hi) {
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return (dx * dy + dy * dz) + dz * dx;
}

// triangles [first, first + count) of a leaf ref
SPRAY_HD void leaf_range(int32_t ref, uint32_t* first, uint32_t* count) {
  const uint32_t u = ~uint32_t(ref);
  *first = u >> 2;
  *count = (u & 3u) + 1u;
}

}  // namespace refit
}  // namespace spray_rt
