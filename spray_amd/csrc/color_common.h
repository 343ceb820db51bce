// color_common.h -- the colour map rule (spray_rt_isosurface_mapped,
// spray_rt_colormap_apply), shared by the host restatements (isosurface.cpp)
// and the gfx950 kernels (iso_kernels.hip).  Both translation units are
// compiled with -ffp-contract=off.
//
// A map is (table_rgb[n], lo, hi), 1 <= n <= kMaxTable, lo < hi finite, and
// scale = float(n) / (hi - lo), evaluated once on the host in float.  A scalar
// g lands in bin trunc((g - lo) * scale), clamped to [0, n - 1]: nearest bin,
// no interpolation between entries, the shape of the Morton cell rule of the
// device build.  The colour is the table entry, copied verbatim.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "refit_common.h"

namespace spray_rt {
namespace cmap {

constexpr int kMaxTable = 4096;
constexpr uint32_t kBadScalar = 1;  // status bit of spray_rt_colormap_apply: a non-finite scalar

// The bin of scalar g (finite) in a table of n entries.
SPRAY_HD uint32_t bin(float g, float lo, float scale, int n) {
  const float x = (g - lo) * scale;
  return !(x >= 0.0f) ? 0u : (x >= float(n) ? uint32_t(n - 1) : uint32_t(int(x)));
}

// scale of a map, false where (n, lo, hi) is no map: n out of range, lo or hi
// not finite, lo >= hi, or a scale that is not a finite normal float.
inline bool map_scale(int n, float lo, float hi, float* scale) {
  if (n < 1 || n > kMaxTable) return false;
  if (!refit::finite_f(lo) || !refit::finite_f(hi) || !(lo < hi)) return false;
  const float s = float(n) / (hi - lo);
  *scale = s;
  return refit::finite_f(s) && s >= 1.17549435e-38f;
}

}  // namespace cmap
}  // namespace spray_rt
