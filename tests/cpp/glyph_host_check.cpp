// glyph_host_check.cpp -- the host restatements of the glyph filter
// (spray_rt_glyphs_host, spray_rt_glyph_sphere_host) as a stand-alone program,
// for a run under the host sanitizers: no GPU, no HIP runtime.
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -DSPRAY_RT_GLYPH_HOST_ONLY \
//       -I<rocm>/include -Iinclude -Ispray_amd/csrc \
//       spray_amd/csrc/glyphs.cpp tests/cpp/glyph_host_check.cpp -o glyph_host_check
//
// Every array is allocated at exactly the size the count call reports, so a
// store or a read past an end is the sanitizer's to find.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spray_rt.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

// Counts, then extracts into exact-size arrays; returns the kept glyphs.
size_t run(const spray_rt_pointset& S, const spray_rt_glyph& G, const spray_rt_grid_color* gc,
           uint32_t V) {
  size_t nv = 0, nf = 0;
  int rc = spray_rt_glyphs_host(&S, &G, gc, &nv, &nf, nullptr, nullptr, nullptr, nullptr, nullptr);
  expect(rc == SPRAY_RT_OK, "count call");
  std::vector<float> v(3 * nv), n(3 * nv);
  std::vector<uint32_t> c(nv), f(3 * nf), ids(nv / V);
  rc = spray_rt_glyphs_host(&S, &G, gc, &nv, &nf, v.data(), n.data(), c.data(), f.data(), ids.data());
  expect(rc == SPRAY_RT_OK, "extraction");
  for (size_t k = 0; k < f.size(); ++k) expect(f[k] < nv, "face index in range");
  for (size_t k = 0; k < v.size(); ++k) expect(std::isfinite(v[k]), "finite position");
  for (size_t k = 0; k < ids.size(); ++k) expect(ids[k] < S.npoints, "point id in range");
  // single arrays
  rc = spray_rt_glyphs_host(&S, &G, gc, nullptr, nullptr, nullptr, nullptr, nullptr, f.data(), nullptr);
  expect(rc == SPRAY_RT_OK, "faces alone");
  rc = spray_rt_glyphs_host(&S, &G, gc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ids.data());
  expect(rc == SPRAY_RT_OK, "point ids alone");
  return ids.size();
}

}  // namespace

int main() {
  for (int level = 0; level <= 3; ++level) {
    size_t nv = 0, nf = 0;
    expect(spray_rt_glyph_sphere_host(level, &nv, &nf, nullptr, nullptr) == SPRAY_RT_OK, "table size");
    std::vector<float> v(3 * nv);
    std::vector<uint32_t> f(3 * nf);
    expect(spray_rt_glyph_sphere_host(level, nullptr, nullptr, v.data(), f.data()) == SPRAY_RT_OK,
           "table");
    for (uint32_t x : f) expect(x < nv, "table face in range");
  }
  expect(spray_rt_glyph_sphere_host(4, nullptr, nullptr, nullptr, nullptr) == SPRAY_RT_ERR_ARG,
         "level 4");

  const size_t np = 37;
  std::vector<float> p(3 * np), vec(3 * np), scales(np), select(np), field(np);
  for (size_t i = 0; i < np; ++i) {
    for (int a = 0; a < 3; ++a) {
      p[3 * i + a] = float(std::sin(1.0 + double(3 * i + a))) * 4.0f;
      vec[3 * i + a] = float(std::cos(2.0 + double(3 * i + a)));
    }
    scales[i] = i % 7 == 0 ? 0.0f : (i % 11 == 0 ? 3e38f : 0.5f + float(i % 5));
    select[i] = float(i % 4);
    field[i] = float(i) / float(np) - 0.25f;
  }
  vec[3] = vec[4] = vec[5] = 0.0f;           // a speed below min_speed
  vec[6] = 0.0f, vec[7] = -0.0f, vec[8] = 2.0f;  // a tie of the axis rule
  const uint32_t table[5] = {0x0000FF, 0x00FF00, 0xFF0000, 0x808080, 0xFFFFFF};
  const spray_rt_grid_color gc = {field.data(), table, 5, 0.0f, 0.5f};

  size_t kept = 0;
  for (uint32_t stride = 1; stride <= 38; stride += 3) {
    for (int level = 0; level <= 3; ++level) {
      spray_rt_pointset S = {p.data(), np, nullptr, scales.data(), select.data(), 1.0f, 3.0f, stride};
      spray_rt_glyph G = {SPRAY_RT_GLYPH_SPHERE, 0.25f, level, 0, 0, 0.0f, 0x123456, 1};
      kept += run(S, G, level % 2 ? &gc : nullptr, 10u * (1u << (2 * level)) + 2u);
    }
    for (int ns = 3; ns <= 16; ++ns) {
      spray_rt_pointset S = {p.data(), np, vec.data(), ns % 2 ? scales.data() : nullptr,
                             ns % 3 ? select.data() : nullptr, 0.0f, 2.0f, stride};
      spray_rt_glyph G = {SPRAY_RT_GLYPH_ARROW, 0.5f, 0, ns, ns % 2, 1e-6f, 0x654321, 0};
      kept += run(S, G, ns % 2 ? nullptr : &gc, 4u * uint32_t(ns) + 1u);
    }
  }
  expect(kept > 500, "the cases keep points");

  // empty sets, every point dropped, the argument and the limit errors
  spray_rt_glyph sph = {SPRAY_RT_GLYPH_SPHERE, 0.25f, 1, 0, 0, 0.0f, 0, 0};
  spray_rt_pointset none = {nullptr, 0, nullptr, nullptr, nullptr, 0.0f, 0.0f, 1};
  expect(run(none, sph, nullptr, 42) == 0, "an empty set");
  std::vector<float> zeros(np, 0.0f);
  spray_rt_pointset dropped = {p.data(), np, nullptr, zeros.data(), nullptr, 0.0f, 0.0f, 1};
  expect(run(dropped, sph, nullptr, 42) == 0, "every point dropped");
  size_t nv = 0, nf = 0;
  spray_rt_pointset bad = {p.data(), np, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0};
  expect(spray_rt_glyphs_host(&bad, &sph, nullptr, &nv, &nf, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == SPRAY_RT_ERR_ARG, "stride 0");
  spray_rt_pointset huge = {p.data(), size_t(1) << 31, nullptr, nullptr, nullptr, 0.0f, 0.0f, 1};
  expect(spray_rt_glyphs_host(&huge, &sph, nullptr, &nv, &nf, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == SPRAY_RT_ERR_LIMIT, "2^31 points, no array read");
  spray_rt_pointset many = {p.data(), (size_t(1) << 29) / 80 + 1, nullptr, nullptr, nullptr, 0.0f, 0.0f, 1};
  expect(spray_rt_glyphs_host(&many, &sph, nullptr, &nv, &nf, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == SPRAY_RT_ERR_LIMIT, "2^29 faces, no array read");
  p[5] = NAN;
  spray_rt_pointset nan_set = {p.data(), np, nullptr, nullptr, nullptr, 0.0f, 0.0f, 5};
  expect(spray_rt_glyphs_host(&nan_set, &sph, nullptr, &nv, &nf, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == SPRAY_RT_ERR_ARG, "a non-finite point");

  std::printf("glyph_host_check: %zu glyphs kept, %d failures\n", kept, failures);
  return failures ? 1 : 0;
}
