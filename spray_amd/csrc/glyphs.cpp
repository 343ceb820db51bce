// glyphs.cpp -- glyphs of point sets: spray_rt_glyphs (spheres and arrows as
// indexed triangle meshes), spray_rt_domains_glyphs (the meshes into resident
// slots) and the host-only restatements (include/spray_rt.h).
//
// The kept points are found on the device (glyph_kernels.hip) on arrays that
// may already be in HBM: a check pass, a count pass and a scan, the call's one
// host read (the status words and the kept counts), then the place pass into
// context scratch and the expansion into the caller's buffers, or into context
// scratch from where spray_rt_domains_build makes slots.  Nothing is written to
// a slot or a caller buffer before every check has passed (DESIGN.md,
// "Glyphs").
//
// With SPRAY_RT_GLYPH_HOST_ONLY defined the file holds the host restatements
// alone and links without the HIP runtime (tests/cpp/glyph_host_check.cpp).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "color_common.h"
#include "glyph_common.h"
#include "spray_rt.h"

using namespace spray_rt;

namespace {

constexpr uint64_t kMaxPoints = uint64_t(1) << 31;
constexpr uint64_t kMaxVerts = uint64_t(1) << 32;
constexpr uint64_t kMaxFaces = uint64_t(1) << 29;

// What is wrong with a set's description (nullptr: nothing); *code = the error.
const char* set_error(const spray_rt_pointset& S, const spray_rt_glyph& G, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (S.npoints && !S.points) return "null points";
  if (S.stride == 0) return "stride is 0";
  if (G.shape != SPRAY_RT_GLYPH_SPHERE && G.shape != SPRAY_RT_GLYPH_ARROW) return "bad shape";
  if (!(G.size > 0.0f) || !refit::finite_f(G.size)) return "size is not positive and finite";
  if (S.select && (!refit::finite_f(S.select_lo) || !refit::finite_f(S.select_hi) ||
                   !(S.select_lo <= S.select_hi)))
    return "select range is not lo <= hi, both finite";
  if (G.shape == SPRAY_RT_GLYPH_SPHERE) {
    if (G.level < 0 || G.level > glyph::kMaxLevel) return "level is not in 0 .. 3";
  } else {
    if (G.nsides < 3 || G.nsides > glyph::kMaxSides) return "nsides is not in 3 .. 16";
    const float msq = G.min_speed * G.min_speed;
    if (!(G.min_speed > 0.0f) || !refit::finite_f(msq) || !(msq >= 1.17549435e-38f))
      return "min_speed is not positive with a normal square";
    if (S.npoints && !S.vectors) return "arrows without vectors";
  }
  *code = SPRAY_RT_ERR_LIMIT;
  if (uint64_t(S.npoints) >= kMaxPoints) return "2^31 or more points";
  *code = SPRAY_RT_OK;
  return nullptr;
}

// ... with a set's colour map; a set without a colour field has none.
const char* color_error(const spray_rt_grid_color* gc, float* scale) {
  *scale = 0.0f;
  if (!gc || !gc->field) return nullptr;
  if (!gc->table_rgb) return "null colour table";
  if (gc->ntable < 1 || gc->ntable > cmap::kMaxTable)
    return "colour table of fewer than 1 or more than 4096 entries";
  if (!refit::finite_f(gc->lo) || !refit::finite_f(gc->hi) || !(gc->lo < gc->hi))
    return "colour range is not lo < hi, both finite";
  if (!cmap::map_scale(gc->ntable, gc->lo, gc->hi, scale))
    return "colour scale ntable / (hi - lo) is not a finite normal float";
  return nullptr;
}

uint32_t verts_per(const spray_rt_glyph& G) {
  return G.shape == SPRAY_RT_GLYPH_SPHERE ? glyph::sphere_verts(G.level)
                                          : glyph::arrow_verts(uint32_t(G.nsides));
}
uint32_t faces_per(const spray_rt_glyph& G) {
  return G.shape == SPRAY_RT_GLYPH_SPHERE ? glyph::sphere_faces(G.level)
                                          : glyph::arrow_faces(uint32_t(G.nsides));
}

// What is wrong with a set's totals (nullptr: nothing).
const char* totals_error(uint64_t nglyphs, const spray_rt_glyph& G) {
  if (nglyphs * verts_per(G) >= kMaxVerts) return "2^32 or more vertices";
  if (nglyphs * faces_per(G) >= kMaxFaces) return "2^29 or more faces";
  return nullptr;
}

// Whether every candidate of the set is kept whatever its arrays hold: then
// the totals follow from the counts alone.
bool keeps_every_candidate(const spray_rt_pointset& S, const spray_rt_glyph& G) {
  return G.shape == SPRAY_RT_GLYPH_SPHERE && !S.select && !S.scales;
}
uint64_t candidates(const spray_rt_pointset& S) {
  return (uint64_t(S.npoints) + S.stride - 1) / S.stride;
}

glyph::Keep keep_of(const spray_rt_pointset& S, const spray_rt_glyph& G) {
  glyph::Keep K;
  const bool arrow = G.shape == SPRAY_RT_GLYPH_ARROW;
  K.vectors = arrow ? S.vectors : nullptr;
  K.scales = S.scales;
  K.select = S.select;
  K.select_lo = S.select_lo;
  K.select_hi = S.select_hi;
  K.stride = S.stride;
  K.size = G.size;
  K.msq = arrow ? G.min_speed * G.min_speed : 0.0f;
  K.arrow = arrow;
  K.scale_by_vector = arrow && G.scale_by_vector != 0;
  return K;
}

void ring_table(int nsides, float out[][2]) {
  for (int k = 0; k < nsides; ++k) {
    const double a = (6.283185307179586 * double(k)) / double(nsides);
    out[k][0] = float(std::cos(a));
    out[k][1] = float(std::sin(a));
  }
}

void cone_constants(float* cn, float* ct) {
  const double h = std::hypot(0.35, 0.1);
  *cn = float(0.35 / h);
  *ct = float(0.1 / h);
}

// The unit icosphere of a level, built in double: the icosahedron, then `level`
// midpoint subdivisions, every vertex normalised in double, cast at the end.
struct SphereTable {
  std::vector<float> verts;     // [V][3]
  std::vector<uint32_t> faces;  // [F][3]
};
SphereTable make_sphere(int level) {
  const double t = (1.0 + std::sqrt(5.0)) / 2.0;
  const double ico[12][3] = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t},
                             {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
  // (v0 - v1) x (v2 - v0) points outward
  const uint32_t tri[20][3] = {{0, 5, 11}, {0, 1, 5}, {0, 7, 1}, {0, 10, 7}, {0, 11, 10},
                               {1, 9, 5}, {5, 4, 11}, {11, 2, 10}, {10, 6, 7}, {7, 8, 1},
                               {3, 4, 9}, {3, 2, 4}, {3, 6, 2}, {3, 8, 6}, {3, 9, 8},
                               {4, 5, 9}, {2, 11, 4}, {6, 10, 2}, {8, 7, 6}, {9, 1, 8}};
  std::vector<double> v;
  auto push = [&](double x, double y, double z) {
    const double l = std::sqrt((x * x + y * y) + z * z);
    v.push_back(x / l);
    v.push_back(y / l);
    v.push_back(z / l);
    return uint32_t(v.size() / 3 - 1);
  };
  for (const auto& p : ico) push(p[0], p[1], p[2]);
  std::vector<uint32_t> f;
  for (const auto& q : tri) f.insert(f.end(), q, q + 3);
  for (int l = 0; l < level; ++l) {
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> mid;
    auto midpoint = [&](uint32_t a, uint32_t b) {
      const auto key = std::make_pair(a < b ? a : b, a < b ? b : a);
      const auto it = mid.find(key);
      if (it != mid.end()) return it->second;
      const uint32_t lo = key.first, hi = key.second;  // the sum in index order: one result per edge
      const uint32_t m = push(0.5 * (v[3 * lo] + v[3 * hi]), 0.5 * (v[3 * lo + 1] + v[3 * hi + 1]),
                              0.5 * (v[3 * lo + 2] + v[3 * hi + 2]));
      mid.emplace(key, m);
      return m;
    };
    std::vector<uint32_t> g;
    g.reserve(4 * f.size());
    for (size_t r = 0; r < f.size(); r += 3) {
      const uint32_t a = f[r], b = f[r + 1], c = f[r + 2];
      const uint32_t ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
      const uint32_t four[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
      g.insert(g.end(), four, four + 12);
    }
    f.swap(g);
  }
  SphereTable T;
  T.verts.resize(v.size());
  for (size_t k = 0; k < v.size(); ++k) T.verts[k] = float(v[k]);
  T.faces = f;
  return T;
}
const SphereTable& sphere_table(int level) {
  static const SphereTable tables[glyph::kMaxLevel + 1] = {make_sphere(0), make_sphere(1),
                                                          make_sphere(2), make_sphere(3)};
  return tables[level];
}

// The check pass on the host: the first kind that applies, in the kernels' order.
uint32_t check_host(const spray_rt_pointset& S, const spray_rt_glyph& G, const float* cfield) {
  const size_t np = S.npoints;
  uint32_t bad = 0;
  for (size_t e = 0; e < 3 * np; ++e)
    if (!refit::finite_f(S.points[e])) bad |= glyph::kBadPoint;
  if (G.shape == SPRAY_RT_GLYPH_ARROW)
    for (size_t e = 0; e < 3 * np; ++e)
      if (!refit::finite_f(S.vectors[e])) bad |= glyph::kBadVector;
  if (S.scales)
    for (size_t e = 0; e < np; ++e) {
      if (!refit::finite_f(S.scales[e]))
        bad |= glyph::kBadScale;
      else if (S.scales[e] < 0.0f)
        bad |= glyph::kNegScale;
    }
  if (S.select)
    for (size_t e = 0; e < np; ++e)
      if (!refit::finite_f(S.select[e])) bad |= glyph::kBadSelect;
  if (cfield)
    for (size_t e = 0; e < np; ++e)
      if (!refit::finite_f(cfield[e])) bad |= glyph::kBadColor;
  return bad;
}

const char* status_error(uint32_t status) {
  if (status & glyph::kBadPoint) return "non-finite point coordinate";
  if (status & glyph::kBadVector) return "non-finite vector component";
  if (status & glyph::kBadScale) return "non-finite scale";
  if (status & glyph::kNegScale) return "negative scale";
  if (status & glyph::kBadSelect) return "non-finite select value";
  if (status & glyph::kBadColor) return "non-finite sample of the colour field";
  return nullptr;
}

}  // namespace

extern "C" {

int spray_rt_glyph_sphere_host(int32_t level, size_t* nverts, size_t* nfaces, float* verts_out,
                               uint32_t* faces_out) {
  if (nverts) *nverts = 0;
  if (nfaces) *nfaces = 0;
  if (level < 0 || level > glyph::kMaxLevel) return SPRAY_RT_ERR_ARG;
  const SphereTable& T = sphere_table(level);
  if (nverts) *nverts = T.verts.size() / 3;
  if (nfaces) *nfaces = T.faces.size() / 3;
  if (verts_out) std::memcpy(verts_out, T.verts.data(), T.verts.size() * sizeof(float));
  if (faces_out) std::memcpy(faces_out, T.faces.data(), T.faces.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_glyphs_host(const spray_rt_pointset* set, const spray_rt_glyph* g,
                         const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                         float* verts_out, float* vnormals_out, uint32_t* colors_out,
                         uint32_t* faces_out, uint32_t* point_ids_out) {
  if (nverts) *nverts = 0;
  if (nfaces) *nfaces = 0;
  if (!set || !g) return SPRAY_RT_ERR_ARG;
  const spray_rt_pointset& S = *set;
  const spray_rt_glyph& G = *g;
  int code;
  if (set_error(S, G, &code)) return code;
  float cscale;
  if (color_error(gcolor, &cscale)) return SPRAY_RT_ERR_ARG;
  const uint32_t V = verts_per(G), F = faces_per(G);
  if (keeps_every_candidate(S, G) && totals_error(candidates(S), G)) {
    if (nverts) *nverts = size_t(candidates(S) * V);
    if (nfaces) *nfaces = size_t(candidates(S) * F);
    return SPRAY_RT_ERR_LIMIT;  // from the counts: no array has been read
  }
  const float* cf = gcolor ? gcolor->field : nullptr;
  if (check_host(S, G, cf)) return SPRAY_RT_ERR_ARG;
  const glyph::Keep K = keep_of(S, G);
  const uint32_t np = uint32_t(S.npoints);
  uint64_t kept = 0;
  for (uint32_t i = 0; i < np; ++i) {
    float s, d;
    if (glyph::keep(K, i, &s, &d)) ++kept;
  }
  if (nverts) *nverts = size_t(kept * V);
  if (nfaces) *nfaces = size_t(kept * F);
  if (totals_error(kept, G)) return SPRAY_RT_ERR_LIMIT;
  if (!verts_out && !vnormals_out && !colors_out && !faces_out && !point_ids_out)
    return SPRAY_RT_OK;
  const bool arrow = K.arrow;
  const uint32_t ns = uint32_t(G.nsides);
  float ring[glyph::kMaxSides][2] = {};
  float cn = 0.0f, ct = 0.0f;
  const SphereTable* tab = nullptr;
  if (arrow) {
    ring_table(G.nsides, ring);
    cone_constants(&cn, &ct);
  } else {
    tab = &sphere_table(G.level);
  }
  size_t gi = 0;
  for (uint32_t i = 0; i < np; ++i) {
    float s, d;
    if (!glyph::keep(K, i, &s, &d)) continue;
    const float* p = S.points + 3 * size_t(i);
    const uint32_t color =
        cf ? gcolor->table_rgb[cmap::bin(cf[i], gcolor->lo, cscale, gcolor->ntable)] : G.color_rgb;
    float T[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 0.f, 0.f}, B[3] = {0.f, 0.f, 0.f};
    if (arrow) {
      const float l = sqrtf(d);
      for (int a = 0; a < 3; ++a) T[a] = S.vectors[3 * size_t(i) + size_t(a)] / l;
      strm::axis_normal(T, N);
      strm::cross3(T, N, B);
    }
    const size_t v0 = gi * V, f0 = gi * F;
    for (uint32_t k = 0; k < V; ++k) {
      float pos[3], nrm[3];
      if (arrow) {
        const uint32_t j = k / ns, kk = j < 4 ? k - j * ns : 0u;
        glyph::arrow_vertex(p, T, N, B, s, ns, k, ring[kk][0], ring[kk][1], cn, ct, pos, nrm);
      } else {
        glyph::sphere_vertex(p, s, &tab->verts[3 * size_t(k)], pos, nrm);
      }
      for (int a = 0; a < 3; ++a) {
        if (verts_out) verts_out[3 * (v0 + k) + size_t(a)] = pos[a];
        if (vnormals_out) vnormals_out[3 * (v0 + k) + size_t(a)] = nrm[a];
      }
      if (colors_out) colors_out[v0 + k] = color;
    }
    for (uint32_t r = 0; faces_out && r < F; ++r) {
      uint32_t f[3];
      if (arrow)
        glyph::arrow_face(ns, r, f);
      else
        for (int a = 0; a < 3; ++a) f[a] = tab->faces[3 * size_t(r) + size_t(a)];
      for (int a = 0; a < 3; ++a) faces_out[3 * (f0 + r) + size_t(a)] = uint32_t(v0) + f[a];
    }
    if (point_ids_out) point_ids_out[gi] = i;
    ++gi;
  }
  return SPRAY_RT_OK;
}

}  // extern "C"

#ifndef SPRAY_RT_GLYPH_HOST_ONLY
// ---- the device extraction: check, count, scan, the host read, place, expand ----
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>

#include "glyph_kernels.h"
#include "rt_common.h"
#include "rt_ctx.h"

using namespace spray_rt::detail;

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

struct GlyphCall {
  HeadTake<GlyphJob> jobs;  // in the context's glyph arena
  HeadTake<GlyphOut> outs;
  size_t m_outs = 0;  // the mark in front of outs
  uint32_t max_blocks = 0;
  bool staged = false;  // some array came from host memory
  std::vector<uint64_t> nglyphs, nverts, nfaces;
};

// Validates the sets (their glyphs and colour maps), runs the check pass, the
// count pass and the scan and reads the status words and the kept counts (the
// host read).  Messages name the set, and its slot where slots is given.
int glyph_count(spray_rt_ctx* c, const char* what, int n, const spray_rt_pointset* sets,
                const spray_rt_glyph* glyphs, const spray_rt_grid_color* gcolors, const int* slots,
                GlyphCall* call) {
  const size_t nj = size_t(n);
  auto name = [&](int i) {
    char buf[96];
    if (slots)
      snprintf(buf, sizeof(buf), "%s (set %d, slot %d)", what, i, slots[i]);
    else
      snprintf(buf, sizeof(buf), "%s (set %d)", what, i);
    return std::string(buf);
  };
  if (n > 65535) return fail(c, SPRAY_RT_ERR_LIMIT, "%s: more than 65535 sets in one call", what);
  std::vector<float> cscale(nj, 0.0f);
  for (int i = 0; i < n; ++i) {
    int code;
    if (const char* why = set_error(sets[i], glyphs[i], &code))
      return fail(c, code, "%s: %s", name(i).c_str(), why);
    if (gcolors)
      if (const char* why = color_error(&gcolors[i], &cscale[size_t(i)]))
        return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", name(i).c_str(), why);
    if (keeps_every_candidate(sets[i], glyphs[i]))
      if (const char* why = totals_error(candidates(sets[i]), glyphs[i]))
        return fail(c, SPRAY_RT_ERR_LIMIT, "%s: %s", name(i).c_str(), why);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then arrays and scratch ----
  JobArena& A = c->glyph;
  A.reset();
  call->jobs = A.take_head<GlyphJob>(nj);
  const size_t m_status = A.mark();
  const auto t_status = A.take_head<uint32_t>(nj);
  const auto t_count = A.take_head<GlyphCount>(nj);
  call->m_outs = A.mark();
  call->outs = A.take_head<GlyphOut>(nj);
  struct Scratch {
    Take<uint32_t> word, bbase;
    uint32_t nblocks;
  };
  std::vector<Scratch> sk(nj);
  // items 0 .. 7: the sphere tables of the levels (vertices, faces), once per
  // call for the levels in use; items 8 + 6 i ..: set i's points, vectors,
  // scales, select values, colour field and colour table, host ones staged
  // inside the arena
  Stager stage;
  bool level_used[glyph::kMaxLevel + 1] = {};
  for (int i = 0; i < n; ++i)
    if (glyphs[i].shape == SPRAY_RT_GLYPH_SPHERE) level_used[glyphs[i].level] = true;
  for (int l = 0; l <= glyph::kMaxLevel; ++l) {
    const SphereTable* T = level_used[l] ? &sphere_table(l) : nullptr;  // static: outlives the copy
    stage.place(T ? T->verts.data() : nullptr, T ? T->verts.size() * sizeof(float) : 0, &A);
    stage.place(T ? T->faces.data() : nullptr, T ? T->faces.size() * sizeof(uint32_t) : 0, &A);
  }
  stage.any = false;  // the tables are the library's own: they outlive the copy
  for (int i = 0; i < n; ++i) {
    const spray_rt_pointset& S = sets[i];
    Scratch& k = sk[size_t(i)];
    const size_t np = S.npoints;
    const bool arrow = glyphs[i].shape == SPRAY_RT_GLYPH_ARROW;
    const spray_rt_grid_color* gc = gcolors && gcolors[i].field ? &gcolors[i] : nullptr;
    k.nblocks = uint32_t((np + glyph::kBlock - 1) / glyph::kBlock);
    stage.place(S.points, 3 * np * sizeof(float), &A);
    stage.place(arrow ? S.vectors : nullptr, 3 * np * sizeof(float), &A);
    stage.place(S.scales, np * sizeof(float), &A);
    stage.place(S.select, np * sizeof(float), &A);
    stage.place(gc ? gc->field : nullptr, np * sizeof(float), &A);
    stage.place(gc ? gc->table_rgb : nullptr, gc ? size_t(gc->ntable) * sizeof(uint32_t) : 0, &A);
    k.word = A.take<uint32_t>(np);
    k.bbase = A.take<uint32_t>(k.nblocks);
    call->max_blocks = std::max(call->max_blocks, k.nblocks);
  }
  call->staged = stage.any;  // a caller's host array
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  GlyphJob* jobs = A.host(call->jobs);
  uint32_t* h_status = A.host(t_status);
  GlyphCount* h_count = A.host(t_count);
  for (int i = 0; i < n; ++i) {
    const spray_rt_pointset& S = sets[i];
    const spray_rt_glyph& G = glyphs[i];
    const Scratch& k = sk[size_t(i)];
    const size_t b = 8 + 6 * size_t(i);
    const bool arrow = G.shape == SPRAY_RT_GLYPH_ARROW;
    GlyphJob J{};
    J.points = stage.dev<float>(b);
    J.vectors = stage.dev<float>(b + 1);
    J.scales = stage.dev<float>(b + 2);
    J.select = stage.dev<float>(b + 3);
    if (gcolors && gcolors[i].field) {
      J.cfield = stage.dev<float>(b + 4);
      J.ctable = stage.dev<uint32_t>(b + 5);
      J.ntable = gcolors[i].ntable;
      J.clo = gcolors[i].lo;
      J.cscale = cscale[size_t(i)];
    }
    if (!arrow) {
      J.tverts = stage.dev<float>(2 * size_t(G.level));
      J.tfaces = stage.dev<uint32_t>(2 * size_t(G.level) + 1);
    }
    J.word = A.dev(k.word);
    J.bbase = A.dev(k.bbase);
    J.count = A.dev(t_count) + i;
    J.npoints = uint32_t(S.npoints);
    J.nblocks = k.nblocks;
    J.stride = S.stride;
    J.select_lo = S.select_lo;
    J.select_hi = S.select_hi;
    J.size = G.size;
    J.shape = G.shape;
    J.V = verts_per(G);
    J.F = faces_per(G);
    J.color = G.color_rgb;
    if (arrow) {
      J.msq = G.min_speed * G.min_speed;
      J.nsides = G.nsides;
      J.scale_by_vector = G.scale_by_vector ? 1 : 0;
      ring_table(G.nsides, J.ring);
      cone_constants(&J.cn, &J.ct);
    }
    jobs[i] = J;
    h_status[i] = 0;
    h_count[i] = GlyphCount{0, 0};
  }
  HIPCHK(c, arena_copy(A, 0, call->m_outs, true, s));
  const GlyphJob* d_jobs = A.dev(call->jobs);
  HIPCHK(c, launch_glyph_check(s, d_jobs, n, call->max_blocks, A.dev(t_status)));
  HIPCHK(c, launch_glyph_count(s, d_jobs, n, call->max_blocks));
  HIPCHK(c, launch_glyph_scan(s, d_jobs, n));
  HIPCHK(c, arena_copy(A, m_status, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the status words and the counts: the call's host read
  call->nglyphs.assign(nj, 0);
  call->nverts.assign(nj, 0);
  call->nfaces.assign(nj, 0);
  for (int i = 0; i < n; ++i) {
    if (const char* why = status_error(h_status[i]))
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", name(i).c_str(), why);
    const uint64_t kept = h_count[i].kept;
    call->nglyphs[size_t(i)] = kept;
    call->nverts[size_t(i)] = kept * verts_per(glyphs[i]);
    call->nfaces[size_t(i)] = kept * faces_per(glyphs[i]);
    if (const char* why = totals_error(kept, glyphs[i]))
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: %s", name(i).c_str(), why);
  }
  return SPRAY_RT_OK;
}

// The place pass of a counted call into outs[n], then the expansion.
int glyph_emit(spray_rt_ctx* c, int n, const GlyphCall& call, const std::vector<GlyphOut>& outs) {
  hipStream_t s = stream_of(c);
  const JobArena& A = c->glyph;
  std::memcpy(A.host(call.outs), outs.data(), size_t(n) * sizeof(GlyphOut));
  HIPCHK(c, arena_copy(A, call.m_outs, call.m_outs + size_t(n) * sizeof(GlyphOut), true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  HIPCHK(c, launch_glyph_place(s, A.dev(call.jobs), A.dev(call.outs), n, call.max_blocks));
  uint64_t max_items = 0;
  for (int i = 0; i < n; ++i)
    max_items = std::max(max_items, std::max(outs[size_t(i)].cap_verts, outs[size_t(i)].cap_faces));
  HIPCHK(c, launch_glyph_expand(s, A.dev(call.jobs), A.dev(call.outs), n, max_items));
  return SPRAY_RT_OK;
}

}  // namespace

extern "C" {

int spray_rt_glyph_phase_times(spray_rt_ctx_t c, double out_ms[3]) {
  if (!c || !out_ms) return SPRAY_RT_ERR_ARG;
  for (int k = 0; k < 3; ++k) out_ms[k] = c->glyph_ms[k];
  return SPRAY_RT_OK;
}

int spray_rt_glyphs(spray_rt_ctx_t c, int n, const spray_rt_pointset* sets,
                    const spray_rt_glyph* glyphs, const spray_rt_grid_color* gcolors,
                    float* const* verts, float* const* vnormals, uint32_t* const* colors,
                    uint32_t* const* faces, uint32_t* const* point_ids, const size_t* cap_verts,
                    const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!sets || !glyphs)) ||
      (n && (verts || vnormals || colors || point_ids) && !cap_verts) ||
      (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "glyphs: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const auto t0 = Clock::now();
  c->glyph_ms[0] = c->glyph_ms[1] = c->glyph_ms[2] = 0.0;
  GlyphCall call;
  const int r = glyph_count(c, "glyphs", n, sets, glyphs, gcolors, nullptr, &call);
  c->glyph_ms[0] = ms_since(t0);
  if (r) return r;
  for (int i = 0; i < n; ++i) {
    if (nverts_out) nverts_out[i] = size_t(call.nverts[size_t(i)]);
    if (nfaces_out) nfaces_out[i] = size_t(call.nfaces[size_t(i)]);
  }
  if (!verts && !vnormals && !colors && !faces && !point_ids) return SPRAY_RT_OK;
  const auto t1 = Clock::now();
  const size_t nj = size_t(n);
  std::vector<GlyphOut> outs(nj, GlyphOut{});
  std::vector<Take<GlyphRec>> t_recs(nj);
  Layout M;  // of d_isomesh
  bool any = false;
  for (int i = 0; i < n; ++i) {
    GlyphOut& O = outs[size_t(i)];
    O.verts = verts ? verts[i] : nullptr;
    O.vnormals = vnormals ? vnormals[i] : nullptr;
    O.colors = colors ? colors[i] : nullptr;
    O.faces = faces ? faces[i] : nullptr;
    O.point_ids = point_ids ? point_ids[i] : nullptr;
    const bool per_vertex = O.verts || O.vnormals || O.colors;
    const uint64_t nv = call.nverts[size_t(i)], nf = call.nfaces[size_t(i)];
    if (((per_vertex || O.point_ids) && nv > cap_verts[i]) || (O.faces && nf > cap_faces[i]))
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "glyphs (set %d): %llu vertices and %llu faces do not fit the buffers", i,
                  static_cast<unsigned long long>(nv), static_cast<unsigned long long>(nf));
    O.nglyphs = call.nglyphs[size_t(i)];
    O.cap_verts = per_vertex ? nv : 0;
    O.cap_faces = O.faces ? nf : 0;
    if (per_vertex) t_recs[size_t(i)] = M.take<GlyphRec>(size_t(O.nglyphs));
    any = any || per_vertex || O.faces || O.point_ids;
  }
  if (!any) return SPRAY_RT_OK;
  const int g = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (g) return g;
  for (size_t k = 0; k < nj; ++k)
    if (t_recs[k]) outs[k].recs = t_recs[k].at(c->d_isomesh);
  const int e = glyph_emit(c, n, call, outs);
  if (e) return e;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->glyph_ms[1] = ms_since(t1);
  return SPRAY_RT_OK;
}

int spray_rt_domains_glyphs(spray_rt_ctx_t c, int n, const int* slots,
                            const spray_rt_pointset* sets, const spray_rt_glyph* glyphs,
                            const spray_rt_grid_color* gcolors, int with_normals, float* d_bounds,
                            size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!slots || !sets || !glyphs)))
    return fail(c, SPRAY_RT_ERR_ARG, "glyphs: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const size_t nj = size_t(n);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] > 1 << 20)
      return fail(c, SPRAY_RT_ERR_ARG, "glyphs (set %d): bad slot %d", i, slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail(c, SPRAY_RT_ERR_ARG, "glyphs (set %d): slot %d listed twice", i, slots[i]);
  }
  const auto t0 = Clock::now();
  c->glyph_ms[0] = c->glyph_ms[1] = c->glyph_ms[2] = 0.0;
  GlyphCall call;
  int r = glyph_count(c, "glyphs", n, sets, glyphs, gcolors, slots, &call);
  c->glyph_ms[0] = ms_since(t0);
  if (r) return r;

  // ---- the records and the meshes: context scratch, at the exact sizes ----
  const auto t1 = Clock::now();
  Layout M;  // of d_isomesh
  std::vector<GlyphOut> outs(nj, GlyphOut{});
  std::vector<Take<GlyphRec>> t_recs(nj);
  std::vector<Take<float>> t_verts(nj), t_normals(nj);
  std::vector<Take<uint32_t>> t_colors(nj), t_faces(nj);
  std::vector<size_t> nv(nj), nf(nj);
  for (size_t k = 0; k < nj; ++k) {
    outs[k].nglyphs = call.nglyphs[k];
    outs[k].cap_verts = nv[k] = size_t(call.nverts[k]);
    outs[k].cap_faces = nf[k] = size_t(call.nfaces[k]);
    t_recs[k] = M.take<GlyphRec>(size_t(call.nglyphs[k]));
    t_verts[k] = M.take<float>(3 * nv[k]);
    if (with_normals) t_normals[k] = M.take<float>(3 * nv[k]);
    if (glyphs[k].has_color || (gcolors && gcolors[k].field)) t_colors[k] = M.take<uint32_t>(nv[k]);
    t_faces[k] = M.take<uint32_t>(3 * nf[k]);
  }
  r = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (r) return r;
  std::vector<const float*> pv(nj), pn(nj);
  std::vector<const uint32_t*> pc(nj), pf(nj);
  for (size_t k = 0; k < nj; ++k) {
    GlyphOut& O = outs[k];
    O.recs = t_recs[k].at(c->d_isomesh);
    pv[k] = O.verts = t_verts[k].at(c->d_isomesh);
    pn[k] = O.vnormals = t_normals[k] ? t_normals[k].at(c->d_isomesh) : nullptr;
    pc[k] = O.colors = t_colors[k] ? t_colors[k].at(c->d_isomesh) : nullptr;
    pf[k] = O.faces = t_faces[k].at(c->d_isomesh);
  }
  r = glyph_emit(c, n, call, outs);
  if (r) return r;
  c->glyph_ms[1] = ms_since(t1);

  // ---- the slots: the device build on the expanded arrays ----
  const auto t2 = Clock::now();
  int job = -1;  // the build names the slot; name the set as well
  r = domains_build(c, n, slots, pv.data(), nv.data(), pf.data(), nf.data(), pc.data(), pn.data(),
                    d_bounds, &job);
  if (r) {
    const std::string msg = c->err;
    if (job >= 0)
      return fail(c, r, "glyphs (set %d, slot %d): %s", job, slots[job], msg.c_str());
    return fail(c, r, "glyphs: %s", msg.c_str());
  }
  if (nfaces_out)
    for (size_t k = 0; k < nj; ++k) nfaces_out[k] = nf[k];
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->glyph_ms[2] = ms_since(t2);
  return SPRAY_RT_OK;
}

}  // extern "C"
#endif  // SPRAY_RT_GLYPH_HOST_ONLY
