// cell_clip.cpp -- clips of unstructured meshes of hexahedra, wedges, pyramids
// and tets by a level of their scalar field: spray_rt_cell_clip,
// spray_rt_domains_cell_clip, spray_rt_plane_values and the host-only
// restatements (include/spray_rt.h).
//
// The clipped solid's surface is a cap and a skin.  The cap is the cell
// isosurface, entered below its C wrappers (tet_pipeline.h: the cell pass, the
// split of the crossing cells, count and weld), whose sorted instance keys stay
// in the context.  The skin is the boundary of the cells with a kept point
// (surf_kernels.hip's keys and unique pass on clip_kernels.hip's count), each
// triangle cut by the kept bits of its corners; a corner on a cut edge is the
// cap vertex a binary search of the pair finds among those keys.  Five host
// reads: the cap's three, the skin's status and face-instance totals, its
// vertex and piece counts.  Nothing is written to a slot or a caller buffer
// before every check has passed ("Clips of cell meshes").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "clip_common.h"
#include "clip_kernels.h"
#include "rt_common.h"
#include "rt_ctx.h"
#include "spray_rt.h"
#include "surf_kernels.h"
#include "tet_kernels.h"
#include "tet_pipeline.h"

using namespace spray_rt;
using namespace spray_rt::detail;

namespace {

constexpr uint64_t kMaxCells = uint64_t(1) << 29;
constexpr uint64_t kMaxFaces = uint64_t(1) << 29;
constexpr uint64_t kMaxConn = uint64_t(1) << 32;
constexpr uint64_t kMaxInst = uint64_t(1) << 32;
constexpr const char* kWhat = "cell clip";

// What is wrong with a mesh's description (nullptr: nothing).
const char* mesh_error(const spray_rt_cellmesh& m, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (m.ncells && (!m.types || !m.offsets || !m.conn)) return "null types, offsets or conn";
  if (m.ncells && (!m.points || !m.values)) return "null points or values";
  if (!refit::finite_f(m.isovalue)) return "non-finite isovalue";
  *code = SPRAY_RT_ERR_LIMIT;
  if (uint64_t(m.npoints) > surf::kMaxPoints) return "more than 2^21 points";
  if (uint64_t(m.ncells) >= kMaxCells) return "2^29 or more cells";
  if (uint64_t(m.nconn) >= kMaxConn) return "2^32 or more listed point indices";
  *code = SPRAY_RT_OK;
  return nullptr;
}

// What the status bits of a mesh say.
const char* status_error(uint32_t st) {
  if (st & cell::kBadType) return "unknown cell type";
  if (st & cell::kBadOffsets) return "offsets of a cell do not match its type's point count";
  if (st & cell::kBadConn) return "offsets of a cell beyond nconn";
  if (st & tet::kBadIndex) return "point index out of range";
  if (st & tet::kBadPoint) return "non-finite coordinate of a referenced point";
  if (st & tet::kBadSample) return "non-finite value at a referenced point";
  if (st & tet::kBadColor) return "non-finite sample of the colour field at a referenced point";
  if (st & tet::kBadNormal) return "non-finite normal of a referenced point";
  return nullptr;
}

struct HostClip {
  std::vector<float> verts, normals, vt;
  std::vector<uint32_t> faces, colors, pairs;
  uint64_t nverts = 0, nfaces = 0, ncap_verts = 0, ncap_faces = 0;
};

// The clip on the host: the kernels' passes, one after the other.
int clip_host(const spray_rt_cellmesh& m, uint32_t invert, const spray_rt_grid_color* gc,
              bool emit, bool with_normals, HostClip* out) {
  int code;
  if (mesh_error(m, &code)) return code;
  float cscale;
  if (tet_color_error(gc, &cscale)) return SPRAY_RT_ERR_ARG;
  if (with_normals && !m.point_normals) return SPRAY_RT_ERR_ARG;
  const float* cf = gc ? gc->field : nullptr;
  const float* pn = with_normals ? m.point_normals : nullptr;
  const size_t nc = m.ncells;
  const int w = tet::index_bits(m.npoints);
  // count: every check, the cells that take part and the first instance of each
  std::vector<uint8_t> nfaces(nc);
  std::vector<uint64_t> first(nc);
  uint64_t ninst = 0;
  for (size_t i = 0; i < nc; ++i) {
    const surf::Cell C = clip::classify(m.points, m.types, m.offsets, m.conn, m.values, cf, pn,
                                        m.npoints, m.nconn, i, m.isovalue, invert);
    if (C.status) return SPRAY_RT_ERR_ARG;
    nfaces[i] = uint8_t(C.nfaces);
    first[i] = ninst;
    ninst += C.nfaces;
  }
  if (ninst >= kMaxInst) return SPRAY_RT_ERR_LIMIT;
  // the cap: the pairs of the tet split's edges whose ends differ, ascending,
  // and the cell isosurface's counts
  std::vector<uint64_t> ukeys;
  for (size_t i = 0; i < nc; ++i) {
    uint32_t tets[24];
    cell::split(m.types[i], m.conn + m.offsets[i], tets);
    for (int t = 0; t < cell::cell_tets(m.types[i]); ++t)
      for (int k = 0; k < 6; ++k) {
        const uint32_t pu = tets[4 * t + tet::edge_u(k)], pw = tets[4 * t + tet::edge_w(k)];
        if (iso::inside(m.values[pu], m.isovalue) != iso::inside(m.values[pw], m.isovalue))
          ukeys.push_back(tet::pair_key(std::min(pu, pw), std::max(pu, pw), 32));
      }
  }
  std::sort(ukeys.begin(), ukeys.end());
  ukeys.erase(std::unique(ukeys.begin(), ukeys.end()), ukeys.end());
  size_t ncv = 0, ncf = 0;
  if (const int r = spray_rt_cell_isosurface_host(&m, gc, &ncv, &ncf, nullptr, nullptr, nullptr,
                                                  nullptr))
    return r;
  if (ncv != ukeys.size()) return SPRAY_RT_ERR_STATE;
  // the skin's source: keys, the sort, the keys that occur once
  std::vector<std::pair<uint64_t, uint64_t>> inst;
  inst.reserve(size_t(ninst));
  for (size_t i = 0; i < nc; ++i)
    for (int f = 0; f < int(nfaces[i]); ++f) {
      const surf::Face F =
          surf::face_points(surf::face_of(m.types[i], f), m.conn + m.offsets[i]);
      inst.emplace_back(surf::face_key(F, w), first[i] + uint64_t(f));
    }
  std::sort(inst.begin(), inst.end());
  std::vector<uint8_t> alive(inst.size(), 0);
  for (size_t k = 0; k < inst.size(); ++k)
    alive[size_t(inst[k].second)] = (k == 0 || inst[k - 1].first != inst[k].first) &&
                                    (k + 1 == inst.size() || inst[k + 1].first != inst[k].first);
  // the pieces and the kept points they use; with emit, the pieces themselves
  // as (point, point) corners, a kept point twice
  std::vector<uint32_t> vid(nc ? m.npoints : 0, UINT32_MAX);
  std::vector<uint32_t> corners;  // [npieces][3][2]
  uint64_t np = 0;
  for (size_t i = 0; i < nc; ++i)
    for (int f = 0; f < int(nfaces[i]); ++f) {
      if (!alive[size_t(first[i]) + size_t(f)]) continue;
      const uint32_t* P = m.conn + m.offsets[i];
      const uint32_t face = surf::face_of(m.types[i], f);
      const surf::Face F = surf::face_points(face, P);
      uint32_t tri[6];
      const int nt = surf::face_triangles(F, m.points,
                                          m.points + 3 * size_t(P[surf::face_ref(face)]), tri);
      for (int t = 0; t < nt; ++t) {
        uint32_t bits = 0;
        for (int v = 0; v < 3; ++v)
          if (clip::kept(m.values[tri[3 * t + v]], m.isovalue, invert)) {
            bits |= 1u << v;
            vid[tri[3 * t + v]] = 0;
          }
        const int pieces = clip::piece_count(bits);
        np += uint64_t(pieces);
        for (int piece = 0; emit && piece < pieces; ++piece)
          for (int v = 0; v < 3; ++v) {
            int ci, cj;
            clip::piece_corner(bits, piece, v, &ci, &cj);
            corners.push_back(tri[3 * t + ci]);
            corners.push_back(tri[3 * t + cj]);
          }
      }
    }
  uint64_t nsv = 0;
  for (uint32_t& v : vid)
    if (v == 0) v = uint32_t(nsv++);
  const uint64_t nv = uint64_t(ncv) + nsv, nf = uint64_t(ncf) + np;
  out->nverts = nv;
  out->nfaces = nf;
  out->ncap_verts = ncv;
  out->ncap_faces = ncf;
  if (!emit) return SPRAY_RT_OK;
  out->verts.resize(3 * size_t(nv));
  if (with_normals) out->normals.resize(3 * size_t(nv));
  out->colors.resize(size_t(nv));
  out->pairs.resize(2 * size_t(nv));
  out->vt.resize(size_t(nv));
  out->faces.resize(3 * size_t(nf));
  // the cap: the isosurface's bytes, the pairs beside them, the swap
  if (const int r = spray_rt_cell_isosurface_host(
          &m, gc, &ncv, &ncf, out->verts.data(), with_normals ? out->normals.data() : nullptr,
          out->colors.data(), out->faces.data()))
    return r;
  for (size_t v = 0; v < ncv; ++v) {
    const uint32_t a = tet::key_a(ukeys[v], 32), b = tet::key_b(ukeys[v], 32);
    out->pairs[2 * v] = a;
    out->pairs[2 * v + 1] = b;
    out->vt[v] = tet::pair_t(m.values, a, b, m.isovalue);
  }
  for (size_t f = 0; invert && f < ncf; ++f) std::swap(out->faces[3 * f + 1], out->faces[3 * f + 2]);
  // the skin
  for (size_t p = 0; p < vid.size(); ++p) {
    if (vid[p] == UINT32_MAX) continue;
    const size_t v = ncv + vid[p];
    for (int ax = 0; ax < 3; ++ax) {
      out->verts[3 * v + size_t(ax)] = m.points[3 * p + size_t(ax)];
      if (with_normals) out->normals[3 * v + size_t(ax)] = pn[3 * p + size_t(ax)];
    }
    out->colors[v] = surf::point_color(cf, gc ? gc->table_rgb : nullptr, gc ? gc->lo : 0.0f,
                                       cscale, gc ? gc->ntable : 0, m.color_rgb, p);
    out->pairs[2 * v] = out->pairs[2 * v + 1] = uint32_t(p);
    out->vt[v] = 0.0f;
  }
  for (size_t k = 0; k < corners.size() / 2; ++k) {
    const uint32_t pi = corners[2 * k], pj = corners[2 * k + 1];
    uint32_t id;
    if (pi == pj) {
      id = uint32_t(ncv) + vid[pi];
    } else {
      const uint64_t key = tet::pair_key(std::min(pi, pj), std::max(pi, pj), 32);
      const uint32_t at = clip::find_key(ukeys.data(), uint32_t(ukeys.size()), key);
      if (at >= ukeys.size()) return SPRAY_RT_ERR_STATE;
      id = at;
    }
    out->faces[3 * ncf + k] = id;
  }
  return SPRAY_RT_OK;
}

// ---- the device clip: the cap's three reads, count, read 4, sort, unique,
// skin count, read 5, emit ----

using Clock = TetCall::Clock;
double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

std::string mesh_name(int i, const int* slots) {
  char buf[96];
  if (slots)
    snprintf(buf, sizeof(buf), "%s (mesh %d, slot %d)", kWhat, i, slots[i]);
  else
    snprintf(buf, sizeof(buf), "%s (mesh %d)", kWhat, i);
  return std::string(buf);
}

// A counted call: the welded cap, the skin's tables in the context's clip
// arena and what the host read of them.
struct ClipCall {
  TetCall tet;
  HeadTake<SurfJob> jobs;
  HeadTake<ClipJob> cjobs;
  HeadTake<uint32_t> status;
  HeadTake<ClipOut> outs;
  size_t m_outs = 0;  // the mark in front of outs
  uint32_t max_blocks = 0, max_pblocks = 0;
  bool staged = false;                        // some array came from host memory
  std::vector<uint64_t> ncv, ncf, nsv, nsf;   // cap and skin vertices and faces per mesh
};

// Everything up to the fifth host read.  want_normals[i]: the call reads mesh
// i's point_normals.  Messages name the mesh, and its slot where slots is given.
int clip_count(spray_rt_ctx* c, int n, const spray_rt_cellmesh* meshes, const int32_t* invert,
               const spray_rt_grid_color* gcolors, const int* slots,
               const std::vector<char>& want_normals, ClipCall* call) {
  const size_t nj = size_t(n);
  if (n > 65535)
    return fail(c, SPRAY_RT_ERR_LIMIT, "%s: more than 65535 meshes in one call", kWhat);
  std::vector<float> cscale(nj, 0.0f);
  for (int i = 0; i < n; ++i) {
    int code;
    if (const char* why = mesh_error(meshes[i], &code))
      return fail(c, code, "%s: %s", mesh_name(i, slots).c_str(), why);
    if (want_normals[size_t(i)] && !meshes[i].point_normals)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: normals asked of a mesh without point_normals",
                  mesh_name(i, slots).c_str());
    if (const char* why = gcolors ? tet_color_error(&gcolors[i], &cscale[size_t(i)]) : nullptr)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", mesh_name(i, slots).c_str(), why);
  }
  // ---- the cap: host reads 1 to 3 ----
  if (const int r = cell_weld(c, kWhat, n, meshes, gcolors, slots, want_normals, &call->tet))
    return r;
  const Clock::time_point t0 = call->tet.t0;
  const double cap_ms = ms_since(t0);
  c->clip_ms[0] = c->cell_ms;
  c->clip_ms[1] = c->tet_ms[0] - c->cell_ms;
  c->clip_ms[2] = c->tet_ms[1];
  c->clip_ms[3] = c->clip_ms[5] = 0.0;
  c->clip_ms[4] = c->tet_ms[3];
  call->ncv.resize(nj);
  call->ncf.resize(nj);
  for (size_t k = 0; k < nj; ++k) {
    call->ncv[k] = call->tet.rec[k].nverts;
    call->ncf[k] = call->tet.rec[k].nfaces;
  }
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then arrays and scratch ----
  JobArena& A = c->clip;
  A.reset();
  call->jobs = A.take_head<SurfJob>(nj);
  call->cjobs = A.take_head<ClipJob>(nj);
  const size_t m_views = A.mark();
  // TetJob views for tet_scan: [0, n) instances, [n, 2n) pieces, [2n, 3n) vertices
  const HeadTake<TetJob> t_views = A.take_head<TetJob>(3 * nj);
  const size_t m_status = A.mark();
  call->status = A.take_head<uint32_t>(nj);
  const HeadTake<uint32_t> t_offsets = A.take_head<uint32_t>(nj + 1);
  const size_t m_recs = A.mark();
  const HeadTake<TetRec> t_recs = A.take_head<TetRec>(3 * nj);
  call->m_outs = A.mark();
  call->outs = A.take_head<ClipOut>(nj);
  struct Scratch {
    Take<uint32_t> word, iblock, tblock, pword, pblock;
    uint32_t nblocks, npblocks;
  };
  std::vector<Scratch> sk(nj);
  // items 8 i ..: mesh i's arrays, host ones staged inside the arena
  enum { kPoints, kTypes, kOffsets, kConn, kValues, kNormals, kField, kTable, kItems };
  Stager stage;
  for (int i = 0; i < n; ++i) {
    const spray_rt_cellmesh& m = meshes[i];
    Scratch& k = sk[size_t(i)];
    // a mesh without cells reads nothing
    const size_t np = m.ncells ? m.npoints : 0;
    const spray_rt_grid_color* gc = gcolors && gcolors[i].field && np ? &gcolors[i] : nullptr;
    k.nblocks = uint32_t((m.ncells + surf::kSurfBlock - 1) / surf::kSurfBlock);
    k.npblocks = uint32_t((np + surf::kSurfBlock - 1) / surf::kSurfBlock);
    stage.place(m.points, 3 * np * sizeof(float), &A);
    stage.place(m.types, m.ncells * sizeof(uint8_t), &A);
    stage.place(m.offsets, m.ncells ? (m.ncells + 1) * sizeof(uint32_t) : 0, &A);
    stage.place(m.conn, m.ncells ? m.nconn * sizeof(uint32_t) : 0, &A);
    stage.place(m.values, np * sizeof(float), &A);
    stage.place(want_normals[size_t(i)] ? m.point_normals : nullptr, 3 * np * sizeof(float), &A);
    stage.place(gc ? gc->field : nullptr, np * sizeof(float), &A);
    stage.place(gc ? gc->table_rgb : nullptr, gc ? size_t(gc->ntable) * sizeof(uint32_t) : 0, &A);
    k.word = A.take<uint32_t>(m.ncells);
    k.iblock = A.take<uint32_t>(k.nblocks);
    k.tblock = A.take<uint32_t>(k.nblocks);
    k.pword = A.take<uint32_t>(np);
    k.pblock = A.take<uint32_t>(k.npblocks);
    call->max_blocks = std::max(call->max_blocks, k.nblocks);
    call->max_pblocks = std::max(call->max_pblocks, k.npblocks);
  }
  call->staged = stage.any || call->tet.staged;
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  SurfJob* jobs = A.host(call->jobs);
  ClipJob* cjobs = A.host(call->cjobs);
  TetJob* views = A.host(t_views);
  uint32_t* h_status = A.host(call->status);
  unsigned key_bits = 0;
  for (int i = 0; i < n; ++i) {
    const spray_rt_cellmesh& m = meshes[i];
    const Scratch& k = sk[size_t(i)];
    const size_t item = size_t(kItems) * size_t(i);
    SurfJob J{};
    J.points = stage.dev<float>(item + kPoints);
    J.types = stage.dev<uint8_t>(item + kTypes);
    J.offsets = stage.dev<uint32_t>(item + kOffsets);
    J.conn = stage.dev<uint32_t>(item + kConn);
    J.values = stage.dev<float>(item + kValues);
    J.normals = stage.dev<float>(item + kNormals);
    J.cfield = stage.dev<float>(item + kField);
    if (J.cfield) {
      J.ctable = stage.dev<uint32_t>(item + kTable);
      J.ntable = gcolors[i].ntable;
      J.clo = gcolors[i].lo;
      J.cscale = cscale[size_t(i)];
    }
    J.word = A.dev(k.word);
    J.iblock = A.dev(k.iblock);
    J.tblock = A.dev(k.tblock);
    J.pword = A.dev(k.pword);
    J.pblock = A.dev(k.pblock);
    J.npoints = m.npoints;
    J.nconn = m.nconn;
    J.ncells = uint32_t(m.ncells);
    J.nblocks = k.nblocks;
    J.npblocks = k.npblocks;
    J.mode = surf::kAll;
    J.color = m.color_rgb;
    J.shift = tet::index_bits(m.npoints);
    if (m.ncells) key_bits = std::max(key_bits, unsigned(surf::key_bits(J.shift)));
    jobs[i] = J;
    ClipJob K{};
    K.isovalue = m.isovalue;
    K.invert = invert && invert[i] ? 1u : 0u;
    cjobs[i] = K;
    for (int v = 0; v < 3; ++v) {
      TetJob V{};
      V.eblock = v == 0 ? J.iblock : v == 1 ? J.tblock : J.pblock;
      V.nblocks = v == 2 ? k.npblocks : k.nblocks;
      V.rec = A.dev(t_recs) + size_t(v) * nj + size_t(i);
      views[size_t(v) * nj + size_t(i)] = V;
    }
    h_status[i] = 0;
  }
  HIPCHK(c, arena_copy(A, 0, m_recs, true, s));
  const SurfJob* d_jobs = A.dev(call->jobs);
  const ClipJob* d_cjobs = A.dev(call->cjobs);
  const TetJob* d_views = A.dev(t_views);
  uint32_t* d_status = A.dev(call->status);
  HIPCHK(c, launch_clip_count(s, d_jobs, d_cjobs, n, call->max_blocks, call->max_pblocks,
                              d_status));
  HIPCHK(c, launch_tet_scan(s, d_views, nullptr, n, false));
  HIPCHK(c, arena_copy(A, m_status, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // status and instance totals: host read 4
  const TetRec* h_rec = A.host(t_recs);
  uint64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (const char* why = status_error(h_status[i]))
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", mesh_name(i, slots).c_str(), why);
    total += h_rec[i].ninst;
  }
  if (total >= kMaxInst)
    return fail(c, SPRAY_RT_ERR_LIMIT, "%s: 2^32 or more face instances in one call", kWhat);

  // ---- the instance scratch, sized by the totals ----
  bool timed = false;  // the sort ran between the context's two events
  if (total) {
    Layout M;  // of d_surfinst
    const auto t_keys = M.take<uint64_t>(size_t(total));
    const auto t_skeys = M.take<uint64_t>(size_t(total));
    const auto t_vals = M.take<uint32_t>(size_t(total));
    const auto t_svals = M.take<uint32_t>(size_t(total));
    const auto t_alive = M.take<uint8_t>(size_t(total));
    if (const int r = ensure(c, &c->d_surfinst, &c->surfinst_cap, std::max<size_t>(M.used, 256)))
      return r;
    void* base = c->d_surfinst;
    uint32_t* offsets = A.host(t_offsets);
    uint32_t first = 0, max_iblocks = 0;
    for (size_t k = 0; k < nj; ++k) {
      SurfJob& J = jobs[k];
      J.keys = t_keys.at(base) + first;
      J.skeys = t_skeys.at(base) + first;
      J.vals = t_vals.at(base) + first;
      J.svals = t_svals.at(base) + first;
      J.alive = t_alive.at(base) + first;
      J.ninst = uint32_t(h_rec[k].ninst);
      offsets[k] = first;
      first += J.ninst;
      const uint64_t iblocks = (uint64_t(J.ninst) + surf::kSurfBlock - 1) / surf::kSurfBlock;
      max_iblocks = std::max(max_iblocks, uint32_t(iblocks));
    }
    offsets[nj] = first;
    HIPCHK(c, arena_copy(A, 0, m_views, true, s));
    HIPCHK(c, arena_copy(A, m_status, m_recs, true, s));  // status (zero) and the offsets
    HIPCHK(c, launch_surf_keys(s, d_jobs, n, call->max_blocks));
    size_t tmp_bytes = 0;
    HIPCHK(c, tet_sort(s, nullptr, &tmp_bytes, t_keys.at(base), t_skeys.at(base), t_vals.at(base),
                       t_svals.at(base), first, n, A.dev(t_offsets), key_bits));
    if (const int r = ensure(c, &c->d_sort, &c->sort_cap, std::max<size_t>(tmp_bytes, 256)))
      return r;
    timed = c->tet_timing;
    for (hipEvent_t& e : c->tet_ev)
      if (timed && !e) HIPCHK(c, hipEventCreate(&e));
    if (timed) HIPCHK(c, hipEventRecord(c->tet_ev[0], s));
    HIPCHK(c, tet_sort(s, c->d_sort, &tmp_bytes, t_keys.at(base), t_skeys.at(base),
                       t_vals.at(base), t_svals.at(base), first, n, A.dev(t_offsets), key_bits));
    if (timed) HIPCHK(c, hipEventRecord(c->tet_ev[1], s));
    HIPCHK(c, launch_surf_unique(s, d_jobs, n, max_iblocks));
  }
  HIPCHK(c, launch_clip_skin_count(s, d_jobs, d_cjobs, c->tet.dev(call->tet.insts), n,
                                   call->max_blocks, call->max_pblocks, d_status));
  HIPCHK(c, launch_tet_scan(s, d_views + nj, nullptr, 2 * n, false));
  HIPCHK(c, arena_copy(A, m_status, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // lookup status, vertex and piece counts: host read 5
  c->clip_ms[5] = ms_since(t0) - cap_ms;
  if (timed) {
    float sort_ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&sort_ms, c->tet_ev[0], c->tet_ev[1]));
    c->clip_ms[4] += double(sort_ms);
  }
  for (int i = 0; i < n; ++i)
    if (h_status[i] & clip::kMiss)  // a guard no known input reaches: see clip_common.h
      return fail(c, SPRAY_RT_ERR_STATE, "%s: a cut edge of the skin has no cap vertex",
                  mesh_name(i, slots).c_str());
  call->nsv.resize(nj);
  call->nsf.resize(nj);
  for (size_t k = 0; k < nj; ++k) {
    call->nsf[k] = h_rec[nj + k].ninst;
    call->nsv[k] = h_rec[2 * nj + k].ninst;
  }
  return SPRAY_RT_OK;
}

// The cap's and the skin's vertex and face passes of a counted call into
// outs[n], whose ncap_* are the call's.
int clip_emit(spray_rt_ctx* c, int n, const ClipCall& call, const std::vector<ClipOut>& outs,
              const int32_t* invert) {
  const Clock::time_point t1 = Clock::now();
  hipStream_t s = stream_of(c);
  std::vector<TetOut> touts(size_t(n), TetOut{});
  uint64_t swap_faces = 0;
  for (size_t k = 0; k < size_t(n); ++k) {
    const ClipOut& O = outs[k];
    TetOut& T = touts[k];
    T.verts = O.verts;
    T.normals = O.normals;
    T.colors = O.colors;
    T.faces = O.faces;
    T.cap_verts = (O.verts || O.normals || O.colors) ? std::min(O.ncap_verts, O.cap_verts) : 0;
    T.cap_faces = O.faces ? std::min(O.ncap_faces, O.cap_faces) : 0;
    if (invert && invert[k] && O.faces) swap_faces = std::max(swap_faces, O.ncap_faces);
  }
  if (const int r = tet_emit(c, n, call.tet, touts)) return r;
  const JobArena& A = c->clip;
  std::memcpy(A.host(call.outs), outs.data(), size_t(n) * sizeof(ClipOut));
  HIPCHK(c, arena_copy(A, call.m_outs, call.m_outs + size_t(n) * sizeof(ClipOut), true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  const uint32_t max_fblocks = uint32_t((swap_faces + surf::kSurfBlock - 1) / surf::kSurfBlock);
  HIPCHK(c, launch_clip_emit(s, A.dev(call.jobs), A.dev(call.cjobs), c->tet.dev(call.tet.insts),
                             A.dev(call.outs), n, call.max_blocks, call.max_pblocks,
                             call.tet.max_iblocks, max_fblocks, A.dev(call.status)));
  c->clip_ms[3] = std::chrono::duration<double, std::milli>(Clock::now() - t1).count();
  return SPRAY_RT_OK;
}

}  // namespace

extern "C" {

int spray_rt_cell_clip_host(const spray_rt_cellmesh* mesh, int32_t invert,
                            const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                            size_t* ncap_verts, size_t* ncap_faces, float* verts_out,
                            float* vnormals_out, uint32_t* colors_out, uint32_t* vert_pairs_out,
                            float* vert_t_out, uint32_t* faces_out) {
  if (!mesh) return SPRAY_RT_ERR_ARG;
  for (size_t* p : {nverts, nfaces, ncap_verts, ncap_faces})
    if (p) *p = 0;
  HostClip m;
  const bool emit = verts_out || vnormals_out || colors_out || vert_pairs_out || vert_t_out ||
                    faces_out;
  const int r = clip_host(*mesh, invert ? 1u : 0u, gcolor, emit, vnormals_out != nullptr, &m);
  if (r) return r;
  if (nverts) *nverts = size_t(m.nverts);
  if (nfaces) *nfaces = size_t(m.nfaces);
  if (ncap_verts) *ncap_verts = size_t(m.ncap_verts);
  if (ncap_faces) *ncap_faces = size_t(m.ncap_faces);
  if (verts_out) std::memcpy(verts_out, m.verts.data(), m.verts.size() * sizeof(float));
  if (vnormals_out) std::memcpy(vnormals_out, m.normals.data(), m.normals.size() * sizeof(float));
  if (colors_out) std::memcpy(colors_out, m.colors.data(), m.colors.size() * sizeof(uint32_t));
  if (vert_pairs_out)
    std::memcpy(vert_pairs_out, m.pairs.data(), m.pairs.size() * sizeof(uint32_t));
  if (vert_t_out) std::memcpy(vert_t_out, m.vt.data(), m.vt.size() * sizeof(float));
  if (faces_out) std::memcpy(faces_out, m.faces.data(), m.faces.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_cell_clip_phase_times(spray_rt_ctx_t c, double out_ms[6]) {
  if (!c || !out_ms) return SPRAY_RT_ERR_ARG;
  for (int k = 0; k < 6; ++k) out_ms[k] = c->clip_ms[k];
  return SPRAY_RT_OK;
}

int spray_rt_cell_clip(spray_rt_ctx_t c, int n, const spray_rt_cellmesh* meshes,
                       const int32_t* invert, const spray_rt_grid_color* gcolors,
                       float* const* verts, float* const* vnormals, uint32_t* const* colors,
                       uint32_t* const* vert_pairs, float* const* vert_t, uint32_t* const* faces,
                       const size_t* cap_verts, const size_t* cap_faces, size_t* nverts_out,
                       size_t* nfaces_out, size_t* ncap_verts_out, size_t* ncap_faces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  const bool per_vertex_any = verts || vnormals || colors || vert_pairs || vert_t;
  if (n < 0 || (n && !meshes) || (n && per_vertex_any && !cap_verts) ||
      (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "%s: null arguments", kWhat);
  if (n == 0) return SPRAY_RT_OK;
  std::vector<char> want_normals(size_t(n), 0);
  for (int i = 0; vnormals && i < n; ++i) want_normals[size_t(i)] = vnormals[i] != nullptr;
  ClipCall call;
  int r = clip_count(c, n, meshes, invert, gcolors, nullptr, want_normals, &call);
  if (r) {
    (void)hipStreamSynchronize(stream_of(c));  // the pinned tables may still be on their way
    return r;
  }
  for (size_t k = 0; k < size_t(n); ++k) {
    if (nverts_out) nverts_out[k] = size_t(call.ncv[k] + call.nsv[k]);
    if (nfaces_out) nfaces_out[k] = size_t(call.ncf[k] + call.nsf[k]);
    if (ncap_verts_out) ncap_verts_out[k] = size_t(call.ncv[k]);
    if (ncap_faces_out) ncap_faces_out[k] = size_t(call.ncf[k]);
  }
  if (!per_vertex_any && !faces) return SPRAY_RT_OK;
  std::vector<ClipOut> outs(size_t(n), ClipOut{});
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const uint64_t nv = call.ncv[size_t(i)] + call.nsv[size_t(i)];
    const uint64_t nf = call.ncf[size_t(i)] + call.nsf[size_t(i)];
    ClipOut& O = outs[size_t(i)];
    O.verts = verts ? verts[i] : nullptr;
    O.normals = vnormals ? vnormals[i] : nullptr;
    O.colors = colors ? colors[i] : nullptr;
    O.pairs = vert_pairs ? vert_pairs[i] : nullptr;
    O.vt = vert_t ? vert_t[i] : nullptr;
    O.faces = faces ? faces[i] : nullptr;
    const bool per_vertex = O.verts || O.normals || O.colors || O.pairs || O.vt;
    if ((per_vertex && nv > cap_verts[i]) || (O.faces && nf > cap_faces[i]))
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "%s (mesh %d): %llu vertices and %llu faces do not fit the buffers", kWhat, i,
                  static_cast<unsigned long long>(nv), static_cast<unsigned long long>(nf));
    O.cap_verts = per_vertex ? nv : 0;
    O.cap_faces = O.faces ? nf : 0;
    O.ncap_verts = call.ncv[size_t(i)];
    O.ncap_faces = call.ncf[size_t(i)];
    any = any || per_vertex || O.faces;
  }
  if (!any) return SPRAY_RT_OK;
  r = clip_emit(c, n, call, outs, invert);
  if (r) return r;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  return SPRAY_RT_OK;
}

int spray_rt_domains_cell_clip(spray_rt_ctx_t c, int n, const int* slots,
                               const spray_rt_cellmesh* meshes, const int32_t* invert,
                               const spray_rt_grid_color* gcolors, int with_normals,
                               float* d_bounds, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!slots || !meshes)))
    return fail(c, SPRAY_RT_ERR_ARG, "%s: null arguments", kWhat);
  if (n == 0) return SPRAY_RT_OK;
  const size_t nj = size_t(n);
  if (const int r = tet_slots_error(c, kWhat, n, slots)) return r;
  std::vector<char> want_normals(nj, 0), want_colors(nj, 0);
  for (size_t k = 0; k < nj; ++k) {
    want_normals[k] = with_normals && meshes[k].point_normals;
    want_colors[k] = meshes[k].has_color || (gcolors && gcolors[k].field);
  }
  ClipCall call;
  int r = clip_count(c, n, meshes, invert, gcolors, slots, want_normals, &call);
  if (r) {
    (void)hipStreamSynchronize(stream_of(c));
    return r;
  }
  for (int i = 0; i < n; ++i)
    if (call.ncf[size_t(i)] + call.nsf[size_t(i)] >= kMaxFaces)
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: 2^29 or more faces", mesh_name(i, slots).c_str());

  // ---- the meshes: context scratch, at the exact sizes ----
  Layout M;  // of d_isomesh
  std::vector<ClipOut> outs(nj, ClipOut{});
  std::vector<Take<float>> t_verts(nj), t_normals(nj);
  std::vector<Take<uint32_t>> t_colors(nj), t_faces(nj);
  std::vector<size_t> nv(nj), nf(nj);
  for (size_t k = 0; k < nj; ++k) {
    outs[k].ncap_verts = call.ncv[k];
    outs[k].ncap_faces = call.ncf[k];
    outs[k].cap_verts = nv[k] = size_t(call.ncv[k] + call.nsv[k]);
    outs[k].cap_faces = nf[k] = size_t(call.ncf[k] + call.nsf[k]);
    t_verts[k] = M.take<float>(3 * nv[k]);
    if (want_normals[k]) t_normals[k] = M.take<float>(3 * nv[k]);
    if (want_colors[k]) t_colors[k] = M.take<uint32_t>(nv[k]);
    t_faces[k] = M.take<uint32_t>(3 * nf[k]);
  }
  r = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (r) return r;
  std::vector<const float*> pv(nj), pn(nj);
  std::vector<const uint32_t*> pc(nj), pf(nj);
  for (size_t k = 0; k < nj; ++k) {
    ClipOut& O = outs[k];
    pv[k] = O.verts = t_verts[k].at(c->d_isomesh);
    pn[k] = O.normals = t_normals[k] ? t_normals[k].at(c->d_isomesh) : nullptr;
    pc[k] = O.colors = t_colors[k] ? t_colors[k].at(c->d_isomesh) : nullptr;
    pf[k] = O.faces = t_faces[k].at(c->d_isomesh);
  }
  r = clip_emit(c, n, call, outs, invert);
  if (r) return r;

  // ---- the slots: the device build on the extracted arrays ----
  int job = -1;  // the build names the slot; name the mesh as well
  r = domains_build(c, n, slots, pv.data(), nv.data(), pf.data(), nf.data(), pc.data(), pn.data(),
                    d_bounds, &job);
  if (r) {
    const std::string msg = c->err;
    if (job >= 0)
      return fail(c, r, "%s (mesh %d, slot %d): %s", kWhat, job, slots[job], msg.c_str());
    return fail(c, r, "%s: %s", kWhat, msg.c_str());
  }
  if (nfaces_out)
    for (size_t k = 0; k < nj; ++k) nfaces_out[k] = nf[k];
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  return SPRAY_RT_OK;
}

int spray_rt_plane_values_host(const float* points, size_t npoints, const float origin[3],
                               const float normal[3], float* values_out) {
  if (!origin || !normal) return SPRAY_RT_ERR_ARG;
  for (int ax = 0; ax < 3; ++ax)
    if (!refit::finite_f(origin[ax]) || !refit::finite_f(normal[ax])) return SPRAY_RT_ERR_ARG;
  if (normal[0] == 0.0f && normal[1] == 0.0f && normal[2] == 0.0f) return SPRAY_RT_ERR_ARG;
  if (npoints && (!points || !values_out)) return SPRAY_RT_ERR_ARG;
  for (size_t p = 0; p < npoints; ++p)
    values_out[p] = clip::plane_value(points + 3 * p, origin, normal);
  return SPRAY_RT_OK;
}

int spray_rt_plane_values(spray_rt_ctx_t c, const float* points, size_t npoints,
                          const float origin[3], const float normal[3], float* values_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (!origin || !normal) return fail(c, SPRAY_RT_ERR_ARG, "plane values: null origin or normal");
  Plane plane;
  for (int ax = 0; ax < 3; ++ax) {
    if (!refit::finite_f(origin[ax]) || !refit::finite_f(normal[ax]))
      return fail(c, SPRAY_RT_ERR_ARG, "plane values: non-finite origin or normal");
    plane.origin[ax] = origin[ax];
    plane.normal[ax] = normal[ax];
  }
  if (normal[0] == 0.0f && normal[1] == 0.0f && normal[2] == 0.0f)
    return fail(c, SPRAY_RT_ERR_ARG, "plane values: zero normal");
  if (npoints && (!points || !values_out))
    return fail(c, SPRAY_RT_ERR_ARG, "plane values: null points or values");
  if (!npoints) return SPRAY_RT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);
  Stager stage;
  stage.place(points, 3 * npoints * sizeof(float));
  if (stage.any) {
    if (const int r = ensure(c, &c->d_stage, &c->stage_cap, stage.own.used)) return r;
    HIPCHK(c, stage.copy(c->d_stage, s));
  }
  HIPCHK(c, launch_plane_values(s, stage.dev<float>(0), npoints, plane, values_out));
  if (stage.any) HIPCHK(c, hipStreamSynchronize(s));  // the host array: done on return
  return SPRAY_RT_OK;
}

}  // extern "C"
