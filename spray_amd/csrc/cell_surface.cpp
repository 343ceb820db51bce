// cell_surface.cpp -- boundary surfaces and thresholds of unstructured meshes
// of hexahedra, wedges, pyramids and tets: spray_rt_cell_surface,
// spray_rt_domains_cell_surface and the host-only restatement
// (include/spray_rt.h).
//
// On the device (surf_kernels.hip) a count pass over the cells makes every
// check and applies the select, the first host read brings status and the
// face-instance totals, the keys of the kept cells' faces are sorted per mesh,
// the faces whose key occurs once survive and flag their points, the second
// host read brings the vertex and triangle counts, and the last two passes
// write into the caller's buffers or into context scratch, from where
// spray_rt_domains_build makes slots of the meshes.  Nothing is written to a
// slot or a caller buffer before every check has passed ("Boundary
// surfaces and thresholds of cell meshes").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "rt_common.h"
#include "rt_ctx.h"
#include "spray_rt.h"
#include "surf_common.h"
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
constexpr const char* kWhat = "cell surface";
static_assert(surf::kAll == SPRAY_RT_SELECT_ALL && surf::kPoints == SPRAY_RT_SELECT_POINTS &&
                  surf::kCells == SPRAY_RT_SELECT_CELLS,
              "surf_common.h's modes are the header's");

const spray_rt_cell_select kSelectAll{nullptr, 0.0f, 0.0f, SPRAY_RT_SELECT_ALL};

// What is wrong with a mesh's description and its select (nullptr: nothing).
const char* mesh_error(const spray_rt_cellmesh& m, const spray_rt_cell_select& sel, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (sel.mode != SPRAY_RT_SELECT_ALL && sel.mode != SPRAY_RT_SELECT_POINTS &&
      sel.mode != SPRAY_RT_SELECT_CELLS)
    return "unknown select mode";
  if (sel.mode != SPRAY_RT_SELECT_ALL &&
      (!refit::finite_f(sel.lo) || !refit::finite_f(sel.hi) || sel.lo > sel.hi))
    return "the select's bounds are not lo <= hi, both finite";
  if (m.ncells && (!m.types || !m.offsets || !m.conn)) return "null types, offsets or conn";
  if (m.ncells && !m.points) return "null points";
  if (m.ncells && sel.mode == SPRAY_RT_SELECT_POINTS && !m.values)
    return "null values in mode POINTS";
  if (m.ncells && sel.mode == SPRAY_RT_SELECT_CELLS && !sel.cell_values)
    return "null cell_values in mode CELLS";
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
  if (st & surf::kBadCellValue) return "non-finite cell value";
  if (st & tet::kBadColor) return "non-finite sample of the colour field at a referenced point";
  if (st & tet::kBadNormal) return "non-finite normal of a referenced point";
  return nullptr;
}

struct HostMesh {
  std::vector<float> verts, normals;
  std::vector<uint32_t> faces, colors, ids;
  uint64_t nverts = 0, nfaces = 0;
};

// The extraction on the host: the kernels' passes, one after the other.
int extract_host(const spray_rt_cellmesh& m, const spray_rt_cell_select& sel,
                 const spray_rt_grid_color* gc, bool emit, bool with_normals, HostMesh* out) {
  int code;
  if (mesh_error(m, sel, &code)) return code;
  float cscale;
  if (tet_color_error(gc, &cscale)) return SPRAY_RT_ERR_ARG;
  if (with_normals && !m.point_normals) return SPRAY_RT_ERR_ARG;
  const float* cf = gc ? gc->field : nullptr;
  const float* pn = with_normals ? m.point_normals : nullptr;
  const size_t nc = m.ncells;
  const int w = tet::index_bits(m.npoints);
  // count: every check, the kept cells and the first instance of each
  std::vector<uint8_t> nfaces(nc);
  std::vector<uint64_t> first(nc);
  uint64_t ninst = 0;
  for (size_t i = 0; i < nc; ++i) {
    const surf::Cell C =
        surf::classify(m.points, m.types, m.offsets, m.conn, m.values, sel.cell_values, cf, pn,
                       m.npoints, m.nconn, i, sel.mode, sel.lo, sel.hi);
    if (C.status) return SPRAY_RT_ERR_ARG;
    nfaces[i] = uint8_t(C.nfaces);
    first[i] = ninst;
    ninst += C.nfaces;
  }
  if (ninst >= kMaxInst) return SPRAY_RT_ERR_LIMIT;
  // keys, the sort, the keys that occur once
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
  // the points the surviving faces use, and the triangle count
  std::vector<uint32_t> vid(nc ? m.npoints : 0, UINT32_MAX);
  uint64_t nf = 0;
  for (size_t i = 0; i < nc; ++i)
    for (int f = 0; f < int(nfaces[i]); ++f) {
      if (!alive[size_t(first[i]) + size_t(f)]) continue;
      const uint32_t face = surf::face_of(m.types[i], f);
      const int n = surf::face_corners(face);
      for (int d = 0; d < n; ++d) vid[m.conn[m.offsets[i] + uint32_t(cell::face_q(face, d))]] = 0;
      nf += uint64_t(n - 2);
    }
  uint64_t nv = 0;
  for (uint32_t& v : vid)
    if (v == 0) v = uint32_t(nv++);
  out->nverts = nv;
  out->nfaces = nf;
  if (!emit) return SPRAY_RT_OK;
  out->verts.resize(3 * size_t(nv));
  if (with_normals) out->normals.resize(3 * size_t(nv));
  out->colors.resize(size_t(nv));
  out->ids.resize(size_t(nv));
  out->faces.resize(3 * size_t(nf));
  for (size_t p = 0; p < vid.size(); ++p) {
    if (vid[p] == UINT32_MAX) continue;
    const size_t v = vid[p];
    for (int ax = 0; ax < 3; ++ax) {
      out->verts[3 * v + size_t(ax)] = m.points[3 * p + size_t(ax)];
      if (with_normals) out->normals[3 * v + size_t(ax)] = pn[3 * p + size_t(ax)];
    }
    out->colors[v] = surf::point_color(cf, gc ? gc->table_rgb : nullptr, gc ? gc->lo : 0.0f,
                                       cscale, gc ? gc->ntable : 0, m.color_rgb, p);
    out->ids[v] = uint32_t(p);
  }
  size_t fid = 0;
  for (size_t i = 0; i < nc; ++i)
    for (int f = 0; f < int(nfaces[i]); ++f) {
      if (!alive[size_t(first[i]) + size_t(f)]) continue;
      const uint32_t* P = m.conn + m.offsets[i];
      const uint32_t face = surf::face_of(m.types[i], f);
      const surf::Face F = surf::face_points(face, P);
      uint32_t tri[6];
      const int nt = surf::face_triangles(F, m.points,
                                          m.points + 3 * size_t(P[surf::face_ref(face)]), tri);
      for (int k = 0; k < 3 * nt; ++k) out->faces[3 * fid + size_t(k)] = vid[tri[k]];
      fid += size_t(nt);
    }
  return SPRAY_RT_OK;
}

// ---- the device extraction: count, read 1, sort, unique, read 2, emit ----

using Clock = std::chrono::steady_clock;
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

// A counted call: the tables in the context's surf arena and what the host
// read of them.
struct SurfCall {
  HeadTake<SurfJob> jobs;
  HeadTake<SurfOut> outs;
  size_t m_outs = 0;  // the mark in front of outs
  uint32_t max_blocks = 0, max_pblocks = 0;
  bool staged = false;            // some array came from host memory
  std::vector<uint64_t> nv, nf;   // vertices and triangles per mesh
  Clock::time_point t0 = Clock::now();
};

// Everything up to the second host read.  want_normals[i]: the call reads mesh
// i's point_normals.  Messages name the mesh, and its slot where slots is given.
int surf_count(spray_rt_ctx* c, int n, const spray_rt_cellmesh* meshes,
               const spray_rt_cell_select* selects, const spray_rt_grid_color* gcolors,
               const int* slots, const std::vector<char>& want_normals, SurfCall* call) {
  const size_t nj = size_t(n);
  if (n > 65535)
    return fail(c, SPRAY_RT_ERR_LIMIT, "%s: more than 65535 meshes in one call", kWhat);
  std::vector<float> cscale(nj, 0.0f);
  for (int i = 0; i < n; ++i) {
    int code;
    if (const char* why = mesh_error(meshes[i], selects ? selects[i] : kSelectAll, &code))
      return fail(c, code, "%s: %s", mesh_name(i, slots).c_str(), why);
    if (want_normals[size_t(i)] && !meshes[i].point_normals)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: normals asked of a mesh without point_normals",
                  mesh_name(i, slots).c_str());
    if (const char* why = gcolors ? tet_color_error(&gcolors[i], &cscale[size_t(i)]) : nullptr)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", mesh_name(i, slots).c_str(), why);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then arrays and scratch ----
  JobArena& A = c->surf;
  A.reset();
  call->jobs = A.take_head<SurfJob>(nj);
  const size_t m_views = A.mark();
  // TetJob views for tet_scan: [0, n) instances, [n, 2n) triangles, [2n, 3n) vertices
  const HeadTake<TetJob> t_views = A.take_head<TetJob>(3 * nj);
  const size_t m_status = A.mark();
  const HeadTake<uint32_t> t_status = A.take_head<uint32_t>(nj);
  const HeadTake<uint32_t> t_offsets = A.take_head<uint32_t>(nj + 1);
  const size_t m_recs = A.mark();
  const HeadTake<TetRec> t_recs = A.take_head<TetRec>(3 * nj);
  call->m_outs = A.mark();
  call->outs = A.take_head<SurfOut>(nj);
  struct Scratch {
    Take<uint32_t> word, iblock, tblock, pword, pblock;
    uint32_t nblocks, npblocks;
  };
  std::vector<Scratch> sk(nj);
  // items 9 i ..: mesh i's arrays, host ones staged inside the arena
  enum { kPoints, kTypes, kOffsets, kConn, kValues, kCellValues, kNormals, kField, kTable, kItems };
  Stager stage;
  for (int i = 0; i < n; ++i) {
    const spray_rt_cellmesh& m = meshes[i];
    const spray_rt_cell_select& sel = selects ? selects[i] : kSelectAll;
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
    stage.place(sel.mode == SPRAY_RT_SELECT_POINTS ? m.values : nullptr, np * sizeof(float), &A);
    stage.place(sel.mode == SPRAY_RT_SELECT_CELLS ? sel.cell_values : nullptr,
                m.ncells * sizeof(float), &A);
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
  call->staged = stage.any;
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  SurfJob* jobs = A.host(call->jobs);
  TetJob* views = A.host(t_views);
  uint32_t* h_status = A.host(t_status);
  unsigned key_bits = 0;
  for (int i = 0; i < n; ++i) {
    const spray_rt_cellmesh& m = meshes[i];
    const spray_rt_cell_select& sel = selects ? selects[i] : kSelectAll;
    const Scratch& k = sk[size_t(i)];
    const size_t item = size_t(kItems) * size_t(i);
    SurfJob J{};
    J.points = stage.dev<float>(item + kPoints);
    J.types = stage.dev<uint8_t>(item + kTypes);
    J.offsets = stage.dev<uint32_t>(item + kOffsets);
    J.conn = stage.dev<uint32_t>(item + kConn);
    J.values = stage.dev<float>(item + kValues);
    J.cell_values = stage.dev<float>(item + kCellValues);
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
    J.mode = sel.mode;
    J.lo = sel.lo;
    J.hi = sel.hi;
    J.color = m.color_rgb;
    J.shift = tet::index_bits(m.npoints);
    if (m.ncells) key_bits = std::max(key_bits, unsigned(surf::key_bits(J.shift)));
    jobs[i] = J;
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
  const TetJob* d_views = A.dev(t_views);
  HIPCHK(c, launch_surf_count(s, d_jobs, n, call->max_blocks, call->max_pblocks,
                              A.dev(t_status)));
  HIPCHK(c, launch_tet_scan(s, d_views, nullptr, n, false));
  HIPCHK(c, arena_copy(A, m_status, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // status and instance totals: host read 1
  c->surf_ms[0] = ms_since(call->t0);
  c->surf_ms[1] = c->surf_ms[2] = c->surf_ms[3] = 0.0;
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
  HIPCHK(c, launch_surf_tri_count(s, d_jobs, n, call->max_blocks, call->max_pblocks));
  HIPCHK(c, launch_tet_scan(s, d_views + nj, nullptr, 2 * n, false));
  HIPCHK(c, arena_copy(A, m_recs, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the vertex and triangle counts: host read 2
  c->surf_ms[1] = ms_since(call->t0) - c->surf_ms[0];
  if (timed) {
    float sort_ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&sort_ms, c->tet_ev[0], c->tet_ev[1]));
    c->surf_ms[3] = double(sort_ms);
  }
  call->nv.resize(nj);
  call->nf.resize(nj);
  for (size_t k = 0; k < nj; ++k) {
    call->nf[k] = h_rec[nj + k].ninst;
    call->nv[k] = h_rec[2 * nj + k].ninst;
  }
  return SPRAY_RT_OK;
}

// The vertex and face passes of a counted call into outs[n].
int surf_emit(spray_rt_ctx* c, int n, const SurfCall& call, const std::vector<SurfOut>& outs) {
  hipStream_t s = stream_of(c);
  const JobArena& A = c->surf;
  std::memcpy(A.host(call.outs), outs.data(), size_t(n) * sizeof(SurfOut));
  HIPCHK(c, arena_copy(A, call.m_outs, call.m_outs + size_t(n) * sizeof(SurfOut), true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  HIPCHK(c, launch_surf_emit(s, A.dev(call.jobs), A.dev(call.outs), n, call.max_blocks,
                             call.max_pblocks));
  c->surf_ms[2] = ms_since(call.t0) - c->surf_ms[0] - c->surf_ms[1];
  return SPRAY_RT_OK;
}

}  // namespace

extern "C" {

int spray_rt_cell_surface_host(const spray_rt_cellmesh* mesh, const spray_rt_cell_select* select,
                               const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                               float* verts_out, float* vnormals_out, uint32_t* colors_out,
                               uint32_t* point_ids_out, uint32_t* faces_out) {
  if (!mesh) return SPRAY_RT_ERR_ARG;
  if (nverts) *nverts = 0;
  if (nfaces) *nfaces = 0;
  HostMesh m;
  const bool emit = verts_out || vnormals_out || colors_out || point_ids_out || faces_out;
  const int r = extract_host(*mesh, select ? *select : kSelectAll, gcolor, emit,
                             vnormals_out != nullptr, &m);
  if (r) return r;
  if (nverts) *nverts = size_t(m.nverts);
  if (nfaces) *nfaces = size_t(m.nfaces);
  if (verts_out) std::memcpy(verts_out, m.verts.data(), m.verts.size() * sizeof(float));
  if (vnormals_out) std::memcpy(vnormals_out, m.normals.data(), m.normals.size() * sizeof(float));
  if (colors_out) std::memcpy(colors_out, m.colors.data(), m.colors.size() * sizeof(uint32_t));
  if (point_ids_out) std::memcpy(point_ids_out, m.ids.data(), m.ids.size() * sizeof(uint32_t));
  if (faces_out) std::memcpy(faces_out, m.faces.data(), m.faces.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_cell_surface_phase_times(spray_rt_ctx_t c, double out_ms[4]) {
  if (!c || !out_ms) return SPRAY_RT_ERR_ARG;
  for (int k = 0; k < 4; ++k) out_ms[k] = c->surf_ms[k];
  return SPRAY_RT_OK;
}

int spray_rt_cell_surface(spray_rt_ctx_t c, int n, const spray_rt_cellmesh* meshes,
                          const spray_rt_cell_select* selects, const spray_rt_grid_color* gcolors,
                          float* const* verts, float* const* vnormals, uint32_t* const* colors,
                          uint32_t* const* point_ids, uint32_t* const* faces,
                          const size_t* cap_verts, const size_t* cap_faces, size_t* nverts_out,
                          size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && !meshes) || (n && (verts || vnormals || colors || point_ids) && !cap_verts) ||
      (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "%s: null arguments", kWhat);
  if (n == 0) return SPRAY_RT_OK;
  std::vector<char> want_normals(size_t(n), 0);
  for (int i = 0; vnormals && i < n; ++i) want_normals[size_t(i)] = vnormals[i] != nullptr;
  SurfCall call;
  int r = surf_count(c, n, meshes, selects, gcolors, nullptr, want_normals, &call);
  if (r) {
    (void)hipStreamSynchronize(stream_of(c));  // the pinned tables may still be on their way
    return r;
  }
  for (int i = 0; i < n; ++i) {
    if (nverts_out) nverts_out[i] = size_t(call.nv[size_t(i)]);
    if (nfaces_out) nfaces_out[i] = size_t(call.nf[size_t(i)]);
  }
  if (!verts && !vnormals && !colors && !point_ids && !faces) return SPRAY_RT_OK;
  std::vector<SurfOut> outs(size_t(n), SurfOut{});
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const uint64_t nv = call.nv[size_t(i)], nf = call.nf[size_t(i)];
    SurfOut& O = outs[size_t(i)];
    O.verts = verts ? verts[i] : nullptr;
    O.normals = vnormals ? vnormals[i] : nullptr;
    O.colors = colors ? colors[i] : nullptr;
    O.ids = point_ids ? point_ids[i] : nullptr;
    O.faces = faces ? faces[i] : nullptr;
    const bool per_vertex = O.verts || O.normals || O.colors || O.ids;
    if ((per_vertex && nv > cap_verts[i]) || (O.faces && nf > cap_faces[i]))
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "%s (mesh %d): %llu vertices and %llu faces do not fit the buffers", kWhat, i,
                  static_cast<unsigned long long>(nv), static_cast<unsigned long long>(nf));
    O.cap_verts = per_vertex ? nv : 0;
    O.cap_faces = O.faces ? nf : 0;
    any = any || per_vertex || O.faces;
  }
  if (!any) return SPRAY_RT_OK;
  r = surf_emit(c, n, call, outs);
  if (r) return r;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  return SPRAY_RT_OK;
}

int spray_rt_domains_cell_surface(spray_rt_ctx_t c, int n, const int* slots,
                                  const spray_rt_cellmesh* meshes,
                                  const spray_rt_cell_select* selects,
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
  SurfCall call;
  int r = surf_count(c, n, meshes, selects, gcolors, slots, want_normals, &call);
  if (r) {
    (void)hipStreamSynchronize(stream_of(c));
    return r;
  }
  for (int i = 0; i < n; ++i)
    if (call.nf[size_t(i)] >= kMaxFaces)
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: 2^29 or more faces", mesh_name(i, slots).c_str());

  // ---- the meshes: context scratch, at the exact sizes ----
  Layout M;  // of d_isomesh
  std::vector<SurfOut> outs(nj, SurfOut{});
  std::vector<Take<float>> t_verts(nj), t_normals(nj);
  std::vector<Take<uint32_t>> t_colors(nj), t_faces(nj);
  std::vector<size_t> nv(nj), nf(nj);
  for (size_t k = 0; k < nj; ++k) {
    outs[k].cap_verts = nv[k] = size_t(call.nv[k]);
    outs[k].cap_faces = nf[k] = size_t(call.nf[k]);
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
    SurfOut& O = outs[k];
    pv[k] = O.verts = t_verts[k].at(c->d_isomesh);
    pn[k] = O.normals = t_normals[k] ? t_normals[k].at(c->d_isomesh) : nullptr;
    pc[k] = O.colors = t_colors[k] ? t_colors[k].at(c->d_isomesh) : nullptr;
    pf[k] = O.faces = t_faces[k].at(c->d_isomesh);
  }
  r = surf_emit(c, n, call, outs);
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

}  // extern "C"
