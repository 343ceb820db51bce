// cell_isosurface.cpp -- isosurfaces of unstructured meshes of hexahedra,
// wedges, pyramids and tets: spray_rt_cell_isosurface,
// spray_rt_domains_cell_isosurface and the host-only restatements
// (include/spray_rt.h).
//
// The cells are split into tets by cell_common.h's rule, and the surface is
// the tet extraction's of that list.  On the device (cell_kernels.hip) a count
// pass over the cells makes every check and finds the cells the surface
// crosses, the first host read brings status and the tet totals, a split pass
// writes the tets of the crossing cells alone, and tet_pipeline.h's count,
// weld and emit run on those device arrays: a cell that does not cross gives
// neither vertices nor faces, so leaving its tets out changes no output byte
// ("Isosurfaces of hexahedral, wedge and pyramid cells").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "cell_common.h"
#include "cell_kernels.h"
#include "rt_common.h"
#include "rt_ctx.h"
#include "spray_rt.h"
#include "tet_common.h"
#include "tet_kernels.h"
#include "tet_pipeline.h"

using namespace spray_rt;
using namespace spray_rt::detail;

namespace {

constexpr uint64_t kMaxCells = uint64_t(1) << 29;
constexpr uint64_t kMaxTets = uint64_t(1) << 29;
constexpr uint64_t kMaxConn = uint64_t(1) << 32;
constexpr uint64_t kMaxPoints = uint64_t(1) << 32;
constexpr const char* kWhat = "cell isosurface";

// What is wrong with the description of a mesh's cells (nullptr: nothing).
const char* list_error(const spray_rt_cellmesh& m, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (m.ncells && (!m.types || !m.offsets || !m.conn)) return "null types, offsets or conn";
  *code = SPRAY_RT_ERR_LIMIT;
  if (uint64_t(m.ncells) >= kMaxCells) return "2^29 or more cells";
  if (uint64_t(m.nconn) >= kMaxConn) return "2^32 or more listed point indices";
  if (uint64_t(m.npoints) >= kMaxPoints) return "2^32 or more points";
  *code = SPRAY_RT_OK;
  return nullptr;
}

// ... with the mesh as a whole.
const char* mesh_error(const spray_rt_cellmesh& m, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (m.ncells && (!m.points || !m.values)) return "null points or values";
  if (!refit::finite_f(m.isovalue)) return "non-finite isovalue";
  return list_error(m, code);
}

// What the status bits of a mesh say.
const char* status_error(uint32_t st) {
  if (st & cell::kBadType) return "unknown cell type";
  if (st & cell::kBadOffsets) return "offsets of a cell do not match its type's point count";
  if (st & cell::kBadConn) return "offsets of a cell beyond nconn";
  if (st & tet::kBadIndex) return "point index out of range";
  if (st & tet::kBadPoint) return "non-finite coordinate of a referenced point";
  if (st & tet::kBadSample) return "non-finite sample at a referenced point";
  if (st & tet::kBadColor) return "non-finite sample of the colour field at a referenced point";
  if (st & tet::kBadNormal) return "non-finite normal of a referenced point";
  return nullptr;
}

// The full tet list of the rule; tets nullptr: the count alone.
int split_host(const spray_rt_cellmesh& m, uint64_t* ntets, std::vector<uint32_t>* tets) {
  *ntets = 0;
  int code;
  if (list_error(m, &code)) return code;
  uint64_t nt = 0;
  for (size_t i = 0; i < m.ncells; ++i) {
    uint32_t type, o0;
    if (cell::check_cell(m.types, m.offsets, m.conn, m.npoints, m.nconn, i, &type, &o0))
      return SPRAY_RT_ERR_ARG;
    nt += uint64_t(cell::cell_tets(type));
  }
  *ntets = nt;
  if (!tets) return SPRAY_RT_OK;
  tets->resize(4 * size_t(nt));
  size_t at = 0;
  for (size_t i = 0; i < m.ncells; ++i) {
    const uint32_t type = m.types[i];
    cell::split(type, m.conn + m.offsets[i], tets->data() + 4 * at);
    at += size_t(cell::cell_tets(type));
  }
  return SPRAY_RT_OK;
}

double ms_since(TetCall::Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(TetCall::Clock::now() - t0).count();
}

std::string mesh_name(const char* what, int i, const int* slots) {
  char buf[96];
  if (slots)
    snprintf(buf, sizeof(buf), "%s (mesh %d, slot %d)", what, i, slots[i]);
  else
    snprintf(buf, sizeof(buf), "%s (mesh %d)", what, i);
  return std::string(buf);
}

// The tet meshes of the crossing cells, on the device, and their colour fields.
struct CellCall {
  std::vector<spray_rt_tetmesh> meshes;
  std::vector<spray_rt_grid_color> gcolors;  // empty: none
  bool staged = false;                       // some array came from host memory
};

// Validates the meshes and their colour maps, runs the count pass and the scan
// and reads status and tet totals (host read 1), then enqueues the split of
// the crossing cells.  want_normals[i]: the call reads mesh i's point_normals.
int cell_split(spray_rt_ctx* c, int n, const spray_rt_cellmesh* meshes,
               const spray_rt_grid_color* gcolors, const int* slots,
               const std::vector<char>& want_normals, const TetCall& call, CellCall* out) {
  const size_t nj = size_t(n);
  if (n > 65535)
    return fail(c, SPRAY_RT_ERR_LIMIT, "%s: more than 65535 meshes in one call", call.what);
  for (int i = 0; i < n; ++i) {
    int code;
    if (const char* why = mesh_error(meshes[i], &code))
      return fail(c, code, "%s: %s", mesh_name(call.what, i, slots).c_str(), why);
    if (want_normals[size_t(i)] && !meshes[i].point_normals)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: normals asked of a mesh without point_normals",
                  mesh_name(call.what, i, slots).c_str());
    float scale;
    if (const char* why = gcolors ? tet_color_error(&gcolors[i], &scale) : nullptr)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", mesh_name(call.what, i, slots).c_str(), why);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then arrays and scratch ----
  JobArena& A = c->cell;
  A.reset();
  const HeadTake<CellJob> t_jobs = A.take_head<CellJob>(nj);
  const size_t m_views = A.mark();
  const HeadTake<TetJob> t_views = A.take_head<TetJob>(nj);  // of the block sums, for tet_scan
  const size_t m_status = A.mark();
  const HeadTake<uint32_t> t_status = A.take_head<uint32_t>(nj);
  const HeadTake<TetRec> t_recs = A.take_head<TetRec>(nj);
  struct Scratch {
    Take<uint32_t> word, tblock;
    uint32_t nblocks;
  };
  std::vector<Scratch> sk(nj);
  // items 7 i ..: mesh i's arrays, host ones staged inside the arena
  enum { kPoints, kTypes, kOffsets, kConn, kValues, kNormals, kField, kItems };
  Stager stage;
  uint32_t max_blocks = 0;
  for (int i = 0; i < n; ++i) {
    const spray_rt_cellmesh& m = meshes[i];
    Scratch& k = sk[size_t(i)];
    // a mesh without cells reads nothing
    const size_t np = m.ncells ? m.npoints : 0;
    const bool mapped = gcolors && gcolors[i].field;
    k.nblocks = uint32_t((m.ncells + cell::kCellBlock - 1) / cell::kCellBlock);
    stage.place(m.points, 3 * np * sizeof(float), &A);
    stage.place(m.types, m.ncells * sizeof(uint8_t), &A);
    stage.place(m.offsets, m.ncells ? (m.ncells + 1) * sizeof(uint32_t) : 0, &A);
    stage.place(m.conn, m.ncells ? m.nconn * sizeof(uint32_t) : 0, &A);
    stage.place(m.values, np * sizeof(float), &A);
    stage.place(want_normals[size_t(i)] ? m.point_normals : nullptr, 3 * np * sizeof(float), &A);
    stage.place(mapped ? gcolors[i].field : nullptr, np * sizeof(float), &A);
    k.word = A.take<uint32_t>(m.ncells);
    k.tblock = A.take<uint32_t>(k.nblocks);
    max_blocks = std::max(max_blocks, k.nblocks);
  }
  out->staged = stage.any;
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  CellJob* jobs = A.host(t_jobs);
  TetJob* views = A.host(t_views);
  uint32_t* h_status = A.host(t_status);
  for (int i = 0; i < n; ++i) {
    const spray_rt_cellmesh& m = meshes[i];
    const Scratch& k = sk[size_t(i)];
    const size_t item = size_t(kItems) * size_t(i);
    CellJob J{};
    J.points = stage.dev<float>(item + kPoints);
    J.types = stage.dev<uint8_t>(item + kTypes);
    J.offsets = stage.dev<uint32_t>(item + kOffsets);
    J.conn = stage.dev<uint32_t>(item + kConn);
    J.values = stage.dev<float>(item + kValues);
    J.normals = stage.dev<float>(item + kNormals);
    J.cfield = stage.dev<float>(item + kField);
    J.word = A.dev(k.word);
    J.tblock = A.dev(k.tblock);
    J.npoints = m.npoints;
    J.nconn = m.nconn;
    J.ncells = uint32_t(m.ncells);
    J.nblocks = k.nblocks;
    J.isovalue = m.isovalue;
    jobs[i] = J;
    TetJob V{};
    V.eblock = J.tblock;
    V.nblocks = k.nblocks;
    V.rec = A.dev(t_recs) + i;
    views[i] = V;
    h_status[i] = 0;
  }
  HIPCHK(c, arena_copy(A, 0, A.head, true, s));
  const CellJob* d_jobs = A.dev(t_jobs);
  HIPCHK(c, launch_cell_count(s, d_jobs, n, max_blocks, A.dev(t_status)));
  HIPCHK(c, launch_tet_scan(s, A.dev(t_views), nullptr, n, false));
  HIPCHK(c, arena_copy(A, m_status, A.head, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // status and tet totals: host read 1
  c->cell_ms = ms_since(call.t0);
  const TetRec* h_rec = A.host(t_recs);
  for (int i = 0; i < n; ++i) {
    if (const char* why = status_error(h_status[i]))
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", mesh_name(call.what, i, slots).c_str(), why);
    if (h_rec[i].ninst >= kMaxTets)
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: 2^29 or more tets from crossing cells",
                  mesh_name(call.what, i, slots).c_str());
  }

  // ---- the tets of the crossing cells, sized by the totals ----
  Layout T;  // of d_celltets
  std::vector<Take<uint32_t>> t_tets(nj);
  for (size_t k = 0; k < nj; ++k) t_tets[k] = T.take<uint32_t>(4 * size_t(h_rec[k].ninst));
  if (const int r = ensure(c, &c->d_celltets, &c->celltets_cap, std::max<size_t>(T.used, 256)))
    return r;
  out->meshes.assign(nj, spray_rt_tetmesh{});
  if (gcolors) out->gcolors.assign(gcolors, gcolors + n);
  bool any = false;
  for (size_t k = 0; k < nj; ++k) {
    CellJob& J = jobs[k];
    J.tets = t_tets[k].at(c->d_celltets);
    J.ntets = uint32_t(h_rec[k].ninst);
    any = any || J.ntets;
    spray_rt_tetmesh& M = out->meshes[k];
    M.points = J.points;
    M.tets = J.tets;
    M.values = J.values;
    // a mesh without cells reads nothing: its own pointer stands for "has normals"
    M.point_normals = J.normals ? J.normals : (want_normals[k] ? meshes[k].point_normals : nullptr);
    M.npoints = meshes[k].npoints;
    M.ntets = J.ntets;
    M.isovalue = meshes[k].isovalue;
    M.color_rgb = meshes[k].color_rgb;
    M.has_color = meshes[k].has_color;
    if (gcolors) out->gcolors[k].field = J.cfield;
  }
  if (any) {
    HIPCHK(c, arena_copy(A, 0, m_views, true, s));
    HIPCHK(c, launch_cell_split(s, d_jobs, n, max_blocks));
  }
  return SPRAY_RT_OK;
}

}  // namespace

namespace spray_rt {
namespace detail {

// The tet pipeline's first two stages on the split meshes.  A failure waits
// for the stream: the pinned job table may still be on its way.
int cell_weld(spray_rt_ctx* c, const char* what, int n, const spray_rt_cellmesh* meshes,
              const spray_rt_grid_color* gcolors, const int* slots,
              const std::vector<char>& want_normals, TetCall* call) {
  CellCall cells;
  call->what = what;
  int r = cell_split(c, n, meshes, gcolors, slots, want_normals, *call, &cells);
  if (r) return r;
  r = tet_count(c, n, cells.meshes.data(), cells.gcolors.empty() ? nullptr : cells.gcolors.data(),
                slots, want_normals, call);
  if (!r) r = tet_weld(c, n, call);
  call->staged = call->staged || cells.staged;
  if (r) (void)hipStreamSynchronize(stream_of(c));
  return r;
}

}  // namespace detail
}  // namespace spray_rt

extern "C" {

int spray_rt_cell_split_host(const spray_rt_cellmesh* mesh, size_t* ntets, uint32_t* tets_out) {
  if (!mesh) return SPRAY_RT_ERR_ARG;
  uint64_t nt = 0;
  std::vector<uint32_t> tets;
  const int r = split_host(*mesh, &nt, tets_out ? &tets : nullptr);
  if (ntets) *ntets = size_t(nt);
  if (r) return r;
  if (tets_out) std::copy(tets.begin(), tets.end(), tets_out);
  return SPRAY_RT_OK;
}

int spray_rt_cell_isosurface_host(const spray_rt_cellmesh* mesh, const spray_rt_grid_color* gcolor,
                                  size_t* nverts, size_t* nfaces, float* verts_out,
                                  float* vnormals_out, uint32_t* colors_out, uint32_t* faces_out) {
  if (!mesh) return SPRAY_RT_ERR_ARG;
  if (nverts) *nverts = 0;
  if (nfaces) *nfaces = 0;
  int code;
  if (mesh_error(*mesh, &code)) return code;
  uint64_t nt = 0;
  std::vector<uint32_t> tets;
  if (const int r = split_host(*mesh, &nt, &tets)) return r;
  spray_rt_tetmesh M{};
  M.points = mesh->points;
  M.tets = tets.data();
  M.values = mesh->values;
  M.point_normals = mesh->point_normals;
  M.npoints = mesh->npoints;
  M.ntets = size_t(nt);
  M.isovalue = mesh->isovalue;
  M.color_rgb = mesh->color_rgb;
  M.has_color = mesh->has_color;
  return spray_rt_tet_isosurface_host(&M, gcolor, nverts, nfaces, verts_out, vnormals_out,
                                      colors_out, faces_out);
}

int spray_rt_cell_phase_times(spray_rt_ctx_t c, double out_ms[5]) {
  if (!c || !out_ms) return SPRAY_RT_ERR_ARG;
  out_ms[0] = c->cell_ms;
  out_ms[1] = c->tet_ms[0] - c->cell_ms;
  for (int k = 1; k < 4; ++k) out_ms[k + 1] = c->tet_ms[k];
  return SPRAY_RT_OK;
}

int spray_rt_cell_isosurface(spray_rt_ctx_t c, int n, const spray_rt_cellmesh* meshes,
                             const spray_rt_grid_color* gcolors, float* const* verts,
                             float* const* vnormals, uint32_t* const* colors,
                             uint32_t* const* faces, const size_t* cap_verts,
                             const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && !meshes) || (n && (verts || vnormals || colors) && !cap_verts) ||
      (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "%s: null arguments", kWhat);
  if (n == 0) return SPRAY_RT_OK;
  std::vector<char> want_normals(size_t(n), 0);
  for (int i = 0; vnormals && i < n; ++i) want_normals[size_t(i)] = vnormals[i] != nullptr;
  TetCall call;
  if (const int r = cell_weld(c, kWhat, n, meshes, gcolors, nullptr, want_normals, &call)) return r;
  return tet_to_buffers(c, n, call, verts, vnormals, colors, faces, cap_verts, cap_faces,
                        nverts_out, nfaces_out);
}

int spray_rt_domains_cell_isosurface(spray_rt_ctx_t c, int n, const int* slots,
                                     const spray_rt_cellmesh* meshes,
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
  TetCall call;
  if (const int r = cell_weld(c, kWhat, n, meshes, gcolors, slots, want_normals, &call)) return r;
  return tet_to_slots(c, n, slots, call, want_normals, want_colors, d_bounds, nfaces_out);
}

}  // extern "C"
