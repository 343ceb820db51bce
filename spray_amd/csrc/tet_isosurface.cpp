// tet_isosurface.cpp -- isosurfaces of unstructured tetrahedral meshes:
// spray_rt_tet_isosurface, spray_rt_domains_tet_isosurface and the host-only
// restatement (include/spray_rt.h).
//
// The extraction runs on the device (tet_kernels.hip) on meshes that may
// already be in HBM: a count pass over the tets, the first host read (status
// and instance / face totals), keys, a segmented sort and a run count over the
// crossing-edge instances, the second host read (the vertex counts), then the
// vertex and face passes into the caller's buffers or into context scratch,
// from where spray_rt_domains_build makes slots of the meshes.  Nothing is
// written to a slot or a caller buffer before every check has passed
// ("Isosurfaces of tetrahedral meshes").
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
#include "tet_common.h"
#include "tet_kernels.h"
#include "tet_pipeline.h"

using namespace spray_rt;
using namespace spray_rt::detail;

namespace {

constexpr uint64_t kMaxTets = uint64_t(1) << 29;
constexpr uint64_t kMaxPoints = uint64_t(1) << 32;
constexpr uint64_t kMaxInst = uint64_t(1) << 32;

// What is wrong with a mesh's description (nullptr: nothing); *code = the error.
const char* mesh_error(const spray_rt_tetmesh& m, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (m.ntets && !m.tets) return "null tets";
  if (m.ntets && (!m.points || !m.values)) return "null points or values";
  if (!refit::finite_f(m.isovalue)) return "non-finite isovalue";
  *code = SPRAY_RT_ERR_LIMIT;
  if (uint64_t(m.ntets) >= kMaxTets) return "2^29 or more tets";
  if (uint64_t(m.npoints) >= kMaxPoints) return "2^32 or more points";
  *code = SPRAY_RT_OK;
  return nullptr;
}

// What the status bits of a mesh say.
const char* status_error(uint32_t st) {
  if (st & tet::kBadIndex) return "point index out of range";
  if (st & tet::kBadPoint) return "non-finite coordinate of a referenced point";
  if (st & tet::kBadSample) return "non-finite sample at a referenced point";
  if (st & tet::kBadColor) return "non-finite sample of the colour field at a referenced point";
  if (st & tet::kBadNormal) return "non-finite normal of a referenced point";
  return nullptr;
}

struct HostMesh {
  std::vector<float> verts, normals;
  std::vector<uint32_t> faces, colors;
  uint64_t nverts = 0, nfaces = 0;
};

// The extraction on the host: the kernels' passes, one after the other.
int extract_host(const spray_rt_tetmesh& m, const spray_rt_grid_color* gc, bool emit,
                 bool with_normals, bool with_colors, HostMesh* out) {
  int code;
  if (mesh_error(m, &code)) return code;
  float cscale;
  if (tet_color_error(gc, &cscale)) return SPRAY_RT_ERR_ARG;
  if (with_normals && !m.point_normals) return SPRAY_RT_ERR_ARG;
  const float* cf = gc ? gc->field : nullptr;
  const float* pn = with_normals ? m.point_normals : nullptr;
  const size_t nt = m.ntets;
  // count: inside bits, parity and first instance of every tet, the totals
  std::vector<uint8_t> signs(nt), odd(nt);
  std::vector<uint64_t> efirst(nt);
  uint64_t ninst = 0, nf = 0;
  for (size_t t = 0; t < nt; ++t) {
    const tet::Corner C =
        tet::classify(m.points, m.tets, m.values, cf, pn, m.npoints, t, m.isovalue);
    if (C.status) return SPRAY_RT_ERR_ARG;
    signs[t] = uint8_t(C.signs);
    odd[t] = uint8_t(C.odd);
    efirst[t] = ninst;
    ninst += uint64_t(iso::popc(tet::cross_mask(C.signs)));
    nf += uint64_t(iso::tet_tri_count(C.signs));
  }
  if (ninst >= kMaxInst) return SPRAY_RT_ERR_LIMIT;
  // keys, the sort, one vertex per run
  std::vector<std::pair<uint64_t, uint32_t>> inst;
  inst.reserve(size_t(ninst));
  for (size_t t = 0; t < nt; ++t) {
    const uint32_t mask = tet::cross_mask(signs[t]);
    for (int k = 0; k < 6; ++k) {
      if (!((mask >> k) & 1u)) continue;
      const uint32_t pu = m.tets[4 * t + size_t(tet::edge_u(k))];
      const uint32_t pw = m.tets[4 * t + size_t(tet::edge_w(k))];
      inst.emplace_back(tet::pair_key(std::min(pu, pw), std::max(pu, pw), 32),
                        uint32_t(inst.size()));
    }
  }
  std::sort(inst.begin(), inst.end());
  std::vector<uint32_t> vid(inst.size());
  std::vector<uint64_t> ukeys;
  for (size_t i = 0; i < inst.size(); ++i) {
    if (i == 0 || inst[i].first != inst[i - 1].first) ukeys.push_back(inst[i].first);
    vid[inst[i].second] = uint32_t(ukeys.size() - 1);
  }
  const uint64_t nv = ukeys.size();
  out->nverts = nv;
  out->nfaces = nf;
  if (!emit) return SPRAY_RT_OK;
  out->verts.resize(3 * size_t(nv));
  if (with_normals) out->normals.resize(3 * size_t(nv));
  if (with_colors) out->colors.resize(size_t(nv));
  out->faces.resize(3 * size_t(nf));
  for (size_t v = 0; v < size_t(nv); ++v) {
    const uint32_t a = tet::key_a(ukeys[v], 32), b = tet::key_b(ukeys[v], 32);
    const float t = tet::pair_t(m.values, a, b, m.isovalue);
    tet::pair_lerp3(m.points, a, b, t, &out->verts[3 * v]);
    if (with_normals) tet::pair_lerp3(pn, a, b, t, &out->normals[3 * v]);
    if (with_colors)
      out->colors[v] = cf ? gc->table_rgb[cmap::bin(iso::lerp(cf[a], cf[b], t), gc->lo, cscale,
                                                    gc->ntable)]
                          : m.color_rgb;
  }
  size_t fid = 0;
  for (size_t t = 0; t < nt; ++t) {
    uint8_t e[2][3];
    const int ntri = iso::tet_triangles(signs[t], odd[t], e);
    const uint32_t mask = tet::cross_mask(signs[t]);
    for (int n = 0; n < ntri; ++n, ++fid)
      for (int v = 0; v < 3; ++v) {
        const int k = tet::edge_index(e[n][v]);
        out->faces[3 * fid + size_t(v)] =
            vid[size_t(efirst[t]) + size_t(iso::popc(mask & ((1u << k) - 1u)))];
      }
  }
  return SPRAY_RT_OK;
}

// ---- the device extraction: count, read 1, weld, read 2, emit ----

using Clock = TetCall::Clock;
double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

std::string mesh_name(const char* what, int i, const int* slots) {
  char buf[96];
  if (slots)
    snprintf(buf, sizeof(buf), "%s (mesh %d, slot %d)", what, i, slots[i]);
  else
    snprintf(buf, sizeof(buf), "%s (mesh %d)", what, i);
  return std::string(buf);
}

}  // namespace

namespace spray_rt {
namespace detail {

const char* tet_color_error(const spray_rt_grid_color* gc, float* scale) {
  *scale = 0.0f;
  if (!gc || !gc->field) return nullptr;
  if (!gc->table_rgb) return "null colour table";
  if (!cmap::map_scale(gc->ntable, gc->lo, gc->hi, scale))
    return "the colour map is not a table of 1 to 4096 entries over lo < hi, both finite, with a "
           "finite normal scale";
  return nullptr;
}

// Validates the meshes (and their colour maps, gcolors nullptr: none), runs the
// count pass and its scan and reads status and totals: host read 1.
// want_normals[i]: the call reads mesh i's point_normals.  Messages name the
// mesh, and its slot where slots is given.
int tet_count(spray_rt_ctx* c, int n, const spray_rt_tetmesh* meshes,
              const spray_rt_grid_color* gcolors, const int* slots,
              const std::vector<char>& want_normals, TetCall* call) {
  const size_t nj = size_t(n);
  if (n > 65535)
    return fail(c, SPRAY_RT_ERR_LIMIT, "%s: more than 65535 meshes in one call", call->what);
  for (int i = 0; i < n; ++i) {
    int code;
    if (const char* why = mesh_error(meshes[i], &code))
      return fail(c, code, "%s: %s", mesh_name(call->what, i, slots).c_str(), why);
    if (want_normals[size_t(i)] && !meshes[i].point_normals)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: normals asked of a mesh without point_normals",
                  mesh_name(call->what, i, slots).c_str());
  }
  std::vector<float> cscale(nj, 0.0f);
  for (int i = 0; gcolors && i < n; ++i)
    if (const char* why = tet_color_error(&gcolors[i], &cscale[size_t(i)]))
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", mesh_name(call->what, i, slots).c_str(), why);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then arrays and scratch ----
  JobArena& A = c->tet;
  A.reset();
  call->jobs = A.take_head<TetJob>(nj);
  call->m_status = A.mark();
  call->status = A.take_head<uint32_t>(nj);
  call->m_rec = A.mark();
  call->recs = A.take_head<TetRec>(nj);
  call->m_insts = A.mark();
  call->insts = A.take_head<TetInst>(nj);
  call->offsets = A.take_head<uint32_t>(nj + 1);
  call->m_outs = A.mark();
  call->outs = A.take_head<TetOut>(nj);
  struct Scratch {
    Take<uint32_t> word, eblock, fblock;
    uint32_t nblocks;
  };
  std::vector<Scratch> sk(nj);
  // items 6 i ..: mesh i's points, tets, values, normals, colour field and
  // colour table, host ones staged inside the arena; a table several meshes
  // share is staged once
  enum { kPoints, kTets, kValues, kNormals, kField, kTable, kItems };
  Stager stage;
  std::vector<size_t> table_item(nj, 0);
  for (int i = 0; i < n; ++i) {
    const spray_rt_tetmesh& m = meshes[i];
    Scratch& k = sk[size_t(i)];
    // a mesh without tets reads nothing
    const size_t np = m.ntets ? m.npoints : 0;
    k.nblocks = uint32_t((m.ntets + tet::kTetBlock - 1) / tet::kTetBlock);
    stage.place(m.points, 3 * np * sizeof(float), &A);
    stage.place(m.tets, 4 * m.ntets * sizeof(uint32_t), &A);
    stage.place(m.values, np * sizeof(float), &A);
    stage.place(want_normals[size_t(i)] ? m.point_normals : nullptr, 3 * np * sizeof(float), &A);
    const spray_rt_grid_color* gc = gcolors && gcolors[i].field && np ? &gcolors[i] : nullptr;
    stage.place(gc ? gc->field : nullptr, np * sizeof(float), &A);
    table_item[size_t(i)] = size_t(kItems) * size_t(i) + kTable;
    for (int b = 0; gc && b < i; ++b)
      if (gcolors[b].field && meshes[b].ntets && gcolors[b].table_rgb == gc->table_rgb &&
          gcolors[b].ntable == gc->ntable) {
        table_item[size_t(i)] = table_item[size_t(b)];
        gc = nullptr;  // an empty item
      }
    stage.place(gc ? gc->table_rgb : nullptr, gc ? size_t(gc->ntable) * sizeof(uint32_t) : 0, &A);
    k.word = A.take<uint32_t>(m.ntets);
    k.eblock = A.take<uint32_t>(k.nblocks);
    k.fblock = A.take<uint32_t>(k.nblocks);
    call->max_blocks = std::max(call->max_blocks, k.nblocks);
  }
  call->staged = stage.any;
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  TetJob* jobs = A.host(call->jobs);
  uint32_t* h_status = A.host(call->status);
  for (int i = 0; i < n; ++i) {
    const spray_rt_tetmesh& m = meshes[i];
    const Scratch& k = sk[size_t(i)];
    const size_t item = size_t(kItems) * size_t(i);
    TetJob J{};
    J.points = stage.dev<float>(item + kPoints);
    J.tets = stage.dev<uint32_t>(item + kTets);
    J.values = stage.dev<float>(item + kValues);
    J.normals = stage.dev<float>(item + kNormals);
    J.cfield = stage.dev<float>(item + kField);
    if (J.cfield) {
      J.ctable = stage.dev<uint32_t>(table_item[size_t(i)]);
      J.ntable = gcolors[i].ntable;
      J.clo = gcolors[i].lo;
      J.cscale = cscale[size_t(i)];
    }
    J.word = A.dev(k.word);
    J.eblock = A.dev(k.eblock);
    J.fblock = A.dev(k.fblock);
    J.rec = A.dev(call->recs) + i;
    J.npoints = m.npoints;
    J.ntets = uint32_t(m.ntets);
    J.nblocks = k.nblocks;
    J.isovalue = m.isovalue;
    J.color = m.color_rgb;
    J.shift = tet::index_bits(m.npoints);
    if (m.ntets) call->key_bits = std::max(call->key_bits, 2u * unsigned(J.shift));
    jobs[i] = J;
    h_status[i] = 0;
  }
  HIPCHK(c, arena_copy(A, 0, call->m_rec, true, s));
  const TetJob* d_jobs = A.dev(call->jobs);
  HIPCHK(c, launch_tet_count(s, d_jobs, n, call->max_blocks, A.dev(call->status)));
  HIPCHK(c, launch_tet_scan(s, d_jobs, nullptr, n, false));
  HIPCHK(c, arena_copy(A, call->m_status, call->m_insts, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // status and totals: host read 1
  c->tet_ms[0] = ms_since(call->t0);
  c->tet_ms[1] = c->tet_ms[2] = c->tet_ms[3] = 0.0;
  const TetRec* h_rec = A.host(call->recs);
  call->rec.assign(h_rec, h_rec + n);
  uint64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (const char* why = status_error(h_status[i]))
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", mesh_name(call->what, i, slots).c_str(), why);
    total += h_rec[i].ninst;
  }
  if (total >= kMaxInst)
    return fail(c, SPRAY_RT_ERR_LIMIT, "%s: 2^32 or more crossing-edge instances in one call",
                call->what);
  return SPRAY_RT_OK;
}

// Keys, the sort and the run count of a counted call, then the vertex counts:
// host read 2.
int tet_weld(spray_rt_ctx* c, int n, TetCall* call) {
  const size_t nj = size_t(n);
  hipStream_t s = stream_of(c);
  JobArena& A = c->tet;
  // ---- the instance scratch, sized by the totals ----
  uint64_t total = 0;
  for (const TetRec& r : call->rec) total += r.ninst;
  Layout M;  // of d_tetinst
  const auto t_keys = M.take<uint64_t>(size_t(total));
  const auto t_skeys = M.take<uint64_t>(size_t(total));
  const auto t_inst = M.take<uint32_t>(size_t(total));
  const auto t_sinst = M.take<uint32_t>(size_t(total));
  const auto t_loc = M.take<uint32_t>(size_t(total));
  const auto t_vid = M.take<uint32_t>(size_t(total));
  std::vector<Take<uint32_t>> t_ublock(nj);
  std::vector<uint32_t> niblocks(nj);
  for (size_t k = 0; k < nj; ++k) {
    niblocks[k] = uint32_t((call->rec[k].ninst + tet::kTetBlock - 1) / tet::kTetBlock);
    t_ublock[k] = M.take<uint32_t>(niblocks[k]);
    call->max_iblocks = std::max(call->max_iblocks, niblocks[k]);
  }
  if (const int r = ensure(c, &c->d_tetinst, &c->tetinst_cap, std::max<size_t>(M.used, 256)))
    return r;
  void* base = c->d_tetinst;
  TetInst* insts = A.host(call->insts);
  uint32_t* offsets = A.host(call->offsets);
  uint32_t first = 0;
  bool timed = false;  // the sort ran between the context's two events
  for (size_t k = 0; k < nj; ++k) {
    TetInst I{};
    I.keys = t_keys.at(base) + first;
    I.skeys = t_skeys.at(base) + first;
    I.inst = t_inst.at(base) + first;
    I.sinst = t_sinst.at(base) + first;
    I.loc = t_loc.at(base) + first;
    I.vid = t_vid.at(base) + first;
    I.ublock = t_ublock[k].at(base);
    I.ninst = uint32_t(call->rec[k].ninst);
    I.niblocks = niblocks[k];
    insts[k] = I;
    offsets[k] = first;
    first += I.ninst;
  }
  offsets[nj] = first;
  HIPCHK(c, arena_copy(A, call->m_insts, call->m_outs, true, s));
  const TetJob* d_jobs = A.dev(call->jobs);
  const TetInst* d_insts = A.dev(call->insts);
  if (first) {
    HIPCHK(c, launch_tet_keys(s, d_jobs, d_insts, n, call->max_blocks));
    size_t tmp_bytes = 0;
    HIPCHK(c, tet_sort(s, nullptr, &tmp_bytes, t_keys.at(base), t_skeys.at(base), t_inst.at(base),
                       t_sinst.at(base), first, n, A.dev(call->offsets), call->key_bits));
    if (const int r = ensure(c, &c->d_sort, &c->sort_cap, std::max<size_t>(tmp_bytes, 256)))
      return r;
    timed = c->tet_timing;
    for (hipEvent_t& e : c->tet_ev)
      if (timed && !e) HIPCHK(c, hipEventCreate(&e));
    if (timed) HIPCHK(c, hipEventRecord(c->tet_ev[0], s));
    HIPCHK(c, tet_sort(s, c->d_sort, &tmp_bytes, t_keys.at(base), t_skeys.at(base),
                       t_inst.at(base), t_sinst.at(base), first, n, A.dev(call->offsets),
                       call->key_bits));
    if (timed) HIPCHK(c, hipEventRecord(c->tet_ev[1], s));
    HIPCHK(c, launch_tet_unique(s, d_insts, n, call->max_iblocks));
  }
  HIPCHK(c, launch_tet_scan(s, d_jobs, d_insts, n, true));
  HIPCHK(c, arena_copy(A, call->m_rec, call->m_insts, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the vertex counts: host read 2
  c->tet_ms[1] = ms_since(call->t0) - c->tet_ms[0];
  if (timed) {
    float sort_ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&sort_ms, c->tet_ev[0], c->tet_ev[1]));
    c->tet_ms[3] = double(sort_ms);
  }
  const TetRec* h_rec = A.host(call->recs);
  call->rec.assign(h_rec, h_rec + n);
  return SPRAY_RT_OK;
}

// The vertex and face passes of a welded call into outs[n].
int tet_emit(spray_rt_ctx* c, int n, const TetCall& call, const std::vector<TetOut>& outs) {
  hipStream_t s = stream_of(c);
  const JobArena& A = c->tet;
  std::memcpy(A.host(call.outs), outs.data(), size_t(n) * sizeof(TetOut));
  HIPCHK(c, arena_copy(A, call.m_outs, call.m_outs + size_t(n) * sizeof(TetOut), true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  // the vertex pass numbers the instances for the faces: it runs for either
  HIPCHK(c, launch_tet_verts(s, A.dev(call.jobs), A.dev(call.insts), A.dev(call.outs), n,
                             call.max_iblocks));
  HIPCHK(c, launch_tet_faces(s, A.dev(call.jobs), A.dev(call.insts), A.dev(call.outs), n,
                             call.max_blocks));
  c->tet_ms[2] = ms_since(call.t0) - c->tet_ms[0] - c->tet_ms[1];
  return SPRAY_RT_OK;
}

int tet_to_buffers(spray_rt_ctx* c, int n, const TetCall& call, float* const* verts,
                   float* const* vnormals, uint32_t* const* colors, uint32_t* const* faces,
                   const size_t* cap_verts, const size_t* cap_faces, size_t* nverts_out,
                   size_t* nfaces_out) {
  for (int i = 0; i < n; ++i) {
    if (nverts_out) nverts_out[i] = size_t(call.rec[size_t(i)].nverts);
    if (nfaces_out) nfaces_out[i] = size_t(call.rec[size_t(i)].nfaces);
  }
  if (!verts && !vnormals && !colors && !faces) return SPRAY_RT_OK;
  std::vector<TetOut> outs(size_t(n), TetOut{});
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const TetRec& rec = call.rec[size_t(i)];
    TetOut& O = outs[size_t(i)];
    O.verts = verts ? verts[i] : nullptr;
    O.normals = vnormals ? vnormals[i] : nullptr;
    O.colors = colors ? colors[i] : nullptr;
    O.faces = faces ? faces[i] : nullptr;
    const bool per_vertex = O.verts || O.normals || O.colors;
    if ((per_vertex && rec.nverts > cap_verts[i]) || (O.faces && rec.nfaces > cap_faces[i]))
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "%s (mesh %d): %llu vertices and %llu faces do not fit the buffers", call.what,
                  i, static_cast<unsigned long long>(rec.nverts),
                  static_cast<unsigned long long>(rec.nfaces));
    O.cap_verts = per_vertex ? rec.nverts : 0;
    O.cap_faces = O.faces ? rec.nfaces : 0;
    any = any || per_vertex || O.faces;
  }
  if (!any) return SPRAY_RT_OK;
  const int r = tet_emit(c, n, call, outs);
  if (r) return r;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  return SPRAY_RT_OK;
}

int tet_slots_error(spray_rt_ctx* c, const char* what, int n, const int* slots) {
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] > 1 << 20)
      return fail(c, SPRAY_RT_ERR_ARG, "%s (mesh %d): bad slot %d", what, i, slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail(c, SPRAY_RT_ERR_ARG, "%s (mesh %d): slot %d listed twice", what, i, slots[i]);
  }
  return SPRAY_RT_OK;
}

int tet_to_slots(spray_rt_ctx* c, int n, const int* slots, const TetCall& call,
                 const std::vector<char>& want_normals, const std::vector<char>& want_colors,
                 float* d_bounds, size_t* nfaces_out) {
  const size_t nj = size_t(n);
  for (int i = 0; i < n; ++i)
    if (call.rec[size_t(i)].nfaces >= kMaxTets)
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: 2^29 or more faces",
                  mesh_name(call.what, i, slots).c_str());

  // ---- the meshes: context scratch, at the exact sizes ----
  Layout M;  // of d_isomesh
  std::vector<TetOut> outs(nj, TetOut{});
  std::vector<Take<float>> t_verts(nj), t_normals(nj);
  std::vector<Take<uint32_t>> t_colors(nj), t_faces(nj);
  std::vector<size_t> nv(nj), nf(nj);
  for (size_t k = 0; k < nj; ++k) {
    outs[k].cap_verts = nv[k] = size_t(call.rec[k].nverts);
    outs[k].cap_faces = nf[k] = size_t(call.rec[k].nfaces);
    t_verts[k] = M.take<float>(3 * nv[k]);
    if (want_normals[k]) t_normals[k] = M.take<float>(3 * nv[k]);
    if (want_colors[k]) t_colors[k] = M.take<uint32_t>(nv[k]);
    t_faces[k] = M.take<uint32_t>(3 * nf[k]);
  }
  int r = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (r) return r;
  std::vector<const float*> pv(nj), pn(nj);
  std::vector<const uint32_t*> pc(nj), pf(nj);
  for (size_t k = 0; k < nj; ++k) {
    TetOut& O = outs[k];
    pv[k] = O.verts = t_verts[k].at(c->d_isomesh);
    pn[k] = O.normals = t_normals[k] ? t_normals[k].at(c->d_isomesh) : nullptr;
    pc[k] = O.colors = t_colors[k] ? t_colors[k].at(c->d_isomesh) : nullptr;
    pf[k] = O.faces = t_faces[k].at(c->d_isomesh);
  }
  r = tet_emit(c, n, call, outs);
  if (r) return r;

  // ---- the slots: the device build on the extracted arrays ----
  int job = -1;  // the build names the slot; name the mesh as well
  r = domains_build(c, n, slots, pv.data(), nv.data(), pf.data(), nf.data(), pc.data(), pn.data(),
                    d_bounds, &job);
  if (r) {
    const std::string msg = c->err;
    if (job >= 0)
      return fail(c, r, "%s (mesh %d, slot %d): %s", call.what, job, slots[job], msg.c_str());
    return fail(c, r, "%s: %s", call.what, msg.c_str());
  }
  if (nfaces_out)
    for (size_t k = 0; k < nj; ++k) nfaces_out[k] = nf[k];
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  return SPRAY_RT_OK;
}

}  // namespace detail
}  // namespace spray_rt

extern "C" {

int spray_rt_tet_isosurface_host(const spray_rt_tetmesh* mesh, const spray_rt_grid_color* gcolor,
                                 size_t* nverts, size_t* nfaces, float* verts_out,
                                 float* vnormals_out, uint32_t* colors_out, uint32_t* faces_out) {
  if (!mesh) return SPRAY_RT_ERR_ARG;
  HostMesh m;
  const bool emit = verts_out || vnormals_out || colors_out || faces_out;
  const int r = extract_host(*mesh, gcolor, emit, vnormals_out != nullptr, colors_out != nullptr, &m);
  if (nverts) *nverts = size_t(m.nverts);
  if (nfaces) *nfaces = size_t(m.nfaces);
  if (r) return r;
  if (verts_out) std::memcpy(verts_out, m.verts.data(), m.verts.size() * sizeof(float));
  if (vnormals_out) std::memcpy(vnormals_out, m.normals.data(), m.normals.size() * sizeof(float));
  if (colors_out) std::memcpy(colors_out, m.colors.data(), m.colors.size() * sizeof(uint32_t));
  if (faces_out) std::memcpy(faces_out, m.faces.data(), m.faces.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_tet_set_timing(spray_rt_ctx_t c, int on) {
  if (!c) return SPRAY_RT_ERR_ARG;
  c->tet_timing = on != 0;
  return SPRAY_RT_OK;
}

int spray_rt_tet_phase_times(spray_rt_ctx_t c, double out_ms[4]) {
  if (!c || !out_ms) return SPRAY_RT_ERR_ARG;
  for (int k = 0; k < 4; ++k) out_ms[k] = c->tet_ms[k];
  return SPRAY_RT_OK;
}

int spray_rt_tet_isosurface(spray_rt_ctx_t c, int n, const spray_rt_tetmesh* meshes,
                            const spray_rt_grid_color* gcolors, float* const* verts,
                            float* const* vnormals, uint32_t* const* colors,
                            uint32_t* const* faces, const size_t* cap_verts,
                            const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && !meshes) || (n && (verts || vnormals || colors) && !cap_verts) ||
      (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "tet isosurface: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  std::vector<char> want_normals(size_t(n), 0);
  for (int i = 0; vnormals && i < n; ++i) want_normals[size_t(i)] = vnormals[i] != nullptr;
  TetCall call;
  int r = tet_count(c, n, meshes, gcolors, nullptr, want_normals, &call);
  if (r) return r;
  r = tet_weld(c, n, &call);
  if (r) return r;
  return tet_to_buffers(c, n, call, verts, vnormals, colors, faces, cap_verts, cap_faces,
                        nverts_out, nfaces_out);
}

int spray_rt_domains_tet_isosurface(spray_rt_ctx_t c, int n, const int* slots,
                                    const spray_rt_tetmesh* meshes,
                                    const spray_rt_grid_color* gcolors, int with_normals,
                                    float* d_bounds, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!slots || !meshes)))
    return fail(c, SPRAY_RT_ERR_ARG, "tet isosurface: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const size_t nj = size_t(n);
  if (const int r = tet_slots_error(c, "tet isosurface", n, slots)) return r;
  std::vector<char> want_normals(nj, 0), want_colors(nj, 0);
  for (size_t k = 0; k < nj; ++k) {
    want_normals[k] = with_normals && meshes[k].point_normals;
    want_colors[k] = meshes[k].has_color || (gcolors && gcolors[k].field);
  }
  TetCall call;
  int r = tet_count(c, n, meshes, gcolors, slots, want_normals, &call);
  if (r) return r;
  r = tet_weld(c, n, &call);
  if (r) return r;
  return tet_to_slots(c, n, slots, call, want_normals, want_colors, d_bounds, nfaces_out);
}

}  // extern "C"
