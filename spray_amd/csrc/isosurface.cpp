// isosurface.cpp -- isosurfaces of scalar grids: spray_rt_isosurface,
// spray_rt_domains_isosurface, their forms coloured by a second field through
// a colour map (_mapped), the map over per-vertex data
// (spray_rt_colormap_apply), new colours for resident slots
// (spray_rt_domains_recolor) and the host-only restatements (include/spray_rt.h).
//
// The extraction runs on the device (iso_kernels.hip) on fields that may
// already be in HBM: a count pass, the call's one host read (the sizes), an
// emit pass into the caller's buffers or into context scratch, from where
// spray_rt_domains_build makes slots of the meshes.  Nothing is written to a
// slot or a caller buffer before every check has passed (DESIGN.md,
// "Isosurfaces").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "color_common.h"
#include "iso_common.h"
#include "iso_kernels.h"
#include "rt_common.h"
#include "rt_ctx.h"
#include "spray_rt.h"

using namespace spray_rt;
using namespace spray_rt::detail;

namespace {

constexpr uint64_t kMaxPoints = uint64_t(1) << 31;
constexpr uint64_t kMaxFaces = uint64_t(1) << 29;

// What is wrong with a grid's description (nullptr: nothing); *code = the error.
const char* grid_error(const spray_rt_grid& g, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (!g.values) return "null values";
  for (int a = 0; a < 3; ++a) {
    if (g.dims[a] < 2) return "fewer than 2 points on an axis";
    if (!(g.spacing[a] > 0.0f) || !refit::finite_f(g.spacing[a]))
      return "spacing is not positive and finite";
    if (!refit::finite_f(g.origin[a])) return "non-finite origin";
  }
  if (!refit::finite_f(g.isovalue)) return "non-finite isovalue";
  *code = SPRAY_RT_ERR_LIMIT;
  if (uint64_t(g.dims[0]) * uint64_t(g.dims[1]) * uint64_t(g.dims[2]) >= kMaxPoints)
    return "2^31 or more points";
  *code = SPRAY_RT_OK;
  return nullptr;
}

// What is wrong with (table, ntable, lo, hi) as a colour map (nullptr:
// nothing); *scale = the map's.
const char* map_error(const uint32_t* table, int ntable, float lo, float hi, float* scale) {
  *scale = 0.0f;
  if (!table) return "null colour table";
  if (ntable < 1 || ntable > cmap::kMaxTable)
    return "colour table of fewer than 1 or more than 4096 entries";
  if (!refit::finite_f(lo) || !refit::finite_f(hi) || !(lo < hi))
    return "colour range is not lo < hi, both finite";
  if (!cmap::map_scale(ntable, lo, hi, scale))
    return "colour scale ntable / (hi - lo) is not a finite normal float";
  return nullptr;
}

// ... with a grid's colour map; a grid without a colour field has none.
const char* color_error(const spray_rt_grid_color* gc, float* scale) {
  *scale = 0.0f;
  if (!gc || !gc->field) return nullptr;
  return map_error(gc->table_rgb, gc->ntable, gc->lo, gc->hi, scale);
}

// The samples of the cell whose minimum corner is (i, j, k).
void load_cell(const spray_rt_grid& g, int i, int j, int k, uint32_t valid, float f[8]) {
  const size_t nx = size_t(g.dims[0]), ny = size_t(g.dims[1]);
  const size_t p = size_t(i) + nx * (size_t(j) + ny * size_t(k));
  for (int c = 0; c < 8; ++c) {
    f[c] = 0.0f;
    if ((valid >> c) & 1u)
      f[c] = g.values[p + size_t(c & 1) + nx * (size_t((c >> 1) & 1) + ny * size_t(c >> 2))];
  }
}

struct HostMesh {
  std::vector<float> verts, normals;
  std::vector<uint32_t> faces, colors;
  uint64_t nverts = 0, nfaces = 0;
};

// The extraction on the host, step for step what the kernels do.  gc: the
// grid's colour map (nullptr or no field: the grid's constant colour).
int extract_host(const spray_rt_grid& g, const spray_rt_grid_color* gc, bool emit,
                 bool with_normals, bool with_colors, HostMesh* out) {
  int code;
  if (grid_error(g, &code)) return code;
  float cscale;
  if (color_error(gc, &cscale)) return SPRAY_RT_ERR_ARG;
  const float* cf = gc ? gc->field : nullptr;
  const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  const size_t np = size_t(nx) * size_t(ny) * size_t(nz);
  // count: crossing mask and first vertex of every point, the totals
  std::vector<uint8_t> emask(np);
  std::vector<uint64_t> vfirst(np);
  uint64_t nv = 0, nf = 0;
  size_t p = 0;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i, ++p) {
        const uint32_t valid = iso::valid_corners(i, j, k, nx, ny, nz);
        float f[8];
        load_cell(g, i, j, k, valid, f);
        if (!refit::finite_f(f[0])) return SPRAY_RT_ERR_ARG;
        if (cf && !refit::finite_f(cf[p])) return SPRAY_RT_ERR_ARG;
        const uint32_t ins = iso::inside_mask(f, valid, g.isovalue);
        emask[p] = uint8_t(iso::edge_mask(ins, valid));
        vfirst[p] = nv;
        nv += uint64_t(iso::popc(emask[p]));
        if (valid == 0xFFu) nf += iso::cell_tri_count(ins);
      }
  out->nverts = nv;
  out->nfaces = nf;
  if (nf >= kMaxFaces || nv > UINT32_MAX) return SPRAY_RT_ERR_LIMIT;
  if (!emit) return SPRAY_RT_OK;
  out->verts.resize(3 * size_t(nv));
  if (with_normals) out->normals.resize(3 * size_t(nv));
  if (with_colors) out->colors.resize(size_t(nv));
  out->faces.resize(3 * size_t(nf));
  size_t fid = 0;
  p = 0;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i, ++p) {
        const uint32_t valid = iso::valid_corners(i, j, k, nx, ny, nz);
        if (!emask[p] && valid != 0xFFu) continue;
        float f[8];
        load_cell(g, i, j, k, valid, f);
        if (emask[p]) {
          size_t vid = size_t(vfirst[p]);
          float ga[3] = {0.f, 0.f, 0.f};
          if (with_normals) iso::neg_gradient(g.values, nx, ny, nz, i, j, k, g.spacing, ga);
          for (int type = 0; type < 7; ++type) {
            if (!((emask[p] >> type) & 1u)) continue;
            const int c = iso::type_corner(type);
            const float t = iso::edge_t(f[0], f[c], g.isovalue);
            iso::edge_vertex(g.origin, g.spacing, i, j, k, type, t, &out->verts[3 * vid]);
            if (with_normals) {
              float gb[3];
              iso::neg_gradient(g.values, nx, ny, nz, i + (c & 1), j + ((c >> 1) & 1),
                                k + (c >> 2), g.spacing, gb);
              for (int ax = 0; ax < 3; ++ax)
                out->normals[3 * vid + size_t(ax)] = iso::lerp(ga[ax], gb[ax], t);
            }
            if (with_colors) {
              uint32_t col = g.color_rgb;
              if (cf) {
                const size_t q = p + size_t(c & 1) +
                                 size_t(nx) * (size_t((c >> 1) & 1) + size_t(ny) * size_t(c >> 2));
                col = gc->table_rgb[cmap::bin(iso::lerp(cf[p], cf[q], t), gc->lo, cscale,
                                              gc->ntable)];
              }
              out->colors[vid] = col;
            }
            ++vid;
          }
        }
        if (valid != 0xFFu) continue;
        const uint32_t ins = iso::inside_mask(f, valid, g.isovalue);
        if (ins == 0 || ins == 0xFFu) continue;
        for (int tet = 0; tet < 6; ++tet) {
          int T[4];
          iso::tet_corners(tet, T);
          uint8_t e[2][3];
          const int nt = iso::tet_triangles(iso::tet_signs(T, ins), iso::tet_odd(tet), e);
          for (int n = 0; n < nt; ++n, ++fid)
            for (int v = 0; v < 3; ++v) {
              const int cu = T[e[n][v] >> 2], cv = T[e[n][v] & 3];
              const size_t q = p + size_t(cu & 1) +
                               size_t(nx) * (size_t((cu >> 1) & 1) + size_t(ny) * size_t(cu >> 2));
              const int type = iso::diff_type(cu ^ cv);
              out->faces[3 * fid + size_t(v)] =
                  uint32_t(vfirst[q]) + uint32_t(iso::popc(emask[q] & ((1u << type) - 1u)));
            }
        }
      }
  return SPRAY_RT_OK;
}

// ---- the device extraction: count, the host read, emit ----

struct IsoCall {
  HeadTake<IsoJob> jobs;  // in the context's iso arena
  HeadTake<IsoOut> outs;
  size_t m_outs = 0;  // the mark in front of outs
  uint32_t max_blocks = 0;
  bool staged = false;  // some field came from host memory
  std::vector<IsoRec> rec;
};

// Validates the grids (and their colour maps, gcolors nullptr: none), runs the
// count pass and the scan and reads the sizes (the host read).  Messages name
// the grid, and its slot where slots is given.
int iso_count(spray_rt_ctx* c, int n, const spray_rt_grid* grids,
              const spray_rt_grid_color* gcolors, const int* slots, IsoCall* call) {
  const size_t nj = size_t(n);
  auto name = [&](int i) {
    char buf[64];
    if (slots)
      snprintf(buf, sizeof(buf), "isosurface (grid %d, slot %d)", i, slots[i]);
    else
      snprintf(buf, sizeof(buf), "isosurface (grid %d)", i);
    return std::string(buf);
  };
  if (n > 65535) return fail(c, SPRAY_RT_ERR_LIMIT, "isosurface: more than 65535 grids in one call");
  for (int i = 0; i < n; ++i) {
    int code;
    if (const char* why = grid_error(grids[i], &code)) return fail(c, code, "%s: %s", name(i).c_str(), why);
  }
  std::vector<float> cscale(nj, 0.0f);
  for (int i = 0; gcolors && i < n; ++i)
    if (const char* why = color_error(&gcolors[i], &cscale[size_t(i)]))
      return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", name(i).c_str(), why);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then fields and scratch ----
  JobArena& A = c->iso;
  A.reset();
  call->jobs = A.take_head<IsoJob>(nj);
  const size_t m_status = A.mark();
  const auto t_status = A.take_head<uint32_t>(nj);
  const size_t m_rec = A.mark();
  const auto t_rec = A.take_head<IsoRec>(nj);
  call->m_outs = A.mark();
  call->outs = A.take_head<IsoOut>(nj);
  struct Scratch {
    Take<uint32_t> code, vblock, fblock;
    uint32_t npoints, nblocks;
  };
  std::vector<Scratch> sk(nj);
  // items 3 i ..: grid i's field, colour field and colour table, host ones
  // staged inside the arena; a table several grids share is staged once
  Stager stage;
  std::vector<size_t> table_item(nj, 0);
  for (int i = 0; i < n; ++i) {
    const spray_rt_grid& g = grids[i];
    Scratch& k = sk[size_t(i)];
    k.npoints = uint32_t(g.dims[0]) * uint32_t(g.dims[1]) * uint32_t(g.dims[2]);
    k.nblocks = (k.npoints + iso::kIsoBlock - 1) / iso::kIsoBlock;
    stage.place(g.values, size_t(k.npoints) * sizeof(float), &A);
    const spray_rt_grid_color* gc = gcolors && gcolors[i].field ? &gcolors[i] : nullptr;
    stage.place(gc ? gc->field : nullptr, size_t(k.npoints) * sizeof(float), &A);
    table_item[size_t(i)] = 3 * size_t(i) + 2;
    for (int b = 0; gc && b < i; ++b)
      if (gcolors[b].field && gcolors[b].table_rgb == gc->table_rgb &&
          gcolors[b].ntable == gc->ntable) {
        table_item[size_t(i)] = table_item[size_t(b)];
        gc = nullptr;  // an empty item
      }
    stage.place(gc ? gc->table_rgb : nullptr, gc ? size_t(gc->ntable) * sizeof(uint32_t) : 0, &A);
    k.code = A.take<uint32_t>(k.npoints);
    k.vblock = A.take<uint32_t>(k.nblocks);
    k.fblock = A.take<uint32_t>(k.nblocks);
    call->max_blocks = std::max(call->max_blocks, k.nblocks);
  }
  call->staged = stage.any;
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  IsoJob* jobs = A.host(call->jobs);
  uint32_t* h_status = A.host(t_status);
  for (int i = 0; i < n; ++i) {
    const spray_rt_grid& g = grids[i];
    const Scratch& k = sk[size_t(i)];
    IsoJob J{};
    J.values = stage.dev<float>(3 * size_t(i));
    if (gcolors && gcolors[i].field) {
      J.cfield = stage.dev<float>(3 * size_t(i) + 1);
      J.ctable = stage.dev<uint32_t>(table_item[size_t(i)]);
      J.ntable = gcolors[i].ntable;
      J.clo = gcolors[i].lo;
      J.cscale = cscale[size_t(i)];
    }
    J.code = A.dev(k.code);
    J.vblock = A.dev(k.vblock);
    J.fblock = A.dev(k.fblock);
    J.rec = A.dev(t_rec) + i;
    J.nx = g.dims[0];
    J.ny = g.dims[1];
    J.nz = g.dims[2];
    J.npoints = k.npoints;
    J.nblocks = k.nblocks;
    for (int a = 0; a < 3; ++a) {
      J.origin[a] = g.origin[a];
      J.spacing[a] = g.spacing[a];
    }
    J.isovalue = g.isovalue;
    J.color = g.color_rgb;
    jobs[i] = J;
    h_status[i] = 0;
  }
  HIPCHK(c, arena_copy(A, 0, m_rec, true, s));
  const IsoJob* d_jobs = A.dev(call->jobs);
  HIPCHK(c, launch_iso_count(s, d_jobs, n, call->max_blocks, A.dev(t_status)));
  HIPCHK(c, launch_iso_scan(s, d_jobs, n));
  HIPCHK(c, arena_copy(A, m_status, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the sizes: the extraction's host read
  const IsoRec* h_rec = A.host(t_rec);
  call->rec.assign(h_rec, h_rec + n);
  for (int i = 0; i < n; ++i) {
    if (h_status[i] & iso::kBadSample)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite sample", name(i).c_str());
    if (h_status[i] & iso::kBadColor)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite sample of the colour field",
                  name(i).c_str());
    if (h_rec[i].nfaces >= kMaxFaces || h_rec[i].nverts > UINT32_MAX)
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: 2^29 or more faces", name(i).c_str());
  }
  return SPRAY_RT_OK;
}

// The emit pass of a counted call into outs[n]; colors_only: no out has
// another array than colors.
int iso_emit(spray_rt_ctx* c, int n, const IsoCall& call, const std::vector<IsoOut>& outs,
             bool colors_only = false) {
  hipStream_t s = stream_of(c);
  const JobArena& A = c->iso;
  std::memcpy(A.host(call.outs), outs.data(), size_t(n) * sizeof(IsoOut));
  HIPCHK(c, arena_copy(A, call.m_outs, call.m_outs + size_t(n) * sizeof(IsoOut), true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  HIPCHK(c, launch_iso_emit(s, A.dev(call.jobs), A.dev(call.outs), n, call.max_blocks,
                            colors_only));
  return SPRAY_RT_OK;
}

// spray_rt_domains_isosurface and its mapped form (gcolors nullptr: none).
int domains_isosurface(spray_rt_ctx* c, int n, const int* slots, const spray_rt_grid* grids,
                       const spray_rt_grid_color* gcolors, int with_normals, float* d_bounds,
                       size_t* nfaces_out) {
  if (n < 0 || (n && (!slots || !grids)))
    return fail(c, SPRAY_RT_ERR_ARG, "isosurface: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const size_t nj = size_t(n);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] > 1 << 20)
      return fail(c, SPRAY_RT_ERR_ARG, "isosurface (grid %d): bad slot %d", i, slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail(c, SPRAY_RT_ERR_ARG, "isosurface (grid %d): slot %d listed twice", i, slots[i]);
  }
  IsoCall call;
  int r = iso_count(c, n, grids, gcolors, slots, &call);
  if (r) return r;

  // ---- the meshes: context scratch, sized by the counts ----
  Layout M;  // of d_isomesh
  std::vector<IsoOut> outs(nj, IsoOut{});
  std::vector<Take<float>> t_verts(nj), t_normals(nj);
  std::vector<Take<uint32_t>> t_colors(nj), t_faces(nj);
  std::vector<size_t> nv(nj), nf(nj);
  for (size_t k = 0; k < nj; ++k) {
    outs[k].cap_verts = nv[k] = size_t(call.rec[k].nverts);
    outs[k].cap_faces = nf[k] = size_t(call.rec[k].nfaces);
    t_verts[k] = M.take<float>(3 * nv[k]);
    if (with_normals) t_normals[k] = M.take<float>(3 * nv[k]);
    if (grids[k].has_color || (gcolors && gcolors[k].field)) t_colors[k] = M.take<uint32_t>(nv[k]);
    t_faces[k] = M.take<uint32_t>(3 * nf[k]);
  }
  r = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (r) return r;
  std::vector<const float*> pv(nj), pn(nj);
  std::vector<const uint32_t*> pc(nj), pf(nj);
  for (size_t k = 0; k < nj; ++k) {
    IsoOut& O = outs[k];
    pv[k] = O.verts = t_verts[k].at(c->d_isomesh);
    pn[k] = O.normals = t_normals[k] ? t_normals[k].at(c->d_isomesh) : nullptr;
    pc[k] = O.colors = t_colors[k] ? t_colors[k].at(c->d_isomesh) : nullptr;
    pf[k] = O.faces = t_faces[k].at(c->d_isomesh);
  }
  r = iso_emit(c, n, call, outs);
  if (r) return r;

  // ---- the slots: the device build on the extracted arrays ----
  int job = -1;  // the build names the slot; name the grid as well
  r = domains_build(c, n, slots, pv.data(), nv.data(), pf.data(), nf.data(), pc.data(), pn.data(),
                    d_bounds, &job);
  if (r) {
    const std::string msg = c->err;
    if (job >= 0)
      return fail(c, r, "isosurface (grid %d, slot %d): %s", job, slots[job], msg.c_str());
    return fail(c, r, "isosurface: %s", msg.c_str());
  }
  if (nfaces_out)
    for (size_t k = 0; k < nj; ++k) nfaces_out[k] = nf[k];
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host fields: done on return
  return SPRAY_RT_OK;
}

}  // namespace

extern "C" {

int spray_rt_isosurface_host(const spray_rt_grid* grid, size_t* nverts, size_t* nfaces,
                             float* verts_out, float* vnormals_out, uint32_t* faces_out) {
  if (!grid) return SPRAY_RT_ERR_ARG;
  HostMesh m;
  const bool emit = verts_out || vnormals_out || faces_out;
  const int r = extract_host(*grid, nullptr, emit, vnormals_out != nullptr, false, &m);
  if (nverts) *nverts = size_t(m.nverts);
  if (nfaces) *nfaces = size_t(m.nfaces);
  if (r) return r;
  if (verts_out) std::memcpy(verts_out, m.verts.data(), m.verts.size() * sizeof(float));
  if (vnormals_out) std::memcpy(vnormals_out, m.normals.data(), m.normals.size() * sizeof(float));
  if (faces_out) std::memcpy(faces_out, m.faces.data(), m.faces.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_isosurface(spray_rt_ctx_t c, int n, const spray_rt_grid* grids, float* const* verts,
                        float* const* vnormals, uint32_t* const* faces, const size_t* cap_verts,
                        const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && !grids) || (n && verts && (!faces || !cap_verts || !cap_faces)))
    return fail(c, SPRAY_RT_ERR_ARG, "isosurface: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  IsoCall call;
  const int r = iso_count(c, n, grids, nullptr, nullptr, &call);
  if (r) return r;
  for (int i = 0; i < n; ++i) {
    if (nverts_out) nverts_out[i] = size_t(call.rec[size_t(i)].nverts);
    if (nfaces_out) nfaces_out[i] = size_t(call.rec[size_t(i)].nfaces);
  }
  if (!verts) return SPRAY_RT_OK;
  std::vector<IsoOut> outs(size_t(n), IsoOut{});
  for (int i = 0; i < n; ++i) {
    const IsoRec& rec = call.rec[size_t(i)];
    if (rec.nverts > cap_verts[i] || rec.nfaces > cap_faces[i])
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "isosurface (grid %d): %llu vertices and %llu faces do not fit the buffers", i,
                  static_cast<unsigned long long>(rec.nverts),
                  static_cast<unsigned long long>(rec.nfaces));
    if ((rec.nverts && !verts[i]) || (rec.nfaces && !faces[i]))
      return fail(c, SPRAY_RT_ERR_ARG, "isosurface (grid %d): null output buffers", i);
    IsoOut& O = outs[size_t(i)];
    O.verts = verts[i];
    O.normals = vnormals ? vnormals[i] : nullptr;
    O.faces = faces[i];
    O.cap_verts = rec.nverts;
    O.cap_faces = rec.nfaces;
  }
  const int e = iso_emit(c, n, call, outs);
  if (e) return e;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host fields: done on return
  return SPRAY_RT_OK;
}

int spray_rt_domains_isosurface(spray_rt_ctx_t c, int n, const int* slots,
                                const spray_rt_grid* grids, int with_normals, float* d_bounds,
                                size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  return domains_isosurface(c, n, slots, grids, nullptr, with_normals, d_bounds, nfaces_out);
}

int spray_rt_domains_isosurface_mapped(spray_rt_ctx_t c, int n, const int* slots,
                                       const spray_rt_grid* grids,
                                       const spray_rt_grid_color* gcolors, int with_normals,
                                       float* d_bounds, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  return domains_isosurface(c, n, slots, grids, gcolors, with_normals, d_bounds, nfaces_out);
}

int spray_rt_isosurface_mapped_host(const spray_rt_grid* grid, const spray_rt_grid_color* gcolor,
                                    size_t* nverts, size_t* nfaces, float* verts_out,
                                    float* vnormals_out, uint32_t* colors_out,
                                    uint32_t* faces_out) {
  if (!grid) return SPRAY_RT_ERR_ARG;
  HostMesh m;
  const bool emit = verts_out || vnormals_out || colors_out || faces_out;
  const int r = extract_host(*grid, gcolor, emit, vnormals_out != nullptr, colors_out != nullptr, &m);
  if (nverts) *nverts = size_t(m.nverts);
  if (nfaces) *nfaces = size_t(m.nfaces);
  if (r) return r;
  if (verts_out) std::memcpy(verts_out, m.verts.data(), m.verts.size() * sizeof(float));
  if (vnormals_out) std::memcpy(vnormals_out, m.normals.data(), m.normals.size() * sizeof(float));
  if (colors_out) std::memcpy(colors_out, m.colors.data(), m.colors.size() * sizeof(uint32_t));
  if (faces_out) std::memcpy(faces_out, m.faces.data(), m.faces.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_isosurface_mapped(spray_rt_ctx_t c, int n, const spray_rt_grid* grids,
                               const spray_rt_grid_color* gcolors, float* const* verts,
                               float* const* vnormals, uint32_t* const* colors,
                               uint32_t* const* faces, const size_t* cap_verts,
                               const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && !grids) ||
      (n && (verts || vnormals || colors) && !cap_verts) || (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "isosurface: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  IsoCall call;
  const int r = iso_count(c, n, grids, gcolors, nullptr, &call);
  if (r) return r;
  for (int i = 0; i < n; ++i) {
    if (nverts_out) nverts_out[i] = size_t(call.rec[size_t(i)].nverts);
    if (nfaces_out) nfaces_out[i] = size_t(call.rec[size_t(i)].nfaces);
  }
  if (!verts && !vnormals && !colors && !faces) return SPRAY_RT_OK;
  std::vector<IsoOut> outs(size_t(n), IsoOut{});
  bool colors_only = true, any = false;
  for (int i = 0; i < n; ++i) {
    const IsoRec& rec = call.rec[size_t(i)];
    IsoOut& O = outs[size_t(i)];
    O.verts = verts ? verts[i] : nullptr;
    O.normals = vnormals ? vnormals[i] : nullptr;
    O.colors = colors ? colors[i] : nullptr;
    O.faces = faces ? faces[i] : nullptr;
    const bool per_vertex = O.verts || O.normals || O.colors;
    if ((per_vertex && rec.nverts > cap_verts[i]) || (O.faces && rec.nfaces > cap_faces[i]))
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "isosurface (grid %d): %llu vertices and %llu faces do not fit the buffers", i,
                  static_cast<unsigned long long>(rec.nverts),
                  static_cast<unsigned long long>(rec.nfaces));
    O.cap_verts = per_vertex ? rec.nverts : 0;
    O.cap_faces = O.faces ? rec.nfaces : 0;
    if (O.verts || O.normals || O.faces) colors_only = false;
    any = any || per_vertex || O.faces;
  }
  if (!any) return SPRAY_RT_OK;
  const int e = iso_emit(c, n, call, outs, colors_only);
  if (e) return e;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host fields: done on return
  return SPRAY_RT_OK;
}

int spray_rt_colormap_host(const float* scalars, size_t n, const uint32_t* table_rgb,
                           int32_t ntable, float lo, float hi, uint32_t* colors_out) {
  float scale;
  if (map_error(table_rgb, ntable, lo, hi, &scale)) return SPRAY_RT_ERR_ARG;
  if (n && (!scalars || !colors_out)) return SPRAY_RT_ERR_ARG;
  for (size_t i = 0; i < n; ++i)
    if (!refit::finite_f(scalars[i])) return SPRAY_RT_ERR_ARG;
  for (size_t i = 0; i < n; ++i) colors_out[i] = table_rgb[cmap::bin(scalars[i], lo, scale, ntable)];
  return SPRAY_RT_OK;
}

int spray_rt_colormap_apply(spray_rt_ctx_t c, const float* scalars, size_t n,
                            const uint32_t* table_rgb, int32_t ntable, float lo, float hi,
                            uint32_t* colors_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  float scale;
  if (const char* why = map_error(table_rgb, ntable, lo, hi, &scale))
    return fail(c, SPRAY_RT_ERR_ARG, "colormap: %s", why);
  if (n && (!scalars || !colors_out)) return fail(c, SPRAY_RT_ERR_ARG, "colormap: null arguments");
  if (n >= kMaxPoints) return fail(c, SPRAY_RT_ERR_LIMIT, "colormap: 2^31 or more scalars");
  if (n == 0) return SPRAY_RT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (!is_device_ptr(colors_out))
    return fail(c, SPRAY_RT_ERR_ARG, "colormap: colors_out is not device memory");
  hipStream_t s = stream_of(c);
  // ---- layout: the status word (mirrored), then the table and host scalars ----
  JobArena& A = c->iso;
  A.reset();
  const auto t_status = A.take_head<uint32_t>(1);
  Stager stage;  // items: the scalars, the table
  stage.place(scalars, n * sizeof(float), &A);
  stage.place(table_rgb, size_t(ntable) * sizeof(uint32_t), &A);
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  uint32_t* h_status = A.host(t_status);
  *h_status = 0;
  HIPCHK(c, arena_copy(A, 0, A.head, true, s));
  HIPCHK(c, launch_colormap_apply(s, stage.dev<float>(0), n, stage.dev<uint32_t>(1), ntable, lo,
                                  scale, colors_out, A.dev(t_status)));
  HIPCHK(c, arena_copy(A, 0, A.head, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the call's one host read
  if (*h_status & cmap::kBadScalar)
    return fail(c, SPRAY_RT_ERR_ARG, "colormap: non-finite scalar");
  return SPRAY_RT_OK;
}

int spray_rt_domains_recolor(spray_rt_ctx_t c, int n, const int* slots,
                             const uint32_t* const* colors_rgb, const size_t* nverts) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!slots || !colors_rgb || !nverts)))
    return fail(c, SPRAY_RT_ERR_ARG, "recolor: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  if (n > 65535) return fail(c, SPRAY_RT_ERR_LIMIT, "recolor: more than 65535 slots in one call");
  // ---- host-side validation: nothing is enqueued before it passes ----
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || size_t(slots[i]) >= c->slots.size() || !c->slots[size_t(slots[i])].dmem)
      return fail(c, SPRAY_RT_ERR_ARG, "recolor: slot %d is not loaded", slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail(c, SPRAY_RT_ERR_ARG, "recolor: slot %d listed twice", slots[i]);
    const SlotHost& sh = c->slots[size_t(slots[i])];
    if (nverts[i] != size_t(sh.desc.nverts))
      return fail(c, SPRAY_RT_ERR_ARG, "recolor: slot %d has %u vertices, the call brings %zu",
                  slots[i], sh.desc.nverts, nverts[i]);
    if (!sh.desc.nverts) continue;  // nothing to write
    if (!sh.desc.colors)
      return fail(c, SPRAY_RT_ERR_ARG, "recolor: slot %d carries no colours", slots[i]);
    if (!colors_rgb[i])
      return fail(c, SPRAY_RT_ERR_ARG, "recolor: null colour array for slot %d", slots[i]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);
  // ---- layout: the job table (mirrored), then the host arrays ----
  const size_t nj = size_t(n);
  JobArena& A = c->recolor;
  A.reset();
  const auto t_jobs = A.take_head<RecolorJob>(nj);
  Stager stage;  // item i: job i's colours
  for (int i = 0; i < n; ++i) stage.place(colors_rgb[i], nverts[i] * sizeof(uint32_t), &A);
  // the pinned table of the previous call is free once its copy has run
  if (c->recolor_copied) HIPCHK(c, hipEventSynchronize(c->recolor_copied));
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  RecolorJob* jobs = A.host(t_jobs);
  uint32_t max_n = 0;
  for (int i = 0; i < n; ++i) {
    const SlotHost& sh = c->slots[size_t(slots[i])];
    // the slot's async upload, if one is pending, comes first
    if (sh.ready) HIPCHK(c, hipStreamWaitEvent(s, sh.ready, 0));
    RecolorJob J{};
    J.dst = const_cast<uint32_t*>(sh.desc.colors);
    J.src = stage.dev<uint32_t>(size_t(i));
    J.n = sh.desc.nverts;
    jobs[i] = J;
    max_n = std::max(max_n, J.n);
  }
  HIPCHK(c, arena_copy(A, 0, A.head, true, s));
  if (!c->recolor_copied)
    HIPCHK(c, hipEventCreateWithFlags(&c->recolor_copied, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->recolor_copied, s));
  HIPCHK(c, launch_recolor(s, A.dev(t_jobs), n, max_n));
  if (stage.any) HIPCHK(c, hipStreamSynchronize(s));  // host arrays: done on return
  return SPRAY_RT_OK;
}

}  // extern "C"
