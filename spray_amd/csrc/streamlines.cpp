// streamlines.cpp -- streamlines of vector grids: spray_rt_streamlines (the
// polylines), spray_rt_stream_tubes (their tubes as indexed triangle meshes),
// spray_rt_domains_stream_tubes (the tubes into resident slots) and the
// host-only restatements (include/spray_rt.h).
//
// The integration runs on the device (stream_kernels.hip) on fields and seeds
// that may already be in HBM: a check pass and a count pass, the call's one
// host read (the sizes), then the integrate pass again with the same
// arithmetic into the caller's buffers or into context scratch, from where the
// expansion writes the tubes and spray_rt_domains_build makes slots of them.
// Nothing is written to a slot or a caller buffer before every check has
// passed ("Streamlines").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "color_common.h"
#include "rt_common.h"
#ifndef SPRAY_RT_STREAM_HOST_ONLY
#include "rt_ctx.h"
#endif
#include "spray_rt.h"
#include "stream_common.h"
#include "stream_host.h"
#include "stream_kernels.h"

using namespace spray_rt;
using namespace spray_rt::detail;
using namespace spray_rt::strmhost;

namespace spray_rt {
namespace strmhost {

constexpr uint64_t kMaxLinePoints = uint64_t(1) << 32;
constexpr uint64_t kMaxVerts = uint64_t(1) << 32;
constexpr uint64_t kMaxFaces = uint64_t(1) << 29;

const char* tube_error(const spray_rt_tube& t) {
  if (!(t.radius > 0.0f) || !refit::finite_f(t.radius)) return "radius is not positive and finite";
  if (t.nsides < 3 || t.nsides > strm::kMaxSides) return "nsides is not in 3 .. 16";
  return nullptr;
}

const char* totals_error(uint64_t npoints, uint64_t nverts, uint64_t nfaces) {
  if (npoints >= kMaxLinePoints) return "2^32 or more points of lines";
  if (nverts >= kMaxVerts) return "2^32 or more vertices";
  if (nfaces >= kMaxFaces) return "2^29 or more faces";
  return nullptr;
}

void ring_table(int nsides, float out[][2]) {
  for (int k = 0; k < nsides; ++k) {
    const double a = (6.283185307179586 * double(k)) / double(nsides);
    out[k][0] = float(std::cos(a));
    out[k][1] = float(std::sin(a));
  }
}

const char* color_table_error(const uint32_t* table_rgb, int32_t ntable, float lo, float hi,
                              float* scale) {
  *scale = 0.0f;
  if (!table_rgb) return "null colour table";
  if (ntable < 1 || ntable > cmap::kMaxTable)
    return "colour table of fewer than 1 or more than 4096 entries";
  if (!refit::finite_f(lo) || !refit::finite_f(hi) || !(lo < hi))
    return "colour range is not lo < hi, both finite";
  if (!cmap::map_scale(ntable, lo, hi, scale))
    return "colour scale ntable / (hi - lo) is not a finite normal float";
  return nullptr;
}

const char* trace_error(float step, int32_t max_steps, int32_t direction, float min_speed) {
  if (!(step > 0.0f) || !refit::finite_f(step)) return "step is not positive and finite";
  if (max_steps < 0 || max_steps > strm::kMaxSteps) return "max_steps is not in 0 .. 65535";
  if (direction < SPRAY_RT_STREAM_FORWARD || direction > SPRAY_RT_STREAM_BOTH)
    return "bad direction";
  const float msq = min_speed * min_speed;
  if (!(min_speed > 0.0f) || !refit::finite_f(msq) || !(msq >= 1.17549435e-38f))
    return "min_speed is not positive with a normal square";
  return nullptr;
}

void tubes_host(const HostLines& L, const spray_rt_tube& tube, float* verts_out,
                float* vnormals_out, uint32_t* colors_out, uint32_t* faces_out) {
  const uint32_t ns = uint32_t(tube.nsides);
  float ring[strm::kMaxSides][2];
  ring_table(tube.nsides, ring);
  size_t v0 = 0, f0 = 0;
  for (size_t l = 0; l + 1 < L.off.size(); ++l) {
    const size_t p0 = L.off[l];
    const uint32_t m = L.off[l + 1] - L.off[l];
    if (m < 2) continue;
    for (uint32_t r = 0; r < uint32_t(strm::tube_verts(m, ns)); ++r) {
      const bool is_ring = r < m * ns;
      const uint32_t j = is_ring ? r / ns : (r == m * ns ? 0u : m - 1), k = is_ring ? r - j * ns : 0u;
      const float *P = &L.P[3 * (p0 + j)], *N = &L.N[3 * (p0 + j)], *T = &L.T[3 * (p0 + j)];
      float pos[3], nrm[3];
      if (is_ring) {
        float B[3];
        strm::cross3(T, N, B);
        strm::ring_vertex(P, N, B, ring[k][0], ring[k][1], tube.radius, pos, nrm);
      } else {
        for (int a = 0; a < 3; ++a) {
          pos[a] = P[a];
          nrm[a] = j ? T[a] : -T[a];
        }
      }
      for (int a = 0; a < 3; ++a) {
        if (verts_out) verts_out[3 * (v0 + r) + size_t(a)] = pos[a];
        if (vnormals_out) vnormals_out[3 * (v0 + r) + size_t(a)] = nrm[a];
      }
      if (colors_out) colors_out[v0 + r] = L.col[p0 + j];
    }
    for (uint32_t r = 0; faces_out && r < uint32_t(strm::tube_faces(m, ns)); ++r) {
      uint32_t f[3];
      strm::tube_face(ns, m, r, f);
      for (int a = 0; a < 3; ++a) faces_out[3 * (f0 + r) + size_t(a)] = uint32_t(v0) + f[a];
    }
    v0 += size_t(strm::tube_verts(m, ns));
    f0 += size_t(strm::tube_faces(m, ns));
  }
}

void take_tube_scratch(Layout* M, size_t nseeds, const StreamRec& rec, TubeScratch* t) {
  const size_t np = size_t(rec.npoints);
  t->points = M->take<float>(3 * np);
  t->pnormals = M->take<float>(3 * np);
  t->ptangents = M->take<float>(3 * np);
  t->pcolors = M->take<uint32_t>(np);
  t->line_offsets = M->take<uint32_t>(nseeds + 1);
  t->tube_points = M->take<uint32_t>(nseeds + 1);
  t->tube_lines = M->take<uint32_t>(nseeds + 1);
}
void set_tube_scratch(StreamOut* O, const TubeScratch& t, void* base, const StreamRec& rec) {
  O->points = t.points.at(base);
  O->pnormals = t.pnormals.at(base);
  O->ptangents = t.ptangents.at(base);
  O->pcolors = t.pcolors.at(base);
  O->line_offsets = t.line_offsets.at(base);
  O->tube_points = t.tube_points.at(base);
  O->tube_lines = t.tube_lines.at(base);
  O->cap_points = rec.npoints;
}

}  // namespace strmhost
}  // namespace spray_rt

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// What is wrong with a field's description (nullptr: nothing); *code = the error.
const char* field_error(const spray_rt_vecfield& f, int* code) {
  *code = SPRAY_RT_ERR_ARG;
  if (!f.vectors) return "null vectors";
  if (f.nseeds && !f.seeds) return "null seeds";
  for (int a = 0; a < 3; ++a) {
    if (f.dims[a] < 2) return "fewer than 2 points on an axis";
    if (!(f.spacing[a] > 0.0f) || !refit::finite_f(f.spacing[a]))
      return "spacing is not positive and finite";
    if (!refit::finite_f(f.origin[a])) return "non-finite origin";
  }
  if (const char* why = trace_error(f.step, f.max_steps, f.direction, f.min_speed)) return why;
  *code = SPRAY_RT_ERR_LIMIT;
  if (uint64_t(f.dims[0]) * uint64_t(f.dims[1]) * uint64_t(f.dims[2]) >= kMaxGridPoints)
    return "2^31 or more points";
  if (uint64_t(f.nseeds) >= kMaxSeeds) return "2^31 or more seeds";
  *code = SPRAY_RT_OK;
  return nullptr;
}

// ... with a field's colour map; a field without a colour field has none.
const char* color_error(const spray_rt_grid_color* gc, float* scale) {
  *scale = 0.0f;
  if (!gc || !gc->field) return nullptr;
  return color_table_error(gc->table_rgb, gc->ntable, gc->lo, gc->hi, scale);
}

strm::Grid grid_of(const spray_rt_vecfield& f) {
  strm::Grid G;
  G.vectors = f.vectors;
  for (int a = 0; a < 3; ++a) {
    G.n[a] = f.dims[a];
    G.origin[a] = f.origin[a];
    G.spacing[a] = f.spacing[a];
  }
  return G;
}

// ---- the host restatement, step for step what the kernels do ----

struct Half {
  std::vector<float> P, N, T;
  std::vector<uint32_t> col;
  int end = strm::kEndSteps;  // of a half the direction leaves out
  size_t steps() const { return col.empty() ? 0 : col.size() - 1; }
};

// The validation of the host forms (the kernels' check pass included).
int validate_host(const spray_rt_vecfield& F, const spray_rt_grid_color* gc, float* cscale) {
  int code;
  if (field_error(F, &code)) return code;
  if (color_error(gc, cscale)) return SPRAY_RT_ERR_ARG;
  const size_t np = size_t(F.dims[0]) * size_t(F.dims[1]) * size_t(F.dims[2]);
  for (size_t e = 0; e < 3 * np; ++e)
    if (!refit::finite_f(F.vectors[e])) return SPRAY_RT_ERR_ARG;
  if (gc && gc->field)
    for (size_t e = 0; e < np; ++e)
      if (!refit::finite_f(gc->field[e])) return SPRAY_RT_ERR_ARG;
  for (size_t e = 0; e < 3 * F.nseeds; ++e)
    if (!refit::finite_f(F.seeds[e])) return SPRAY_RT_ERR_ARG;
  return SPRAY_RT_OK;
}

// The lines of a validated field; emit false: the counts alone.
void lines_host(const spray_rt_vecfield& F, const spray_rt_grid_color* gc, float cscale,
                uint32_t color, bool emit, HostLines* L) {
  const strm::Grid G = grid_of(F);
  const float msq = F.min_speed * F.min_speed;
  const float* cf = gc ? gc->field : nullptr;
  const bool do_back = F.direction != SPRAY_RT_STREAM_FORWARD;
  const bool do_fwd = F.direction != SPRAY_RT_STREAM_BACKWARD;
  auto trace = [&](const float* seed, const strm::Cell& c0, float h, Half* H) {
    float p[3] = {seed[0], seed[1], seed[2]};
    strm::Cell c = c0;
    strm::Frame fr = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    for (int steps = 0; steps <= F.max_steps; ++steps) {
      float k1[3], pn[3];
      strm::Cell cn;
      strm::sample_vector(G, c, k1);
      strm::frame_at(k1, msq, steps == 0, &fr);
      H->P.insert(H->P.end(), p, p + 3);
      H->N.insert(H->N.end(), fr.N, fr.N + 3);
      H->T.insert(H->T.end(), fr.T, fr.T + 3);
      H->col.push_back(cf ? gc->table_rgb[cmap::bin(strm::sample_scalar(G, cf, c), gc->lo, cscale,
                                                    gc->ntable)]
                          : color);
      const int r = strm::advance(G, p, k1, h, msq, steps, F.max_steps, pn, &cn);
      if (r != strm::kTaken) {
        H->end = r;
        break;
      }
      for (int a = 0; a < 3; ++a) p[a] = pn[a];
      c = cn;
    }
  };
  auto push = [&](const Half& H, size_t k) {
    L->P.insert(L->P.end(), &H.P[3 * k], &H.P[3 * k] + 3);
    L->N.insert(L->N.end(), &H.N[3 * k], &H.N[3 * k] + 3);
    L->T.insert(L->T.end(), &H.T[3 * k], &H.T[3 * k] + 3);
    L->col.push_back(H.col[k]);
  };
  for (size_t s = 0; s < F.nseeds; ++s) {
    const float* seed = F.seeds + 3 * s;
    if (emit) L->off.push_back(uint32_t(L->npoints));
    strm::Cell c0;
    uint64_t m = 0;
    if (!strm::locate(G, seed, &c0)) {
      if (emit) {
        L->info.push_back(0);
        L->info.push_back(uint32_t(strm::kEndSeed) | (uint32_t(strm::kEndSeed) << 8));
      }
    } else if (!emit) {
      int end;
      m = 1;
      if (do_back) m += uint64_t(strm::trace_count(G, seed, c0, -F.step, msq, F.max_steps, &end));
      if (do_fwd) m += uint64_t(strm::trace_count(G, seed, c0, F.step, msq, F.max_steps, &end));
    } else {
      Half B, W;
      if (do_back) trace(seed, c0, -F.step, &B);
      if (do_fwd) trace(seed, c0, F.step, &W);
      for (size_t k = B.steps(); k >= 1; --k) push(B, k);
      push(do_fwd ? W : B, 0);
      for (size_t k = 1; k <= W.steps(); ++k) push(W, k);
      m = 1 + B.steps() + W.steps();
      L->info.push_back(uint32_t(B.steps()));
      L->info.push_back(uint32_t(B.end) | (uint32_t(W.end) << 8));
    }
    L->npoints += m;
    if (m >= 2) {
      L->tube_points += m;
      L->tube_lines += 1;
    }
  }
  if (emit) L->off.push_back(uint32_t(L->npoints));
}

#ifndef SPRAY_RT_STREAM_HOST_ONLY
// ---- the device extraction: check, count, the host read, integrate, expand ----

struct StreamCall {
  HeadTake<StreamJob> jobs;  // in the context's stream arena
  HeadTake<StreamOut> outs;
  size_t m_outs = 0;  // the mark in front of outs
  uint32_t max_blocks = 0;
  bool staged = false;  // some array came from host memory
  std::vector<StreamRec> rec;
  std::vector<uint64_t> nverts, nfaces;  // of the tubes (zero without tubes)
};

// Validates the fields (their tubes and colour maps where given), runs the
// check pass, the count pass and the scan and reads the sizes (the host read).
// Messages name the field, and its slot where slots is given.
int stream_count(spray_rt_ctx* c, const char* what, int n, const spray_rt_vecfield* fields,
                 const spray_rt_tube* tubes, const spray_rt_grid_color* gcolors, const int* slots,
                 StreamCall* call) {
  const size_t nj = size_t(n);
  auto name = [&](int i) {
    char buf[96];
    if (slots)
      snprintf(buf, sizeof(buf), "%s (field %d, slot %d)", what, i, slots[i]);
    else
      snprintf(buf, sizeof(buf), "%s (field %d)", what, i);
    return std::string(buf);
  };
  if (n > 65535) return fail(c, SPRAY_RT_ERR_LIMIT, "%s: more than 65535 fields in one call", what);
  std::vector<float> cscale(nj, 0.0f);
  for (int i = 0; i < n; ++i) {
    int code;
    if (const char* why = field_error(fields[i], &code))
      return fail(c, code, "%s: %s", name(i).c_str(), why);
    if (tubes)
      if (const char* why = tube_error(tubes[i]))
        return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", name(i).c_str(), why);
    if (gcolors)
      if (const char* why = color_error(&gcolors[i], &cscale[size_t(i)]))
        return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", name(i).c_str(), why);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then arrays and scratch ----
  JobArena& A = c->stream;
  A.reset();
  call->jobs = A.take_head<StreamJob>(nj);
  const size_t m_status = A.mark();
  const auto t_status = A.take_head<uint32_t>(nj);
  const size_t m_rec = A.mark();
  const auto t_rec = A.take_head<StreamRec>(nj);
  call->m_outs = A.mark();
  call->outs = A.take_head<StreamOut>(nj);
  struct Scratch {
    Take<uint32_t> word;
    Take<uint64_t> loc;
    Take<uint4> bbase;
    uint32_t nlanes, nblocks;
  };
  std::vector<Scratch> sk(nj);
  // items 4 i ..: field i's vectors, seeds, colour field and colour table, host
  // ones staged inside the arena
  Stager stage;
  for (int i = 0; i < n; ++i) {
    const spray_rt_vecfield& f = fields[i];
    Scratch& k = sk[size_t(i)];
    const size_t np = size_t(f.dims[0]) * size_t(f.dims[1]) * size_t(f.dims[2]);
    k.nlanes = uint32_t(f.nseeds) * (f.direction == SPRAY_RT_STREAM_BOTH ? 2u : 1u);
    k.nblocks = (k.nlanes + strm::kBlock - 1) / strm::kBlock;
    const spray_rt_grid_color* gc = gcolors && gcolors[i].field ? &gcolors[i] : nullptr;
    stage.place(f.vectors, 3 * np * sizeof(float), &A);
    stage.place(f.seeds, 3 * f.nseeds * sizeof(float), &A);
    stage.place(gc ? gc->field : nullptr, np * sizeof(float), &A);
    stage.place(gc ? gc->table_rgb : nullptr, gc ? size_t(gc->ntable) * sizeof(uint32_t) : 0, &A);
    k.word = A.take<uint32_t>(k.nlanes);
    k.loc = A.take<uint64_t>(k.nlanes);
    k.bbase = A.take<uint4>(k.nblocks);
    call->max_blocks = std::max(call->max_blocks, k.nblocks);
  }
  call->staged = stage.any;
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  StreamJob* jobs = A.host(call->jobs);
  uint32_t* h_status = A.host(t_status);
  for (int i = 0; i < n; ++i) {
    const spray_rt_vecfield& f = fields[i];
    const Scratch& k = sk[size_t(i)];
    StreamJob J{};
    J.vectors = stage.dev<float>(4 * size_t(i));
    J.seeds = stage.dev<float>(4 * size_t(i) + 1);
    if (gcolors && gcolors[i].field) {
      J.cfield = stage.dev<float>(4 * size_t(i) + 2);
      J.ctable = stage.dev<uint32_t>(4 * size_t(i) + 3);
      J.ntable = gcolors[i].ntable;
      J.clo = gcolors[i].lo;
      J.cscale = cscale[size_t(i)];
    }
    J.word = A.dev(k.word);
    J.loc = A.dev(k.loc);
    J.bbase = A.dev(k.bbase);
    J.rec = A.dev(t_rec) + i;
    for (int a = 0; a < 3; ++a) {
      J.dims[a] = f.dims[a];
      J.origin[a] = f.origin[a];
      J.spacing[a] = f.spacing[a];
    }
    J.nseeds = uint32_t(f.nseeds);
    J.nlanes = k.nlanes;
    J.nblocks = k.nblocks;
    J.step = f.step;
    J.msq = f.min_speed * f.min_speed;
    J.max_steps = f.max_steps;
    J.direction = f.direction;
    if (tubes) {
      J.color = tubes[i].color_rgb;
      J.radius = tubes[i].radius;
      J.nsides = tubes[i].nsides;
      ring_table(J.nsides, J.ring);
    }
    jobs[i] = J;
    h_status[i] = 0;
  }
  HIPCHK(c, arena_copy(A, 0, m_rec, true, s));
  const StreamJob* d_jobs = A.dev(call->jobs);
  HIPCHK(c, launch_stream_check(s, d_jobs, n, A.dev(t_status)));
  HIPCHK(c, launch_stream_count(s, d_jobs, n, call->max_blocks));
  HIPCHK(c, launch_stream_scan(s, d_jobs, n));
  HIPCHK(c, arena_copy(A, m_status, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the sizes: the call's host read
  const StreamRec* h_rec = A.host(t_rec);
  call->rec.assign(h_rec, h_rec + n);
  call->nverts.assign(nj, 0);
  call->nfaces.assign(nj, 0);
  for (int i = 0; i < n; ++i) {
    if (h_status[i] & strm::kBadVector)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite vector sample", name(i).c_str());
    if (h_status[i] & strm::kBadColor)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite sample of the colour field",
                  name(i).c_str());
    if (h_status[i] & strm::kBadSeed)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite seed coordinate", name(i).c_str());
    if (tubes) {
      const uint64_t ns = uint64_t(tubes[i].nsides);
      call->nverts[size_t(i)] = h_rec[i].tube_points * ns + 2 * h_rec[i].tube_lines;
      call->nfaces[size_t(i)] = 2 * ns * h_rec[i].tube_points;
    }
    if (const char* why =
            totals_error(h_rec[i].npoints, call->nverts[size_t(i)], call->nfaces[size_t(i)]))
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: %s", name(i).c_str(), why);
  }
  return SPRAY_RT_OK;
}

// The integrate pass of a counted call into outs[n], and with tubes the
// expansion.
int stream_emit(spray_rt_ctx* c, int n, const StreamCall& call, const std::vector<StreamOut>& outs,
                bool tubes) {
  hipStream_t s = stream_of(c);
  const JobArena& A = c->stream;
  std::memcpy(A.host(call.outs), outs.data(), size_t(n) * sizeof(StreamOut));
  HIPCHK(c, arena_copy(A, call.m_outs, call.m_outs + size_t(n) * sizeof(StreamOut), true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  HIPCHK(c, launch_stream_integrate(s, A.dev(call.jobs), A.dev(call.outs), n, call.max_blocks,
                                    tubes));
  if (tubes) {
    uint64_t max_items = 0;
    for (int i = 0; i < n; ++i)
      max_items = std::max(max_items, std::max(outs[size_t(i)].cap_verts ? call.nverts[size_t(i)] : 0,
                                               outs[size_t(i)].cap_faces ? call.nfaces[size_t(i)] : 0));
    HIPCHK(c, launch_stream_expand(s, A.dev(call.jobs), A.dev(call.outs), n, max_items));
  }
  return SPRAY_RT_OK;
}
#endif  // SPRAY_RT_STREAM_HOST_ONLY

}  // namespace

extern "C" {

int spray_rt_tube_ring_host(int32_t nsides, float out[][2]) {
  if (nsides < 3 || nsides > strm::kMaxSides || !out) return SPRAY_RT_ERR_ARG;
  ring_table(nsides, out);
  return SPRAY_RT_OK;
}

int spray_rt_streamlines_host(const spray_rt_vecfield* field, size_t* npoints, float* points_out,
                              uint32_t* line_offsets_out, uint32_t* line_info_out) {
  if (!field) return SPRAY_RT_ERR_ARG;
  if (npoints) *npoints = 0;
  float cscale;
  if (const int r = validate_host(*field, nullptr, &cscale)) return r;
  HostLines L;
  const bool emit = points_out || line_offsets_out || line_info_out;
  lines_host(*field, nullptr, 0.0f, 0u, emit, &L);
  if (npoints) *npoints = size_t(L.npoints);
  if (totals_error(L.npoints, 0, 0)) return SPRAY_RT_ERR_LIMIT;
  if (points_out) std::memcpy(points_out, L.P.data(), L.P.size() * sizeof(float));
  if (line_offsets_out)
    std::memcpy(line_offsets_out, L.off.data(), L.off.size() * sizeof(uint32_t));
  if (line_info_out) std::memcpy(line_info_out, L.info.data(), L.info.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_stream_tubes_host(const spray_rt_vecfield* field, const spray_rt_tube* tube,
                               const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                               float* verts_out, float* vnormals_out, uint32_t* colors_out,
                               uint32_t* faces_out) {
  if (!field || !tube) return SPRAY_RT_ERR_ARG;
  if (nverts) *nverts = 0;
  if (nfaces) *nfaces = 0;
  if (tube_error(*tube)) return SPRAY_RT_ERR_ARG;
  float cscale;
  if (const int r = validate_host(*field, gcolor, &cscale)) return r;
  HostLines L;
  const bool emit = verts_out || vnormals_out || colors_out || faces_out;
  lines_host(*field, gcolor, cscale, tube->color_rgb, emit, &L);
  const uint32_t ns = uint32_t(tube->nsides);
  const uint64_t nv = L.tube_points * ns + 2 * L.tube_lines, nf = 2 * uint64_t(ns) * L.tube_points;
  if (nverts) *nverts = size_t(nv);
  if (nfaces) *nfaces = size_t(nf);
  if (totals_error(L.npoints, nv, nf)) return SPRAY_RT_ERR_LIMIT;
  if (!emit) return SPRAY_RT_OK;
  tubes_host(L, *tube, verts_out, vnormals_out, colors_out, faces_out);
  return SPRAY_RT_OK;
}

#ifndef SPRAY_RT_STREAM_HOST_ONLY
int spray_rt_stream_phase_times(spray_rt_ctx_t c, double out_ms[3]) {
  if (!c || !out_ms) return SPRAY_RT_ERR_ARG;
  for (int k = 0; k < 3; ++k) out_ms[k] = c->stream_ms[k];
  return SPRAY_RT_OK;
}

int spray_rt_streamlines(spray_rt_ctx_t c, int n, const spray_rt_vecfield* fields,
                         float* const* points, uint32_t* const* line_offsets,
                         uint32_t* const* line_info, const size_t* cap_points,
                         size_t* npoints_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && !fields) || (n && points && !cap_points))
    return fail(c, SPRAY_RT_ERR_ARG, "streamlines: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const auto t0 = Clock::now();
  c->stream_ms[0] = c->stream_ms[1] = c->stream_ms[2] = 0.0;
  StreamCall call;
  const int r = stream_count(c, "streamlines", n, fields, nullptr, nullptr, nullptr, &call);
  c->stream_ms[0] = ms_since(t0);
  if (r) return r;
  for (int i = 0; npoints_out && i < n; ++i) npoints_out[i] = size_t(call.rec[size_t(i)].npoints);
  if (!points) return SPRAY_RT_OK;
  const auto t1 = Clock::now();
  std::vector<StreamOut> outs(size_t(n), StreamOut{});
  for (int i = 0; i < n; ++i) {
    const StreamRec& rec = call.rec[size_t(i)];
    StreamOut& O = outs[size_t(i)];
    O.points = points[i];
    O.line_offsets = line_offsets ? line_offsets[i] : nullptr;
    O.line_info = line_info ? line_info[i] : nullptr;
    if (O.points && rec.npoints > cap_points[i])
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "streamlines (field %d): %llu points do not fit the buffer", i,
                  static_cast<unsigned long long>(rec.npoints));
    O.cap_points = O.points ? rec.npoints : 0;
  }
  const int e = stream_emit(c, n, call, outs, false);
  if (e) return e;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->stream_ms[1] = ms_since(t1);
  return SPRAY_RT_OK;
}

int spray_rt_stream_tubes(spray_rt_ctx_t c, int n, const spray_rt_vecfield* fields,
                          const spray_rt_tube* tubes, const spray_rt_grid_color* gcolors,
                          float* const* verts, float* const* vnormals, uint32_t* const* colors,
                          uint32_t* const* faces, const size_t* cap_verts, const size_t* cap_faces,
                          size_t* nverts_out, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!fields || !tubes)) || (n && (verts || vnormals || colors) && !cap_verts) ||
      (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "stream_tubes: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const auto t0 = Clock::now();
  c->stream_ms[0] = c->stream_ms[1] = c->stream_ms[2] = 0.0;
  StreamCall call;
  const int r = stream_count(c, "stream_tubes", n, fields, tubes, gcolors, nullptr, &call);
  c->stream_ms[0] = ms_since(t0);
  if (r) return r;
  for (int i = 0; i < n; ++i) {
    if (nverts_out) nverts_out[i] = size_t(call.nverts[size_t(i)]);
    if (nfaces_out) nfaces_out[i] = size_t(call.nfaces[size_t(i)]);
  }
  if (!verts && !vnormals && !colors && !faces) return SPRAY_RT_OK;
  const auto t1 = Clock::now();
  const size_t nj = size_t(n);
  std::vector<StreamOut> outs(nj, StreamOut{});
  bool any = false;
  for (int i = 0; i < n; ++i) {
    StreamOut& O = outs[size_t(i)];
    O.verts = verts ? verts[i] : nullptr;
    O.vnormals = vnormals ? vnormals[i] : nullptr;
    O.colors = colors ? colors[i] : nullptr;
    O.faces = faces ? faces[i] : nullptr;
    const bool per_vertex = O.verts || O.vnormals || O.colors;
    const uint64_t nv = call.nverts[size_t(i)], nf = call.nfaces[size_t(i)];
    if ((per_vertex && nv > cap_verts[i]) || (O.faces && nf > cap_faces[i]))
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "stream_tubes (field %d): %llu vertices and %llu faces do not fit the buffers", i,
                  static_cast<unsigned long long>(nv), static_cast<unsigned long long>(nf));
    O.cap_verts = per_vertex ? nv : 0;
    O.cap_faces = O.faces ? nf : 0;
    any = any || per_vertex || O.faces;
  }
  if (!any) return SPRAY_RT_OK;
  Layout M;  // of d_isomesh
  std::vector<TubeScratch> ts(nj);
  for (size_t k = 0; k < nj; ++k) take_tube_scratch(&M, fields[k].nseeds, call.rec[k], &ts[k]);
  const int g = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (g) return g;
  for (size_t k = 0; k < nj; ++k) set_tube_scratch(&outs[k], ts[k], c->d_isomesh, call.rec[k]);
  const int e = stream_emit(c, n, call, outs, true);
  if (e) return e;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->stream_ms[1] = ms_since(t1);
  return SPRAY_RT_OK;
}

int spray_rt_domains_stream_tubes(spray_rt_ctx_t c, int n, const int* slots,
                                  const spray_rt_vecfield* fields, const spray_rt_tube* tubes,
                                  const spray_rt_grid_color* gcolors, int with_normals,
                                  float* d_bounds, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!slots || !fields || !tubes)))
    return fail(c, SPRAY_RT_ERR_ARG, "stream_tubes: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const size_t nj = size_t(n);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] > 1 << 20)
      return fail(c, SPRAY_RT_ERR_ARG, "stream_tubes (field %d): bad slot %d", i, slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail(c, SPRAY_RT_ERR_ARG, "stream_tubes (field %d): slot %d listed twice", i,
                    slots[i]);
  }
  const auto t0 = Clock::now();
  c->stream_ms[0] = c->stream_ms[1] = c->stream_ms[2] = 0.0;
  StreamCall call;
  int r = stream_count(c, "stream_tubes", n, fields, tubes, gcolors, slots, &call);
  c->stream_ms[0] = ms_since(t0);
  if (r) return r;

  // ---- the lines' scratch and the meshes: context scratch, sized by the counts ----
  const auto t1 = Clock::now();
  Layout M;  // of d_isomesh
  std::vector<StreamOut> outs(nj, StreamOut{});
  std::vector<TubeScratch> ts(nj);
  std::vector<Take<float>> t_verts(nj), t_normals(nj);
  std::vector<Take<uint32_t>> t_colors(nj), t_faces(nj);
  std::vector<size_t> nv(nj), nf(nj);
  for (size_t k = 0; k < nj; ++k) {
    take_tube_scratch(&M, fields[k].nseeds, call.rec[k], &ts[k]);
    outs[k].cap_verts = nv[k] = size_t(call.nverts[k]);
    outs[k].cap_faces = nf[k] = size_t(call.nfaces[k]);
    t_verts[k] = M.take<float>(3 * nv[k]);
    if (with_normals) t_normals[k] = M.take<float>(3 * nv[k]);
    if (tubes[k].has_color || (gcolors && gcolors[k].field)) t_colors[k] = M.take<uint32_t>(nv[k]);
    t_faces[k] = M.take<uint32_t>(3 * nf[k]);
  }
  r = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (r) return r;
  std::vector<const float*> pv(nj), pn(nj);
  std::vector<const uint32_t*> pc(nj), pf(nj);
  for (size_t k = 0; k < nj; ++k) {
    StreamOut& O = outs[k];
    set_tube_scratch(&O, ts[k], c->d_isomesh, call.rec[k]);
    pv[k] = O.verts = t_verts[k].at(c->d_isomesh);
    pn[k] = O.vnormals = t_normals[k] ? t_normals[k].at(c->d_isomesh) : nullptr;
    pc[k] = O.colors = t_colors[k] ? t_colors[k].at(c->d_isomesh) : nullptr;
    pf[k] = O.faces = t_faces[k].at(c->d_isomesh);
  }
  r = stream_emit(c, n, call, outs, true);
  if (r) return r;
  c->stream_ms[1] = ms_since(t1);

  // ---- the slots: the device build on the expanded arrays ----
  const auto t2 = Clock::now();
  int job = -1;  // the build names the slot; name the field as well
  r = domains_build(c, n, slots, pv.data(), nv.data(), pf.data(), nf.data(), pc.data(), pn.data(),
                    d_bounds, &job);
  if (r) {
    const std::string msg = c->err;
    if (job >= 0)
      return fail(c, r, "stream_tubes (field %d, slot %d): %s", job, slots[job], msg.c_str());
    return fail(c, r, "stream_tubes: %s", msg.c_str());
  }
  if (nfaces_out)
    for (size_t k = 0; k < nj; ++k) nfaces_out[k] = nf[k];
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->stream_ms[2] = ms_since(t2);
  return SPRAY_RT_OK;
}
#endif  // SPRAY_RT_STREAM_HOST_ONLY

}  // extern "C"
