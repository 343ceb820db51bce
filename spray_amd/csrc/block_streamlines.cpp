// block_streamlines.cpp -- streamlines across the blocks of a multi-block
// vector field: spray_rt_block_streamlines (the polylines and the block of
// every point), spray_rt_block_stream_tubes (their tubes),
// spray_rt_domains_block_stream_tubes (a set's tubes into one resident slot)
// and the host-only restatements (include/spray_rt.h).
//
// The passes are streamlines.cpp's: check and count, the call's one host read
// (the sizes), the integrate pass again with the same arithmetic, the tube
// expansion and spray_rt_domains_build.  A set has a StreamJob as a field has,
// so the scan and the expansion are the single-grid launches; the check, count
// and integrate kernels (block_stream_kernels.hip) take the set's blocks from
// a table of block records.  Nothing is written to a slot or a caller buffer
// before every check has passed ("Streamlines across blocks").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "block_stream_common.h"
#include "block_stream_kernels.h"
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

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// What is wrong with a set's description (nullptr: nothing); *code = the error,
// *block = the block at fault (-1: none).  colored: the set has a colour table.
const char* set_error(const spray_rt_blockfield& S, bool colored, int* code, int* block) {
  *code = SPRAY_RT_ERR_ARG;
  *block = -1;
  if (S.nblocks < 1 || S.nblocks > bstrm::kMaxBlocks) return "nblocks is not in 1 .. 65535";
  if (!S.blocks) return "null blocks";
  if (S.nseeds && !S.seeds) return "null seeds";
  for (int b = 0; b < S.nblocks; ++b) {
    const spray_rt_vecblock& B = S.blocks[b];
    *block = b;
    if (!B.vectors) return "null vectors";
    for (int a = 0; a < 3; ++a) {
      if (B.dims[a] < 2) return "fewer than 2 points on an axis";
      if (!(B.spacing[a] > 0.0f) || !refit::finite_f(B.spacing[a]))
        return "spacing is not positive and finite";
      if (!refit::finite_f(B.origin[a])) return "non-finite origin";
    }
    if ((B.color_field != nullptr) != (S.blocks[0].color_field != nullptr))
      return "colour fields on some blocks of the set but not on all";
  }
  *block = -1;
  if (colored && !S.blocks[0].color_field)
    return "a colour table for a set whose blocks have no colour field";
  if (const char* why = trace_error(S.step, S.max_steps, S.direction, S.min_speed)) return why;
  *code = SPRAY_RT_ERR_LIMIT;
  for (int b = 0; b < S.nblocks; ++b) {
    const spray_rt_vecblock& B = S.blocks[b];
    *block = b;
    if (uint64_t(B.dims[0]) * uint64_t(B.dims[1]) * uint64_t(B.dims[2]) >= kMaxGridPoints)
      return "2^31 or more points";
  }
  *block = -1;
  if (uint64_t(S.nseeds) >= kMaxSeeds) return "2^31 or more seeds";
  *code = SPRAY_RT_OK;
  return nullptr;
}

// ... with a set's colour map: a set without a table has none; one with colour
// fields needs one (tubes only).
const char* color_error(const spray_rt_blockfield& S, const spray_rt_block_color* bc, float* scale) {
  *scale = 0.0f;
  if (!S.blocks[0].color_field) return nullptr;
  if (!bc) return "colour fields without a colour table";
  return color_table_error(bc->table_rgb, bc->ntable, bc->lo, bc->hi, scale);
}

bool has_table(const spray_rt_block_color* bc) { return bc && bc->table_rgb; }

size_t block_points(const spray_rt_vecblock& B) {
  return size_t(B.dims[0]) * size_t(B.dims[1]) * size_t(B.dims[2]);
}

bstrm::BlockRec rec_of(const spray_rt_vecblock& B, const float* vectors, const float* cfield) {
  bstrm::BlockRec R{};
  for (int a = 0; a < 3; ++a) {
    R.origin[a] = B.origin[a];
    R.spacing[a] = B.spacing[a];
    R.n[a] = B.dims[a];
  }
  R.vectors = vectors;
  R.cfield = cfield;
  return R;
}

// ---- the host restatement, step for step what the kernels do ----

struct HostBlockLines : HostLines {
  std::vector<uint32_t> blk;  // per point
};

struct Half {
  std::vector<float> P, N, T;
  std::vector<uint32_t> col, blk;
  int end = strm::kEndSteps;  // of a half the direction leaves out
  size_t steps() const { return col.empty() ? 0 : col.size() - 1; }
};

// The validation of the host forms (the kernels' check pass included).
int validate_host(const spray_rt_blockfield& S, const spray_rt_block_color* bc, bool tubes,
                  float* cscale) {
  int code, block;
  *cscale = 0.0f;
  if (set_error(S, has_table(bc), &code, &block)) return code;
  if (tubes && color_error(S, bc, cscale)) return SPRAY_RT_ERR_ARG;
  for (int b = 0; b < S.nblocks; ++b) {
    const spray_rt_vecblock& B = S.blocks[b];
    const size_t np = block_points(B);
    for (size_t e = 0; e < 3 * np; ++e)
      if (!refit::finite_f(B.vectors[e])) return SPRAY_RT_ERR_ARG;
    if (tubes && B.color_field)
      for (size_t e = 0; e < np; ++e)
        if (!refit::finite_f(B.color_field[e])) return SPRAY_RT_ERR_ARG;
  }
  for (size_t e = 0; e < 3 * S.nseeds; ++e)
    if (!refit::finite_f(S.seeds[e])) return SPRAY_RT_ERR_ARG;
  return SPRAY_RT_OK;
}

// The lines of a validated set; emit false: the counts alone.  bc: the colour
// map (nullptr: color).
void lines_host(const spray_rt_blockfield& F, const spray_rt_block_color* bc, float cscale,
                uint32_t color, bool emit, HostBlockLines* L) {
  std::vector<bstrm::BlockRec> tab(size_t(F.nblocks));
  for (int b = 0; b < F.nblocks; ++b)
    tab[size_t(b)] = rec_of(F.blocks[b], F.blocks[b].vectors, bc ? F.blocks[b].color_field : nullptr);
  std::vector<bstrm::BlockBox> box(tab.size());
  for (size_t b = 0; b < tab.size(); ++b) box[b] = bstrm::box_of(tab[b]);
  const bstrm::Blocks S = {tab.data(), box.data(), uint32_t(F.nblocks)};
  const float msq = F.min_speed * F.min_speed;
  const bool do_back = F.direction != SPRAY_RT_STREAM_FORWARD;
  const bool do_fwd = F.direction != SPRAY_RT_STREAM_BACKWARD;
  auto trace = [&](const float* seed, const bstrm::Cur& cur0, const strm::Cell& c0, float h,
                   Half* H) {
    float p[3] = {seed[0], seed[1], seed[2]};
    bstrm::Cur cur = cur0;
    strm::Cell c = c0;
    strm::Frame fr = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    for (int steps = 0; steps <= F.max_steps; ++steps) {
      float k1[3], pn[3];
      strm::Cell cn;
      strm::sample_vector(cur.G, c, k1);
      strm::frame_at(k1, msq, steps == 0, &fr);
      H->P.insert(H->P.end(), p, p + 3);
      H->N.insert(H->N.end(), fr.N, fr.N + 3);
      H->T.insert(H->T.end(), fr.T, fr.T + 3);
      H->blk.push_back(cur.b);
      H->col.push_back(bc ? bc->table_rgb[cmap::bin(
                                strm::sample_scalar(cur.G, tab[cur.b].cfield, c), bc->lo, cscale,
                                bc->ntable)]
                          : color);
      const int r = bstrm::advance(S, &cur, p, k1, h, msq, steps, F.max_steps, pn, &cn);
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
    L->blk.push_back(H.blk[k]);
  };
  for (size_t s = 0; s < F.nseeds; ++s) {
    const float* seed = F.seeds + 3 * s;
    if (emit) L->off.push_back(uint32_t(L->npoints));
    bstrm::Cur cur0;
    strm::Cell c0;
    uint64_t m = 0;
    if (!bstrm::locate_any(S, seed, &cur0, &c0)) {
      if (emit) {
        L->info.push_back(0);
        L->info.push_back(uint32_t(strm::kEndSeed) | (uint32_t(strm::kEndSeed) << 8));
      }
    } else if (!emit) {
      int end;
      m = 1;
      if (do_back)
        m += uint64_t(bstrm::trace_count(S, cur0, seed, c0, -F.step, msq, F.max_steps, &end));
      if (do_fwd)
        m += uint64_t(bstrm::trace_count(S, cur0, seed, c0, F.step, msq, F.max_steps, &end));
    } else {
      Half B, W;
      if (do_back) trace(seed, cur0, c0, -F.step, &B);
      if (do_fwd) trace(seed, cur0, c0, F.step, &W);
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

struct BlockCall {
  HeadTake<StreamJob> jobs;  // in the context's block-stream arena
  HeadTake<BlockJob> bjobs;
  HeadTake<StreamOut> outs;
  HeadTake<BlockOut> bouts;
  size_t m_outs = 0;  // the mark in front of outs
  uint32_t max_blocks = 0;
  bool staged = false;  // some array came from host memory
  std::vector<StreamRec> rec;
  std::vector<uint64_t> nverts, nfaces;  // of the tubes (zero without tubes)
};

// Validates the sets (their tubes and colour maps where given), runs the check
// pass, the count pass and the scan and reads the sizes (the host read).
// Messages name the set, its slot where slots is given, and the block at fault.
int block_count(spray_rt_ctx* c, const char* what, int n, const spray_rt_blockfield* sets,
                const spray_rt_tube* tubes, const spray_rt_block_color* bcolors, const int* slots,
                BlockCall* call) {
  const size_t nj = size_t(n);
  auto name = [&](int i, int block) {
    char buf[128], blk[32] = "";
    if (block >= 0) snprintf(blk, sizeof(blk), ", block %d", block);
    if (slots)
      snprintf(buf, sizeof(buf), "%s (set %d, slot %d%s)", what, i, slots[i], blk);
    else
      snprintf(buf, sizeof(buf), "%s (set %d%s)", what, i, blk);
    return std::string(buf);
  };
  if (n > 65535) return fail(c, SPRAY_RT_ERR_LIMIT, "%s: more than 65535 sets in one call", what);
  std::vector<float> cscale(nj, 0.0f);
  size_t total_blocks = 0;
  for (int i = 0; i < n; ++i) {
    int code, block;
    const spray_rt_block_color* bc = bcolors ? &bcolors[i] : nullptr;
    if (const char* why = set_error(sets[i], has_table(bc), &code, &block))
      return fail(c, code, "%s: %s", name(i, block).c_str(), why);
    if (tubes) {
      if (const char* why = tube_error(tubes[i]))
        return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", name(i, -1).c_str(), why);
      if (const char* why = color_error(sets[i], bc, &cscale[size_t(i)]))
        return fail(c, SPRAY_RT_ERR_ARG, "%s: %s", name(i, -1).c_str(), why);
    }
    total_blocks += size_t(sets[i].nblocks);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- layout: tables (mirrored in pinned memory), then arrays and scratch ----
  JobArena& A = c->bstream;
  A.reset();
  call->jobs = A.take_head<StreamJob>(nj);
  call->bjobs = A.take_head<BlockJob>(nj);
  const auto t_blocks = A.take_head<bstrm::BlockRec>(total_blocks);
  const auto t_boxes = A.take_head<bstrm::BlockBox>(total_blocks);
  const size_t m_status = A.mark();
  const auto t_status = A.take_head<uint32_t>(2 * nj);
  const size_t m_rec = A.mark();
  const auto t_rec = A.take_head<StreamRec>(nj);
  call->m_outs = A.mark();
  call->outs = A.take_head<StreamOut>(nj);
  call->bouts = A.take_head<BlockOut>(nj);
  struct Scratch {
    Take<uint32_t> word;
    Take<uint64_t> loc;
    Take<uint4> bbase;
    uint32_t nlanes, nblocks;
    size_t item0, block0;  // the set's first staged item and first block record
  };
  std::vector<Scratch> sk(nj);
  // per set: its seeds and colour table, then each block's vectors and colour
  // field; host ones staged inside the arena
  Stager stage;
  size_t block0 = 0;
  for (int i = 0; i < n; ++i) {
    const spray_rt_blockfield& f = sets[i];
    Scratch& k = sk[size_t(i)];
    k.nlanes = uint32_t(f.nseeds) * (f.direction == SPRAY_RT_STREAM_BOTH ? 2u : 1u);
    k.nblocks = (k.nlanes + strm::kBlock - 1) / strm::kBlock;
    k.item0 = stage.items.size();
    k.block0 = block0;
    block0 += size_t(f.nblocks);
    const bool colored = tubes && f.blocks[0].color_field;
    stage.place(f.seeds, 3 * f.nseeds * sizeof(float), &A);
    stage.place(colored ? bcolors[i].table_rgb : nullptr,
                colored ? size_t(bcolors[i].ntable) * sizeof(uint32_t) : 0, &A);
    for (int b = 0; b < f.nblocks; ++b) {
      const size_t np = block_points(f.blocks[b]);
      stage.place(f.blocks[b].vectors, 3 * np * sizeof(float), &A);
      stage.place(colored ? f.blocks[b].color_field : nullptr, np * sizeof(float), &A);
    }
    k.word = A.take<uint32_t>(k.nlanes);
    k.loc = A.take<uint64_t>(k.nlanes);
    k.bbase = A.take<uint4>(k.nblocks);
    call->max_blocks = std::max(call->max_blocks, k.nblocks);
  }
  call->staged = stage.any;
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(A.d, s));
  StreamJob* jobs = A.host(call->jobs);
  BlockJob* bjobs = A.host(call->bjobs);
  bstrm::BlockRec* h_blocks = A.host(t_blocks);
  bstrm::BlockBox* h_boxes = A.host(t_boxes);
  uint32_t* h_status = A.host(t_status);
  for (int i = 0; i < n; ++i) {
    const spray_rt_blockfield& f = sets[i];
    const Scratch& k = sk[size_t(i)];
    const bool colored = tubes && f.blocks[0].color_field;
    StreamJob J{};  // the grid members stay empty: the blocks are in the second table
    J.seeds = stage.dev<float>(k.item0);
    if (colored) {
      J.ctable = stage.dev<uint32_t>(k.item0 + 1);
      J.ntable = bcolors[i].ntable;
      J.clo = bcolors[i].lo;
      J.cscale = cscale[size_t(i)];
    }
    J.word = A.dev(k.word);
    J.loc = A.dev(k.loc);
    J.bbase = A.dev(k.bbase);
    J.rec = A.dev(t_rec) + i;
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
    for (int b = 0; b < f.nblocks; ++b) {
      bstrm::BlockRec& R = h_blocks[k.block0 + size_t(b)];
      R = rec_of(f.blocks[b], stage.dev<float>(k.item0 + 2 + 2 * size_t(b)),
                 stage.dev<float>(k.item0 + 3 + 2 * size_t(b)));
      h_boxes[k.block0 + size_t(b)] = bstrm::box_of(R);
    }
    BlockJob B{};
    B.blocks = A.dev(t_blocks) + k.block0;
    B.boxes = A.dev(t_boxes) + k.block0;
    B.nvb = uint32_t(f.nblocks);
    B.has_color = colored ? 1u : 0u;
    bjobs[i] = B;
    h_status[2 * i] = 0;
    h_status[2 * i + 1] = bstrm::kNoBlock;
  }
  HIPCHK(c, arena_copy(A, 0, m_rec, true, s));
  const StreamJob* d_jobs = A.dev(call->jobs);
  const BlockJob* d_bjobs = A.dev(call->bjobs);
  HIPCHK(c, launch_block_stream_check(s, d_jobs, d_bjobs, n, A.dev(t_status)));
  HIPCHK(c, launch_block_stream_count(s, d_jobs, d_bjobs, n, call->max_blocks));
  HIPCHK(c, launch_stream_scan(s, d_jobs, n));
  HIPCHK(c, arena_copy(A, m_status, call->m_outs, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the sizes: the call's host read
  const StreamRec* h_rec = A.host(t_rec);
  call->rec.assign(h_rec, h_rec + n);
  call->nverts.assign(nj, 0);
  call->nfaces.assign(nj, 0);
  for (int i = 0; i < n; ++i) {
    const uint32_t st = h_status[2 * i];
    const int bad_block = h_status[2 * i + 1] == bstrm::kNoBlock ? -1 : int(h_status[2 * i + 1]);
    // the block named is the lowest with a bad sample of either kind
    if ((st & strm::kBadVector) && (st & strm::kBadColor))
      return fail(c, SPRAY_RT_ERR_ARG,
                  "%s: non-finite vector sample or sample of the colour field (the lowest such block)",
                  name(i, bad_block).c_str());
    if (st & strm::kBadVector)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite vector sample", name(i, bad_block).c_str());
    if (st & strm::kBadColor)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite sample of the colour field",
                  name(i, bad_block).c_str());
    if (st & strm::kBadSeed)
      return fail(c, SPRAY_RT_ERR_ARG, "%s: non-finite seed coordinate", name(i, -1).c_str());
    if (tubes) {
      const uint64_t ns = uint64_t(tubes[i].nsides);
      call->nverts[size_t(i)] = h_rec[i].tube_points * ns + 2 * h_rec[i].tube_lines;
      call->nfaces[size_t(i)] = 2 * ns * h_rec[i].tube_points;
    }
    if (const char* why =
            totals_error(h_rec[i].npoints, call->nverts[size_t(i)], call->nfaces[size_t(i)]))
      return fail(c, SPRAY_RT_ERR_LIMIT, "%s: %s", name(i, -1).c_str(), why);
  }
  return SPRAY_RT_OK;
}

// The integrate pass of a counted call into outs[n] and bouts[n], and with
// tubes the expansion.
int block_emit(spray_rt_ctx* c, int n, const BlockCall& call, const std::vector<StreamOut>& outs,
               const std::vector<BlockOut>& bouts, bool tubes) {
  hipStream_t s = stream_of(c);
  const JobArena& A = c->bstream;
  std::memcpy(A.host(call.outs), outs.data(), size_t(n) * sizeof(StreamOut));
  std::memcpy(A.host(call.bouts), bouts.data(), size_t(n) * sizeof(BlockOut));
  HIPCHK(c, arena_copy(A, call.m_outs, A.head, true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  HIPCHK(c, launch_block_stream_integrate(s, A.dev(call.jobs), A.dev(call.bjobs),
                                          A.dev(call.outs), A.dev(call.bouts), n,
                                          call.max_blocks, tubes));
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

int spray_rt_block_streamlines_host(const spray_rt_blockfield* set, size_t* npoints,
                                    float* points_out, uint32_t* line_offsets_out,
                                    uint32_t* line_info_out, uint32_t* point_blocks_out) {
  if (!set) return SPRAY_RT_ERR_ARG;
  if (npoints) *npoints = 0;
  float cscale;
  if (const int r = validate_host(*set, nullptr, false, &cscale)) return r;
  HostBlockLines L;
  const bool emit = points_out || line_offsets_out || line_info_out || point_blocks_out;
  lines_host(*set, nullptr, 0.0f, 0u, emit, &L);
  if (npoints) *npoints = size_t(L.npoints);
  if (totals_error(L.npoints, 0, 0)) return SPRAY_RT_ERR_LIMIT;
  if (points_out) std::memcpy(points_out, L.P.data(), L.P.size() * sizeof(float));
  if (line_offsets_out)
    std::memcpy(line_offsets_out, L.off.data(), L.off.size() * sizeof(uint32_t));
  if (line_info_out) std::memcpy(line_info_out, L.info.data(), L.info.size() * sizeof(uint32_t));
  if (point_blocks_out)
    std::memcpy(point_blocks_out, L.blk.data(), L.blk.size() * sizeof(uint32_t));
  return SPRAY_RT_OK;
}

int spray_rt_block_stream_tubes_host(const spray_rt_blockfield* set, const spray_rt_tube* tube,
                                     const spray_rt_block_color* bcolor, size_t* nverts,
                                     size_t* nfaces, float* verts_out, float* vnormals_out,
                                     uint32_t* colors_out, uint32_t* faces_out) {
  if (!set || !tube) return SPRAY_RT_ERR_ARG;
  if (nverts) *nverts = 0;
  if (nfaces) *nfaces = 0;
  if (tube_error(*tube)) return SPRAY_RT_ERR_ARG;
  float cscale;
  if (const int r = validate_host(*set, bcolor, true, &cscale)) return r;
  HostBlockLines L;
  const bool emit = verts_out || vnormals_out || colors_out || faces_out;
  lines_host(*set, set->blocks[0].color_field ? bcolor : nullptr, cscale, tube->color_rgb, emit, &L);
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
int spray_rt_block_stream_phase_times(spray_rt_ctx_t c, double out_ms[3]) {
  if (!c || !out_ms) return SPRAY_RT_ERR_ARG;
  for (int k = 0; k < 3; ++k) out_ms[k] = c->bstream_ms[k];
  return SPRAY_RT_OK;
}

int spray_rt_block_streamlines(spray_rt_ctx_t c, int n, const spray_rt_blockfield* sets,
                               float* const* points, uint32_t* const* line_offsets,
                               uint32_t* const* line_info, uint32_t* const* point_blocks,
                               const size_t* cap_points, size_t* npoints_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && !sets) || (n && (points || point_blocks) && !cap_points))
    return fail(c, SPRAY_RT_ERR_ARG, "block_streamlines: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const auto t0 = Clock::now();
  c->bstream_ms[0] = c->bstream_ms[1] = c->bstream_ms[2] = 0.0;
  BlockCall call;
  const int r = block_count(c, "block_streamlines", n, sets, nullptr, nullptr, nullptr, &call);
  c->bstream_ms[0] = ms_since(t0);
  if (r) return r;
  for (int i = 0; npoints_out && i < n; ++i) npoints_out[i] = size_t(call.rec[size_t(i)].npoints);
  if (!points && !line_offsets && !line_info && !point_blocks) return SPRAY_RT_OK;
  const auto t1 = Clock::now();
  std::vector<StreamOut> outs(size_t(n), StreamOut{});
  std::vector<BlockOut> bouts(size_t(n), BlockOut{});
  for (int i = 0; i < n; ++i) {
    const StreamRec& rec = call.rec[size_t(i)];
    StreamOut& O = outs[size_t(i)];
    O.points = points ? points[i] : nullptr;
    O.line_offsets = line_offsets ? line_offsets[i] : nullptr;
    O.line_info = line_info ? line_info[i] : nullptr;
    bouts[size_t(i)].point_blocks = point_blocks ? point_blocks[i] : nullptr;
    const bool per_point = O.points || bouts[size_t(i)].point_blocks;
    if (per_point && rec.npoints > cap_points[i])
      return fail(c, SPRAY_RT_ERR_LIMIT,
                  "block_streamlines (set %d): %llu points do not fit the buffers", i,
                  static_cast<unsigned long long>(rec.npoints));
    O.cap_points = per_point ? rec.npoints : 0;
  }
  const int e = block_emit(c, n, call, outs, bouts, false);
  if (e) return e;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->bstream_ms[1] = ms_since(t1);
  return SPRAY_RT_OK;
}

int spray_rt_block_stream_tubes(spray_rt_ctx_t c, int n, const spray_rt_blockfield* sets,
                                const spray_rt_tube* tubes, const spray_rt_block_color* bcolors,
                                float* const* verts, float* const* vnormals,
                                uint32_t* const* colors, uint32_t* const* faces,
                                const size_t* cap_verts, const size_t* cap_faces,
                                size_t* nverts_out, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!sets || !tubes)) || (n && (verts || vnormals || colors) && !cap_verts) ||
      (n && faces && !cap_faces))
    return fail(c, SPRAY_RT_ERR_ARG, "block_stream_tubes: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const auto t0 = Clock::now();
  c->bstream_ms[0] = c->bstream_ms[1] = c->bstream_ms[2] = 0.0;
  BlockCall call;
  const int r = block_count(c, "block_stream_tubes", n, sets, tubes, bcolors, nullptr, &call);
  c->bstream_ms[0] = ms_since(t0);
  if (r) return r;
  for (int i = 0; i < n; ++i) {
    if (nverts_out) nverts_out[i] = size_t(call.nverts[size_t(i)]);
    if (nfaces_out) nfaces_out[i] = size_t(call.nfaces[size_t(i)]);
  }
  if (!verts && !vnormals && !colors && !faces) return SPRAY_RT_OK;
  const auto t1 = Clock::now();
  const size_t nj = size_t(n);
  std::vector<StreamOut> outs(nj, StreamOut{});
  const std::vector<BlockOut> bouts(nj, BlockOut{});
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
                  "block_stream_tubes (set %d): %llu vertices and %llu faces do not fit the buffers",
                  i, static_cast<unsigned long long>(nv), static_cast<unsigned long long>(nf));
    O.cap_verts = per_vertex ? nv : 0;
    O.cap_faces = O.faces ? nf : 0;
    any = any || per_vertex || O.faces;
  }
  if (!any) return SPRAY_RT_OK;
  Layout M;  // of d_isomesh
  std::vector<TubeScratch> ts(nj);
  for (size_t k = 0; k < nj; ++k) take_tube_scratch(&M, sets[k].nseeds, call.rec[k], &ts[k]);
  const int g = ensure(c, &c->d_isomesh, &c->isomesh_cap, std::max<size_t>(M.used, 256));
  if (g) return g;
  for (size_t k = 0; k < nj; ++k) set_tube_scratch(&outs[k], ts[k], c->d_isomesh, call.rec[k]);
  const int e = block_emit(c, n, call, outs, bouts, true);
  if (e) return e;
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->bstream_ms[1] = ms_since(t1);
  return SPRAY_RT_OK;
}

int spray_rt_domains_block_stream_tubes(spray_rt_ctx_t c, int n, const int* slots,
                                        const spray_rt_blockfield* sets,
                                        const spray_rt_tube* tubes,
                                        const spray_rt_block_color* bcolors, int with_normals,
                                        float* d_bounds, size_t* nfaces_out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!slots || !sets || !tubes)))
    return fail(c, SPRAY_RT_ERR_ARG, "block_stream_tubes: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const size_t nj = size_t(n);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] > 1 << 20)
      return fail(c, SPRAY_RT_ERR_ARG, "block_stream_tubes (set %d): bad slot %d", i, slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail(c, SPRAY_RT_ERR_ARG, "block_stream_tubes (set %d): slot %d listed twice", i,
                    slots[i]);
  }
  const auto t0 = Clock::now();
  c->bstream_ms[0] = c->bstream_ms[1] = c->bstream_ms[2] = 0.0;
  BlockCall call;
  int r = block_count(c, "block_stream_tubes", n, sets, tubes, bcolors, slots, &call);
  c->bstream_ms[0] = ms_since(t0);
  if (r) return r;

  // ---- the lines' scratch and the meshes: context scratch, sized by the counts ----
  const auto t1 = Clock::now();
  Layout M;  // of d_isomesh
  std::vector<StreamOut> outs(nj, StreamOut{});
  const std::vector<BlockOut> bouts(nj, BlockOut{});
  std::vector<TubeScratch> ts(nj);
  std::vector<Take<float>> t_verts(nj), t_normals(nj);
  std::vector<Take<uint32_t>> t_colors(nj), t_faces(nj);
  std::vector<size_t> nv(nj), nf(nj);
  for (size_t k = 0; k < nj; ++k) {
    take_tube_scratch(&M, sets[k].nseeds, call.rec[k], &ts[k]);
    outs[k].cap_verts = nv[k] = size_t(call.nverts[k]);
    outs[k].cap_faces = nf[k] = size_t(call.nfaces[k]);
    t_verts[k] = M.take<float>(3 * nv[k]);
    if (with_normals) t_normals[k] = M.take<float>(3 * nv[k]);
    if (tubes[k].has_color || sets[k].blocks[0].color_field) t_colors[k] = M.take<uint32_t>(nv[k]);
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
  r = block_emit(c, n, call, outs, bouts, true);
  if (r) return r;
  c->bstream_ms[1] = ms_since(t1);

  // ---- the slots: the device build on the expanded arrays ----
  const auto t2 = Clock::now();
  int job = -1;  // the build names the slot; name the set as well
  r = domains_build(c, n, slots, pv.data(), nv.data(), pf.data(), nf.data(), pc.data(), pn.data(),
                    d_bounds, &job);
  if (r) {
    const std::string msg = c->err;
    if (job >= 0)
      return fail(c, r, "block_stream_tubes (set %d, slot %d): %s", job, slots[job], msg.c_str());
    return fail(c, r, "block_stream_tubes: %s", msg.c_str());
  }
  if (nfaces_out)
    for (size_t k = 0; k < nj; ++k) nfaces_out[k] = nf[k];
  if (call.staged) HIPCHK(c, hipStreamSynchronize(stream_of(c)));  // host arrays: done on return
  c->bstream_ms[2] = ms_since(t2);
  return SPRAY_RT_OK;
}
#endif  // SPRAY_RT_STREAM_HOST_ONLY

}  // extern "C"
