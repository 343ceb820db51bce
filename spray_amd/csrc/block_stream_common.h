// block_stream_common.h -- the rule of the multi-block streamline filter
// (spray_rt_block_streamlines, spray_rt_block_stream_tubes,
// spray_rt_domains_block_stream_tubes), stated once and shared by the host
// restatement (block_streamlines.cpp) and the gfx950 kernels
// (block_stream_kernels.hip).  Everything of stream_common.h stands: sample,
// step, end reasons, frame, tube.  Only "which grid" differs: a half-line
// carries a current block; a point is sampled there if it is inside it, else in
// the lowest-indexed block it is inside, which becomes the current one
// (include/spray_rt.h).
#pragma once

#include "stream_common.h"

namespace spray_rt {
namespace bstrm {

using strm::Cell;
using strm::Grid;

// status bits of one set of a call beyond strm::kBad*; the lowest block with a
// bad sample goes to a second word (kNoBlock: none)
constexpr uint32_t kNoBlock = 0xFFFFFFFFu;
constexpr int kMaxBlocks = 65535;

// One block of a set (device table), read when a half-line enters the block.
struct alignas(16) BlockRec {
  float origin[3], spacing[3];
  int32_t n[3];
  uint32_t pad0;
  const float* vectors;  // [nz][ny][nx][3]
  const float* cfield;   // [nz][ny][nx], nullptr: none
  uint32_t pad1[2];
};
static_assert(sizeof(BlockRec) == 64, "block records are one 64-B line each");

// The inside test of one block without its divisions, for the miss path
// (device table beside the records): with d = p - origin per axis, p is inside
// exactly when lo <= d <= hi, lo the smallest and hi the largest float whose
// quotient by the spacing lies in [0, float(n - 1)].  x -> x / spacing (rounded)
// never decreases, so the floats with a quotient in range are those between
// the two (box_of finds them by bisection).
struct alignas(16) BlockBox {
  float origin[3], lo[3], hi[3];
  uint32_t pad[3];
};
static_assert(sizeof(BlockBox) == 48, "three boxes to nine 16-B loads");

// A set's blocks and a half-line's current one: its index and its grid.
struct Blocks {
  const BlockRec* tab;
  const BlockBox* box;
  uint32_t n;
};
struct Cur {
  uint32_t b;
  Grid G;
};

SPRAY_HD Grid grid_of(const BlockRec& R) {
  Grid G;
  G.vectors = R.vectors;
  for (int a = 0; a < 3; ++a) {
    G.n[a] = R.n[a];
    G.origin[a] = R.origin[a];
    G.spacing[a] = R.spacing[a];
  }
  return G;
}

// Floats in their order as integers (-0 below +0), and back.
inline uint32_t float_key(float x) {
  const uint32_t b = strm::bits(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float key_float(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// The box of a block (host): 32 halvings per bound between a float that
// passes (-0 and 0: their quotient is zero) and one that fails (an infinity).
inline BlockBox box_of(const BlockRec& R) {
  BlockBox B{};
  for (int a = 0; a < 3; ++a) {
    const float s = R.spacing[a], top = float(R.n[a] - 1);
    B.origin[a] = R.origin[a];
    uint32_t bad = float_key(-strm::pos_inf()), ok = float_key(-0.0f);
    for (int it = 0; it < 32 && ok - bad > 1; ++it) {
      const uint32_t mid = bad + (ok - bad) / 2;
      if (key_float(mid) / s >= 0.0f) ok = mid; else bad = mid;
    }
    B.lo[a] = key_float(ok);
    ok = float_key(0.0f), bad = float_key(strm::pos_inf());
    for (int it = 0; it < 32 && bad - ok > 1; ++it) {
      const uint32_t mid = ok + (bad - ok) / 2;
      if (key_float(mid) / s <= top) ok = mid; else bad = mid;
    }
    B.hi[a] = key_float(ok);
  }
  return B;
}

// strm::locate's inside test alone, by the box.
SPRAY_HD bool inside(const BlockBox& B, const float p[3]) {
  bool in = true;
  for (int a = 0; a < 3; ++a) {
    const float d = p[a] - B.origin[a];
    in = in && d >= B.lo[a] && d <= B.hi[a];
  }
  return in;
}

// The miss path: the lowest-indexed block p is inside becomes the current one.
SPRAY_HD bool locate_any(const Blocks& S, const float p[3], Cur* cur, Cell* c) {
  for (uint32_t k = 0; k < S.n; ++k) {
    if (!inside(S.box[k], p)) continue;
    cur->b = k;
    cur->G = grid_of(S.tab[k]);
    return strm::locate(cur->G, p, c);
  }
  return false;
}

// Whether p is inside some block; *c = its cell in the block it is sampled in.
SPRAY_HD bool locate(const Blocks& S, const float p[3], Cur* cur, Cell* c) {
  if (strm::locate(cur->G, p, c)) return true;
  return locate_any(S, p, cur, c);
}

// strm::rk4 over blocks: the current block follows q2, q3, q4, p' in that order.
SPRAY_HD int rk4(const Blocks& S, Cur* cur, const float p[3], const float k1[3], float h,
                 float pn[3], Cell* cn) {
  const float hh = 0.5f * h, h6 = h / 6.0f;
  float q[3], k2[3], k3[3], k4[3];
  Cell c;
  for (int a = 0; a < 3; ++a) q[a] = p[a] + hh * k1[a];
  if (!locate(S, q, cur, &c)) return strm::kEndGrid;
  strm::sample_vector(cur->G, c, k2);
  for (int a = 0; a < 3; ++a) q[a] = p[a] + hh * k2[a];
  if (!locate(S, q, cur, &c)) return strm::kEndGrid;
  strm::sample_vector(cur->G, c, k3);
  for (int a = 0; a < 3; ++a) q[a] = p[a] + h * k3[a];
  if (!locate(S, q, cur, &c)) return strm::kEndGrid;
  strm::sample_vector(cur->G, c, k4);
  for (int a = 0; a < 3; ++a)
    pn[a] = p[a] + h6 * (((k1[a] + 2.0f * k2[a]) + 2.0f * k3[a]) + k4[a]);
  return locate(S, pn, cur, cn) ? strm::kTaken : strm::kEndGrid;
}

// strm::advance over blocks.
SPRAY_HD int advance(const Blocks& S, Cur* cur, const float p[3], const float k1[3], float h,
                     float msq, int steps, int max_steps, float pn[3], Cell* cn) {
  float d;
  if (!strm::usable(k1, msq, &d)) return strm::kEndSpeed;
  const int r = rk4(S, cur, p, k1, h, pn, cn);
  if (r != strm::kTaken) return r;
  if (strm::bits(pn[0]) == strm::bits(p[0]) && strm::bits(pn[1]) == strm::bits(p[1]) &&
      strm::bits(pn[2]) == strm::bits(p[2]))
    return strm::kEndSpeed;
  if (steps >= max_steps) return strm::kEndSteps;
  return strm::kTaken;
}

// The steps a half-line takes from a seed located in cur0 (its cell c0).
SPRAY_HD int trace_count(const Blocks& S, const Cur& cur0, const float seed[3], const Cell& c0,
                         float h, float msq, int max_steps, int* end) {
  float p[3] = {seed[0], seed[1], seed[2]};
  Cur cur = cur0;
  Cell c = c0;
  *end = strm::kEndSteps;
  int steps = 0;
  for (; steps <= max_steps; ++steps) {  // the step after max_steps is never taken
    float k1[3], pn[3];
    Cell cn;
    strm::sample_vector(cur.G, c, k1);
    const int r = advance(S, &cur, p, k1, h, msq, steps, max_steps, pn, &cn);
    if (r != strm::kTaken) {
      *end = r;
      break;
    }
    for (int a = 0; a < 3; ++a) p[a] = pn[a];
    c = cn;
  }
  return steps;
}

}  // namespace bstrm
}  // namespace spray_rt
