// build_common.h -- the arithmetic and the decisions of the device BVH build
// (spray_rt_domains_build), shared by the host restatement (build_device.cpp)
// and the gfx950 kernels (build_kernels.hip).
//
// The tree is a function of the mesh alone: triangles sorted by a total key
// (30-bit Morton code of the box centroid, then the face index), ranges over
// the sorted order split at the highest differing code bit, nodes and QNode4s
// numbered level by level in range order.  Boxes, records, the grid and the
// quantization are refit_common.h's.  Both translation units are compiled
// with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "refit_common.h"
#include "rt_common.h"

namespace spray_rt {
namespace build {

// further status bits of one slot of a build call (refit::kBad* are 1, 2, 4)
constexpr uint32_t kBadFace = 8;  // a face index >= nverts

constexpr int kCodeBits = 10;  // Morton cells per axis: 2^10
// BFS levels of inner nodes: depths 0 .. kMaxDepth - 1
constexpr int kBuildLevels = kMaxDepth + 1;

// The box of one triangle, vertices grown in face order, and its centroid
// (lo + hi) * 0.5f (the builder's set_prim).
SPRAY_HD void tri_centroid(const float* a, const float* b, const float* c, float cen[3]) {
  float lo[3] = {a[0], a[1], a[2]}, hi[3] = {a[0], a[1], a[2]};
  refit::grow(lo, hi, b, b);
  refit::grow(lo, hi, c, c);
  for (int j = 0; j < 3; ++j) cen[j] = (lo[j] + hi[j]) * 0.5f;
}

// Cell of centroid coordinate x on an axis of centroid bounds [lo, hi]:
// ((x - lo) * (1024 / (hi - lo))) truncated, clamped to [0, 1023]; an axis
// without extent (or a NaN) maps to cell 0.
SPRAY_HD uint32_t code_cell(float x, float lo, float hi) {
  const float ext = hi - lo;
  if (!(ext > 0.0f)) return 0;
  const float s = float(1 << kCodeBits) / ext;
  const float t = (x - lo) * s;
  if (!(t > 0.0f)) return 0;
  if (t >= float((1 << kCodeBits) - 1)) return (1u << kCodeBits) - 1;
  return uint32_t(t);
}

// 10 bits -> every third bit
SPRAY_HD uint32_t spread3(uint32_t v) {
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// 30-bit Morton code, x in the highest bit of each triple
SPRAY_HD uint32_t morton30(uint32_t cx, uint32_t cy, uint32_t cz) {
  return (spread3(cx) << 2) | (spread3(cy) << 1) | spread3(cz);
}

// The sort key of face `face`: total and unique.  cb = centroid bounds lo.xyz hi.xyz.
SPRAY_HD uint64_t sort_key(const float cen[3], const float cb[6], uint32_t face) {
  const uint32_t code = morton30(code_cell(cen[0], cb[0], cb[3]), code_cell(cen[1], cb[1], cb[4]),
                                 code_cell(cen[2], cb[2], cb[5]));
  return (uint64_t(code) << 32) | face;
}

SPRAY_HD int ceil_log2_u32(uint32_t x) {
  int l = 0;
  while ((uint32_t(1) << l) < x) ++l;
  return l;
}

// The host builder's depth rule (bvh_build.cpp): a range of n triangles at
// depth `depth` splits at its median once a balanced tree below it is all
// that still fits kMaxDepth.
SPRAY_HD bool depth_forces_median(uint32_t n, int depth) {
  return depth + ceil_log2_u32((n + kLeafMax - 1) / kLeafMax) >= kMaxDepth;
}

// Split of range [begin, end) (more than kLeafMax triangles) of the sorted
// keys: the first triangle whose code has the highest bit set in which the
// first and the last code differ; the median begin + n / 2 when the codes are
// equal or the depth rule asks for it (*forced).  begin < mid < end.
SPRAY_HD uint32_t split_range(const uint64_t* keys, uint32_t begin, uint32_t end, int depth,
                              bool* forced) {
  const uint32_t n = end - begin;
  const uint32_t first = uint32_t(keys[begin] >> 32), last = uint32_t(keys[end - 1] >> 32);
  *forced = depth_forces_median(n, depth);
  if (*forced || first == last) return begin + n / 2;
  int bit = 31;
  while (!(((first ^ last) >> bit) & 1u)) --bit;
  // codes are ascending and agree above `bit`: the first one with it set
  uint32_t lo = begin, hi = end - 1;  // keys[lo]: bit clear, keys[hi]: bit set
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint32_t(keys[mid] >> 32) >> bit) & 1u)
      hi = mid;
    else
      lo = mid;
  }
  return hi;
}

SPRAY_HD int32_t leaf_ref(uint32_t first, uint32_t count) {
  return ~int32_t((first << 2) | (count - 1));
}

// ---- the 4-wide collapse: Collapse::emit's greedy rule for one QNode4 ----
struct Cand {
  int32_t ref;  // BVH2 child ref
  int32_t src;  // BVH2 (node << 1 | side) whose box the child quantizes
};

SPRAY_HD const float* side_lo(const BvhNode& n, int side) { return side ? n.r_lo : n.l_lo; }
SPRAY_HD const float* side_hi(const BvhNode& n, int side) { return side ? n.r_hi : n.l_hi; }
SPRAY_HD int32_t side_ref(const BvhNode& n, int side) { return side ? n.right : n.left; }

// non-empty children of BVH2 node `node`, left first
SPRAY_HD int node_children(const BvhNode* nodes, int32_t node, Cand out[2]) {
  const BvhNode& n = nodes[node];
  int k = 0;
  for (int side = 0; side < 2; ++side)
    if (!refit::empty_box(side_lo(n, side))) out[k++] = Cand{side_ref(n, side), node * 2 + side};
  return k;
}

// half area of a candidate's padded box (nodes hold the exact boxes)
SPRAY_HD float cand_area(const BvhNode* nodes, const Cand& c) {
  const BvhNode& n = nodes[c.src >> 1];
  float lo[3], hi[3];
  for (int j = 0; j < 3; ++j) {
    lo[j] = side_lo(n, c.src & 1)[j];
    hi[j] = side_hi(n, c.src & 1)[j];
  }
  refit::pad_box(lo, hi);
  return refit::half_area(lo, hi);
}

// Children of the QNode4 that stands for BVH2 node `node`, entered with `pend`
// walk-stack entries pending: the node's two children, the inner one of the
// largest area replaced by its own two while fewer than four are held and
// pend + size - 1 + (largest height among them) stays within kQ4Stack.
// nodes: exact boxes and refs; hgt: BVH2 height per node (leaves 0).
SPRAY_HD int collapse_node(const BvhNode* nodes, const uint8_t* hgt, int32_t node, int pend,
                           Cand cs[4]) {
  Cand two[2];
  int k = node_children(nodes, node, two);
  for (int c = 0; c < k; ++c) cs[c] = two[c];
  for (;;) {
    if (k >= 4) break;
    int pick = -1;
    float best = -1.f;
    for (int c = 0; c < k; ++c) {
      if (cs[c].ref < 0) continue;
      Cand gc[2];
      const int ng = node_children(nodes, cs[c].ref, gc);
      int hmax = 0;
      for (int m = 0; m < k; ++m)
        if (m != c && cs[m].ref >= 0 && int(hgt[cs[m].ref]) > hmax) hmax = hgt[cs[m].ref];
      for (int g = 0; g < ng; ++g)
        if (gc[g].ref >= 0 && int(hgt[gc[g].ref]) > hmax) hmax = hgt[gc[g].ref];
      const int size = k - 1 + ng;
      if (size > 4 || pend + size - 1 + hmax > kQ4Stack) continue;
      const float a = cand_area(nodes, cs[c]);
      if (a > best) {
        best = a;
        pick = c;
      }
    }
    if (pick < 0) break;
    Cand gc[2];
    const int ng = node_children(nodes, cs[pick].ref, gc);
    // erase `pick`, insert its children in its place
    for (int m = k - 1; m > pick; --m) cs[m + ng - 1] = cs[m];
    for (int g = 0; g < ng; ++g) cs[pick + g] = gc[g];
    k += ng - 1;
  }
  return k;
}

}  // namespace build
}  // namespace spray_rt
