// refit.cpp -- moving geometry: spray_rt_domains_refit, its host-only
// restatement spray_rt_bvh_refit_host, spray_rt_slot_export and
// spray_rt_slot_sah (include/spray_rt.h).
//
// A refit keeps the topology a slot was built with and recomputes, on the
// device, every number that depends on the vertex positions: BVH2 child
// boxes, triangle records, the quantization grid, the QNode4 child boxes,
// the normals.  It runs in two phases around ONE host read of the call's
// status words, so a rejected call leaves every slot as it was (DESIGN.md,
// "Moving geometry").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bvh_build.h"
#include "refit_common.h"
#include "refit_kernels.h"
#include "rt_common.h"
#include "rt_ctx.h"
#include "spray_rt.h"

using namespace spray_rt;
using namespace spray_rt::detail;

namespace {
const float* side_lo(const BvhNode& n, int side) { return side ? n.r_lo : n.l_lo; }
const float* side_hi(const BvhNode& n, int side) { return side ? n.r_hi : n.l_hi; }
}  // namespace

namespace spray_rt {
// The refit of a built image on the host, step for step what the kernels do.
// built: the canonical BVH2 (padded boxes; only its refs, prims and empty
// boxes are read), q0 / qsrc: its QNode4 collapse and the children's sources.
// Returns the refit::kBad* bits.
uint32_t refit_host(const BvhImage& built, const std::vector<QNode4>& q0,
                    const std::vector<int32_t>& qsrc, const float* verts, const uint32_t* faces,
                    std::vector<BvhNode>* nodes, std::vector<float>* tris, QGrid* grid,
                    std::vector<QNode4>* qn, std::vector<BvhNode>* exact) {
  uint32_t status = 0;
  const size_t nn = built.nodes.size(), nt = built.prims.size();
  tris->resize(12 * nt);
  for (size_t i = 0; i < nt; ++i) {
    const uint32_t* f = faces + 3 * size_t(built.prims[i]);
    if (!refit::tri_record(verts + 3 * size_t(f[0]), verts + 3 * size_t(f[1]),
                           verts + 3 * size_t(f[2]), &(*tris)[12 * i]))
      status |= refit::kBadVertex;
  }
  // exact boxes bottom up: children follow their parent in the layout
  std::vector<BvhNode> ex = built.nodes;
  for (size_t i = nn; i-- > 0;) {
    const BvhNode& old = built.nodes[i];
    for (int side = 0; side < 2; ++side) {
      float* lo = side ? ex[i].r_lo : ex[i].l_lo;
      float* hi = side ? ex[i].r_hi : ex[i].l_hi;
      if (refit::empty_box(side_lo(old, side))) continue;  // the never-hit box: kept
      for (int j = 0; j < 3; ++j) {
        lo[j] = refit::pos_inf();
        hi[j] = -refit::pos_inf();
      }
      const int32_t ref = side ? old.right : old.left;
      if (ref < 0) {
        uint32_t first, count;
        refit::leaf_range(ref, &first, &count);
        for (uint32_t t = first; t < first + count && t < nt; ++t) {
          const uint32_t* f = faces + 3 * size_t(built.prims[t]);
          for (int k = 0; k < 3; ++k) {
            const float* p = verts + 3 * size_t(f[k]);
            refit::grow(lo, hi, p, p);
          }
        }
      } else {
        const BvhNode& c = ex[size_t(ref)];
        if (!refit::empty_box(c.l_lo)) refit::grow(lo, hi, c.l_lo, c.l_hi);
        if (!refit::empty_box(c.r_lo)) refit::grow(lo, hi, c.r_lo, c.r_hi);
      }
    }
  }
  if (exact) *exact = ex;
  *nodes = ex;
  for (BvhNode& n : *nodes) {
    refit::pad_box(n.l_lo, n.l_hi);
    refit::pad_box(n.r_lo, n.r_hi);
  }
  // grid over the padded non-empty boxes
  float lo[3] = {refit::pos_inf(), refit::pos_inf(), refit::pos_inf()};
  float hi[3] = {-refit::pos_inf(), -refit::pos_inf(), -refit::pos_inf()};
  bool grid_ok = true;
  for (const BvhNode& n : *nodes)
    for (int side = 0; side < 2; ++side) {
      if (refit::empty_box(side_lo(n, side))) continue;
      for (int j = 0; j < 3; ++j)
        if (!refit::finite_f(side_lo(n, side)[j]) || !refit::finite_f(side_hi(n, side)[j]))
          grid_ok = false;
      refit::grow(lo, hi, side_lo(n, side), side_hi(n, side));
    }
  *grid = QGrid{};
  const bool any = lo[0] <= hi[0];
  for (int j = 0; j < 3; ++j)
    grid_ok = refit::qgrid_axis(lo[j], hi[j], any, &grid->base[j], &grid->scale[j]) && grid_ok;
  if (!grid_ok) status |= refit::kBadGrid;
  // QNode4 child boxes on the new grid, child refs kept
  *qn = q0;
  for (size_t i = 0; i < qsrc.size(); ++i) {
    uint16_t* q = (*qn)[i >> 2].q + 6 * (i & 3);
    for (int j = 0; j < 6; ++j) q[j] = 0xFFFF;
    const int32_t src = qsrc[i];
    if (src < 0) continue;
    const BvhNode& n = (*nodes)[size_t(src >> 1)];
    for (int j = 0; j < 3; ++j)
      if (!(grid->scale[j] > 0.f) ||
          !refit::quant_axis(grid->base[j], grid->scale[j], side_lo(n, src & 1)[j],
                             side_hi(n, src & 1)[j], &q[j], &q[3 + j]))
        status |= refit::kBadQuant;
  }
  return status;
}

}  // namespace spray_rt

namespace {

int check_slot(spray_rt_ctx* c, int slot) {
  if (slot < 0 || size_t(slot) >= c->slots.size() || !c->slots[size_t(slot)].dmem)
    return fail(c, SPRAY_RT_ERR_ARG, "slot %d is not loaded", slot);
  return SPRAY_RT_OK;
}

}  // namespace

extern "C" {

int spray_rt_bvh_refit_host(const float* verts0, const float* new_verts, size_t nverts,
                            const uint32_t* faces, size_t nfaces, void* nodes_out,
                            float* tris_out, float grid_out[6], void* qnodes4_out) {
  if ((nverts && (!verts0 || !new_verts)) || (nfaces && !faces)) return SPRAY_RT_ERR_ARG;
  BvhImage img;
  if (!build_bvh(verts0, nverts, faces, nfaces, &img)) return SPRAY_RT_ERR_ARG;
  QGrid grid{};
  std::vector<QNode4> q0, qn;
  std::vector<int32_t> qsrc;
  int bound = 0;
  if (!img.nodes.empty() && !quantize_nodes4(img.nodes, &grid, &q0, &bound, &qsrc))
    return SPRAY_RT_ERR_LIMIT;
  std::vector<BvhNode> nodes;
  std::vector<float> tris;
  const uint32_t st = refit_host(img, q0, qsrc, new_verts, faces, &nodes, &tris, &grid, &qn);
  if (st & refit::kBadVertex) return SPRAY_RT_ERR_ARG;
  if (st) return SPRAY_RT_ERR_LIMIT;
  if (nodes_out) std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(BvhNode));
  if (tris_out) std::memcpy(tris_out, tris.data(), tris.size() * sizeof(float));
  if (grid_out) {
    std::memcpy(grid_out, grid.base, 12);
    std::memcpy(grid_out + 3, grid.scale, 12);
  }
  if (qnodes4_out) std::memcpy(qnodes4_out, qn.data(), qn.size() * sizeof(QNode4));
  return SPRAY_RT_OK;
}

int spray_rt_domains_refit(spray_rt_ctx_t c, int n, const int* slots, const float* const* verts,
                           const float* const* vnormals, float* d_bounds) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (n < 0 || (n && (!slots || !verts))) return fail(c, SPRAY_RT_ERR_ARG, "refit: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  // ---- host-side validation: nothing is enqueued before it passes ----
  for (int i = 0; i < n; ++i) {
    const int r = check_slot(c, slots[i]);
    if (r) return r;
    const SlotHost& sh = c->slots[size_t(slots[i])];
    if (sh.refit.offset == SIZE_MAX)
      return fail(c, SPRAY_RT_ERR_ARG, "refit: slot %d carries no refit metadata", slots[i]);
    if (sh.desc.nverts && !verts[i])
      return fail(c, SPRAY_RT_ERR_ARG, "refit: null vertex array for slot %d", slots[i]);
    if (sh.desc.normals && sh.desc.nverts && (!vnormals || !vnormals[i]))
      return fail(c, SPRAY_RT_ERR_ARG,
                  "refit: slot %d was uploaded with normals and the call brings none", slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail(c, SPRAY_RT_ERR_ARG, "refit: slot %d listed twice", slots[i]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- caller arrays: device pointers as they are, host arrays staged ----
  Stager stage;  // items 2 i, 2 i + 1: job i's vertices and normals
  for (int i = 0; i < n; ++i) {
    const SlotHost& sh = c->slots[size_t(slots[i])];
    const size_t vb = 3 * size_t(sh.desc.nverts) * sizeof(float);
    stage.place(vb ? verts[i] : nullptr, vb);
    stage.place(vb && sh.desc.normals ? vnormals[i] : nullptr, vb);
  }
  if (stage.any)
    if (const int r = ensure(c, &c->d_stage, &c->stage_cap, stage.own.used)) return r;

  // ---- layout: job table, status (mirrored in pinned memory), grids, scratch image ----
  const size_t nj = size_t(n);
  JobArena& A = c->refit;
  A.reset();
  const auto t_jobs = A.take_head<RefitJob>(nj);
  const size_t m_status = A.mark();
  const auto t_status = A.take_head<uint32_t>(nj);
  const auto t_grid = A.take<QGrid>(nj);
  std::vector<Take<BvhNode>> t_nodes(nj);
  std::vector<Take<QNode4>> t_q(nj);
  for (int i = 0; i < n; ++i) {
    const SlotHost& sh = c->slots[size_t(slots[i])];
    t_nodes[size_t(i)] = A.take<BvhNode>(sh.desc.nnodes);
    t_q[size_t(i)] = A.take<QNode4>(sh.refit.nq);
  }
  if (const int r = arena_reserve(c, &A)) return r;
  HIPCHK(c, stage.copy(c->d_stage, s));
  RefitJob* jobs = A.host(t_jobs);
  uint32_t* h_status = A.host(t_status);
  uint32_t* d_status = A.dev(t_status);
  uint32_t max_tris = 0, max_nodes = 0, max_verts = 0, max_nq = 0;
  uint32_t level_max[kRefitLevels] = {};
  int height = 0;
  for (int i = 0; i < n; ++i) {
    const SlotHost& sh = c->slots[size_t(slots[i])];
    // the slot's async upload, if one is pending, comes first
    if (sh.ready) HIPCHK(c, hipStreamWaitEvent(s, sh.ready, 0));
    char* base = static_cast<char*>(sh.dmem);
    const size_t nn = sh.desc.nnodes;
    RefitJob J{};
    J.nodes = const_cast<BvhNode*>(sh.desc.nodes);
    J.tris = const_cast<float*>(sh.desc.tris);
    J.prims = sh.desc.prims;
    J.faces = sh.desc.faces;
    J.normals = const_cast<float*>(sh.desc.normals);
    J.order = reinterpret_cast<const uint32_t*>(base + sh.refit.offset);
    J.level = reinterpret_cast<const uint32_t*>(base + sh.refit.o_level(nn));
    J.qsrc = reinterpret_cast<const int32_t*>(base + sh.refit.o_qsrc(nn));
    J.verts = stage.dev<float>(2 * size_t(i));
    J.vnormals = stage.dev<float>(2 * size_t(i) + 1);
    J.s_nodes = A.dev(t_nodes[size_t(i)]);
    J.s_q = A.dev(t_q[size_t(i)]);
    J.s_grid = A.dev(t_grid) + i;
    J.nnodes = sh.desc.nnodes;
    J.ntris = sh.desc.ntris;
    J.nverts = sh.desc.nverts;
    J.nq = sh.refit.nq;
    J.height = sh.refit.height;
    jobs[i] = J;
    h_status[i] = 0;
    max_tris = std::max(max_tris, J.ntris);
    max_nodes = std::max(max_nodes, J.nnodes);
    max_verts = std::max(max_verts, J.nverts);
    max_nq = std::max(max_nq, J.nq);
    height = std::max(height, sh.refit.height);
    for (int lv = 1; lv <= sh.refit.height; ++lv)
      level_max[lv] = std::max(level_max[lv], sh.refit.level[lv + 1] - sh.refit.level[lv]);
  }
  HIPCHK(c, arena_copy(A, 0, A.head, true, s));
  const RefitJob* d_jobs = A.dev(t_jobs);

  // ---- phase 1: fit and quantize into scratch, flag what cannot be done ----
  HIPCHK(c, launch_refit_check_tris(s, d_jobs, n, max_tris, d_status));
  for (int lv = 1; lv <= height; ++lv)
    HIPCHK(c, launch_refit_fit_level(s, d_jobs, n, lv, level_max[lv]));
  HIPCHK(c, launch_refit_grid(s, d_jobs, n, d_status));
  HIPCHK(c, launch_refit_quant(s, d_jobs, n, max_nq, d_status));
  HIPCHK(c, arena_copy(A, m_status, m_status + nj * sizeof(uint32_t), false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the call's one host read
  for (int i = 0; i < n; ++i) {
    if (!h_status[i]) continue;
    if (h_status[i] & refit::kBadVertex)
      return fail(c, SPRAY_RT_ERR_ARG,
                  "refit (slot %d): non-finite coordinate of a referenced vertex", slots[i]);
    return fail(c, SPRAY_RT_ERR_LIMIT,
                "refit (slot %d): boxes beyond the range of the quantized node grid", slots[i]);
  }

  // ---- phase 2: commit ----
  HIPCHK(c, launch_refit_commit(s, d_jobs, n, max_nodes, max_tris, max_verts, d_bounds));
  if (stage.any) HIPCHK(c, hipStreamSynchronize(s));  // host arrays: done on return
  return SPRAY_RT_OK;
}

int spray_rt_slot_export(spray_rt_ctx_t c, int slot, int what, void* out, size_t cap_bytes,
                         size_t* nbytes) {
  if (!c) return SPRAY_RT_ERR_ARG;
  const int r = check_slot(c, slot);
  if (r) return r;
  const SlotHost& sh = c->slots[size_t(slot)];
  const bool q = sh.refit.offset != SIZE_MAX && sh.refit.nq > 0;
  const char* nodes = reinterpret_cast<const char*>(sh.desc.nodes);
  const void* src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case SPRAY_RT_SLOT_NODES:
      src = sh.desc.nodes;
      bytes = size_t(sh.desc.nnodes) * sizeof(BvhNode);
      break;
    case SPRAY_RT_SLOT_TRIS:
      src = sh.desc.tris;
      bytes = size_t(sh.desc.ntris) * 12 * sizeof(float);
      break;
    case SPRAY_RT_SLOT_PRIMS:
      src = sh.desc.prims;
      bytes = size_t(sh.desc.ntris) * sizeof(uint32_t);
      break;
    case SPRAY_RT_SLOT_QNODES4:
      bytes = q ? size_t(sh.refit.nq) * sizeof(QNode4) : 0;
      src = q ? nodes - 64 - bytes : nullptr;
      break;
    case SPRAY_RT_SLOT_QGRID:
      bytes = q ? 6 * sizeof(float) : 0;
      src = q ? nodes - sizeof(QGrid) : nullptr;
      break;
    case SPRAY_RT_SLOT_NORMALS:
      src = sh.desc.normals;
      bytes = sh.desc.normals ? 3 * size_t(sh.desc.nverts) * sizeof(float) : 0;
      break;
    case SPRAY_RT_SLOT_COLORS:
      src = sh.desc.colors;
      bytes = sh.desc.colors ? size_t(sh.desc.nverts) * sizeof(uint32_t) : 0;
      break;
    case SPRAY_RT_SLOT_FACES:
      src = sh.desc.faces;
      bytes = 3 * size_t(sh.desc.ntris) * sizeof(uint32_t);
      break;
    default:
      return fail(c, SPRAY_RT_ERR_ARG, "slot export: unknown array %d", what);
  }
  if (nbytes) *nbytes = bytes;
  if (!out || !bytes) return SPRAY_RT_OK;
  if (cap_bytes < bytes)
    return fail(c, SPRAY_RT_ERR_ARG, "slot export: %zu bytes do not fit %zu", bytes, cap_bytes);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(stream_of(c)));
  if (sh.ready) HIPCHK(c, hipEventSynchronize(sh.ready));
  if (what == SPRAY_RT_SLOT_QGRID) {
    QGrid g{};
    HIPCHK(c, hipMemcpy(&g, src, sizeof(QGrid), hipMemcpyDeviceToHost));
    std::memcpy(out, g.base, 12);
    std::memcpy(static_cast<char*>(out) + 12, g.scale, 12);
    return SPRAY_RT_OK;
  }
  HIPCHK(c, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
  if (what == SPRAY_RT_SLOT_QNODES4) {  // stored backwards in front of the nodes
    QNode4* qn = static_cast<QNode4*>(out);
    std::reverse(qn, qn + sh.refit.nq);
  }
  return SPRAY_RT_OK;
}

int spray_rt_slot_sah(spray_rt_ctx_t c, int slot, double* out) {
  if (!c) return SPRAY_RT_ERR_ARG;
  if (!out) return fail(c, SPRAY_RT_ERR_ARG, "slot sah: null output");
  const int r = check_slot(c, slot);
  if (r) return r;
  const SlotHost& sh = c->slots[size_t(slot)];
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);
  if (sh.ready) HIPCHK(c, hipStreamWaitEvent(s, sh.ready, 0));
  if (!c->d_sah) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_sah), 256));
  HIPCHK(c, launch_slot_sah(s, sh.desc.nodes, sh.desc.nnodes, c->d_sah));
  HIPCHK(c, hipMemcpyAsync(out, c->d_sah, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return SPRAY_RT_OK;
}

}  // extern "C"
