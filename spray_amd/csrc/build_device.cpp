// build_device.cpp -- geometry that changes topology: spray_rt_domains_build
// and its host-only restatement spray_rt_bvh_build_device_host
// (include/spray_rt.h).
//
// A build brings new triangle lists into slots without the host builder: the
// tree is made on the device (build_kernels.hip) from arrays that may already
// be in HBM, in context scratch sized for the worst case; the host reads one
// record per slot, allocates the exact images and a commit copies them in.  A
// rejected call has written no slot memory ("Changing topology").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "build_common.h"
#include "build_kernels.h"
#include "bvh_build.h"
#include "refit_common.h"
#include "refit_kernels.h"
#include "rt_common.h"
#include "rt_ctx.h"
#include "spray_rt.h"

using namespace spray_rt;
using namespace spray_rt::detail;

namespace {

struct HostBuild {
  BvhImage img;  // nodes padded, tris, prims, depth
  QGrid grid{};
  std::vector<QNode4> qn;
  int stack_bound = 0, nmedian = 0;
};

// The device build on the host, step for step what the kernels do.
int build_host(const float* verts, size_t nverts, const uint32_t* faces, size_t nfaces,
               HostBuild* out) {
  if (nfaces >= (size_t(1) << 29)) return SPRAY_RT_ERR_ARG;
  for (size_t i = 0; i < 3 * nfaces; ++i)
    if (faces[i] >= nverts) return SPRAY_RT_ERR_ARG;
  *out = HostBuild{};
  if (nfaces == 0) return SPRAY_RT_OK;
  const uint32_t nt = uint32_t(nfaces);
  // check + centroid bounds
  float cb[6] = {refit::pos_inf(), refit::pos_inf(), refit::pos_inf(),
                 -refit::pos_inf(), -refit::pos_inf(), -refit::pos_inf()};
  std::vector<float> cen(3 * nfaces);
  for (uint32_t i = 0; i < nt; ++i) {
    const uint32_t* f = faces + 3 * size_t(i);
    const float *a = verts + 3 * size_t(f[0]), *b = verts + 3 * size_t(f[1]),
                *c = verts + 3 * size_t(f[2]);
    float r[12];
    if (!refit::tri_record(a, b, c, r)) return SPRAY_RT_ERR_ARG;
    build::tri_centroid(a, b, c, &cen[3 * size_t(i)]);
    refit::grow(cb, cb + 3, &cen[3 * size_t(i)], &cen[3 * size_t(i)]);
  }
  // keys, sorted
  std::vector<uint64_t> keys(nfaces);
  for (uint32_t i = 0; i < nt; ++i) keys[i] = build::sort_key(&cen[3 * size_t(i)], cb, i);
  std::sort(keys.begin(), keys.end());
  BvhImage topo;
  topo.prims.resize(nfaces);
  for (uint32_t i = 0; i < nt; ++i) topo.prims[i] = uint32_t(keys[i]);
  // ranges level by level, nodes numbered in range order
  struct Range {
    uint32_t b, e;
  };
  std::vector<Range> range;
  std::vector<uint32_t> lbase;  // first node of each BFS level, then the node count
  auto blank = [] {
    BvhNode n;
    std::memset(&n, 0, sizeof(n));
    return n;
  };
  if (nt <= uint32_t(kLeafMax)) {
    BvhNode n = blank();
    for (int j = 0; j < 3; ++j) n.r_lo[j] = n.r_hi[j] = refit::pos_inf();
    n.left = build::leaf_ref(0, nt);
    n.right = ~int32_t(0);
    topo.nodes.push_back(n);
    lbase = {0, 1};
  } else {
    range.push_back({0, nt});
    lbase = {0, 1};
    for (int L = 0;; ++L) {
      const uint32_t base = lbase[size_t(L)], next_base = lbase[size_t(L) + 1];
      if (base == next_base) {
        lbase.pop_back();
        break;
      }
      if (L >= kMaxDepth) return SPRAY_RT_ERR_LIMIT;  // more than 4 * 2^kMaxDepth triangles
      uint32_t pos = next_base;
      topo.nodes.resize(next_base, blank());
      for (uint32_t k = base; k < next_base; ++k) {
        const Range r = range[k];
        bool forced;
        const uint32_t m = build::split_range(keys.data(), r.b, r.e, L, &forced);
        if (forced) ++out->nmedian;
        const bool fl = m - r.b > uint32_t(kLeafMax), fr = r.e - m > uint32_t(kLeafMax);
        BvhNode& n = topo.nodes[k];
        n.left = fl ? int32_t(pos) : build::leaf_ref(r.b, m - r.b);
        if (fl) {
          range.push_back({r.b, m});
          ++pos;
        }
        n.right = fr ? int32_t(pos) : build::leaf_ref(m, r.e - m);
        if (fr) {
          range.push_back({m, r.e});
          ++pos;
        }
      }
      lbase.push_back(pos);
    }
  }
  const size_t nn = topo.nodes.size();
  const int nlev = int(lbase.size()) - 1;
  topo.depth = nlev;
  // heights: children have larger indices
  std::vector<uint8_t> hgt(nn, 0);
  for (size_t i = nn; i-- > 0;) {
    const BvhNode& n = topo.nodes[i];
    const int hl = n.left >= 0 ? hgt[size_t(n.left)] : 0, hr = n.right >= 0 ? hgt[size_t(n.right)] : 0;
    hgt[i] = uint8_t(1 + std::max(hl, hr));
  }
  // fit, grid (the refit's), then the collapse over the exact boxes
  std::vector<BvhNode> nodes, exact;
  std::vector<float> tris;
  std::vector<QNode4> q0, qn;
  std::vector<int32_t> qsrc;
  uint32_t st = refit_host(topo, q0, qsrc, verts, faces, &nodes, &tris, &out->grid, &qn, &exact);
  if (st) return st & refit::kBadVertex ? SPRAY_RT_ERR_ARG : SPRAY_RT_ERR_LIMIT;
  struct QEntry {
    int32_t node;
    int pend;
  };
  std::vector<QEntry> qlist{{0, 0}};
  for (size_t base = 0, cnt = 1; cnt > 0;) {
    const size_t next_base = base + cnt;
    size_t pos = next_base;
    q0.resize(next_base);
    qsrc.resize(4 * next_base);
    for (size_t k = base; k < next_base; ++k) {
      const QEntry e = qlist[k];
      build::Cand cs[4];
      const int nc = build::collapse_node(exact.data(), hgt.data(), e.node, e.pend, cs);
      const int p2 = e.pend + (nc > 0 ? nc - 1 : 0);
      out->stack_bound = std::max(out->stack_bound, p2);
      QNode4 q{};
      for (int c = 0; c < 4; ++c) {
        int32_t ref = kNoChild, src = -1;
        if (c < nc) {
          ref = cs[c].ref;
          src = cs[c].src;
          if (ref >= 0) {
            qlist.push_back({ref, p2});
            ref = int32_t(pos++);
          }
        }
        q.child[c] = ref;
        qsrc[4 * k + size_t(c)] = src;
      }
      q0[k] = q;
    }
    base = next_base;
    cnt = pos - next_base;
  }
  st = refit_host(topo, q0, qsrc, verts, faces, &nodes, &tris, &out->grid, &qn);
  if (st) return st & refit::kBadVertex ? SPRAY_RT_ERR_ARG : SPRAY_RT_ERR_LIMIT;
  out->img.nodes = std::move(nodes);
  out->img.tris = std::move(tris);
  out->img.prims = std::move(topo.prims);
  out->img.depth = topo.depth;
  out->qn = std::move(qn);
  return SPRAY_RT_OK;
}

}  // namespace

extern "C" {

int spray_rt_bvh_build_device_host(const float* verts, size_t nverts, const uint32_t* faces,
                                   size_t nfaces, size_t* nnodes, size_t* nq, int* depth,
                                   int* stack_bound, int* nmedian, void* nodes_out,
                                   float* tris_out, uint32_t* prims_out, float grid_out[6],
                                   void* qnodes4_out) {
  if ((nverts && !verts) || (nfaces && !faces)) return SPRAY_RT_ERR_ARG;
  HostBuild b;
  const int r = build_host(verts, nverts, faces, nfaces, &b);
  if (r) return r;
  if (nnodes) *nnodes = b.img.nodes.size();
  if (nq) *nq = b.qn.size();
  if (depth) *depth = b.img.depth;
  if (stack_bound) *stack_bound = b.stack_bound;
  if (nmedian) *nmedian = b.nmedian;
  if (nodes_out) std::memcpy(nodes_out, b.img.nodes.data(), b.img.nodes.size() * sizeof(BvhNode));
  if (tris_out) std::memcpy(tris_out, b.img.tris.data(), b.img.tris.size() * sizeof(float));
  if (prims_out) std::memcpy(prims_out, b.img.prims.data(), b.img.prims.size() * sizeof(uint32_t));
  if (grid_out) {
    std::memcpy(grid_out, b.grid.base, 12);
    std::memcpy(grid_out + 3, b.grid.scale, 12);
  }
  if (qnodes4_out) std::memcpy(qnodes4_out, b.qn.data(), b.qn.size() * sizeof(QNode4));
  return SPRAY_RT_OK;
}

}  // extern "C"

namespace spray_rt {
namespace detail {

int domains_build(spray_rt_ctx* c, int n, const int* slots, const float* const* verts,
                  const size_t* nverts, const uint32_t* const* faces, const size_t* nfaces,
                  const uint32_t* const* colors_rgb, const float* const* vnormals,
                  float* d_bounds, int* failed_job) {
  *failed_job = -1;
  // a failure that names job i's slot
  auto fail_job = [&](int i, int code, const char* fmt, auto... args) {
    *failed_job = i;
    return fail(c, code, fmt, args...);
  };
  if (n < 0 || (n && (!slots || !verts || !nverts || !faces || !nfaces)))
    return fail(c, SPRAY_RT_ERR_ARG, "build: null arguments");
  if (n == 0) return SPRAY_RT_OK;
  const size_t nj = size_t(n);
  // ---- host-side validation: nothing is enqueued before it passes ----
  uint64_t total_tris = 0;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] > 1 << 20)
      return fail_job(i, SPRAY_RT_ERR_ARG, "build: bad slot %d", slots[i]);
    for (int k = 0; k < i; ++k)
      if (slots[k] == slots[i])
        return fail_job(i, SPRAY_RT_ERR_ARG, "build: slot %d listed twice", slots[i]);
    if ((nverts[i] && !verts[i]) || (nfaces[i] && !faces[i]))
      return fail_job(i, SPRAY_RT_ERR_ARG, "build (slot %d): null mesh arrays", slots[i]);
    if (nfaces[i] >= (size_t(1) << 29))
      return fail_job(i, SPRAY_RT_ERR_ARG, "build (slot %d): mesh too large (>= 2^29 faces)", slots[i]);
    if (nverts[i] > UINT32_MAX)
      return fail_job(i, SPRAY_RT_ERR_ARG, "build (slot %d): too many vertices", slots[i]);
    if (nfaces[i] && !nverts[i])
      return fail_job(i, SPRAY_RT_ERR_ARG, "build (slot %d): face index out of range", slots[i]);
    total_tris += nfaces[i];
  }
  if (total_tris > UINT32_MAX)
    return fail(c, SPRAY_RT_ERR_LIMIT, "build: more than 2^32 - 1 triangles in one call");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream_of(c);

  // ---- caller arrays: device pointers as they are, host arrays staged ----
  Stager stage;  // items 4 i + kVerts .. kNormals: job i's arrays
  enum { kVerts, kFaces, kColors, kNormals };
  auto colors_of = [&](int i) { return stage.dev<uint32_t>(4 * size_t(i) + kColors); };
  auto normals_of = [&](int i) { return stage.dev<float>(4 * size_t(i) + kNormals); };
  for (int i = 0; i < n; ++i) {
    stage.place(verts[i], 3 * nverts[i] * sizeof(float));
    stage.place(faces[i], 3 * nfaces[i] * sizeof(uint32_t));
    stage.place(colors_rgb ? colors_rgb[i] : nullptr, nverts[i] * sizeof(uint32_t));
    stage.place(vnormals ? vnormals[i] : nullptr, 3 * nverts[i] * sizeof(float));
  }
  if (stage.any) {
    if (const int r = ensure(c, &c->d_stage, &c->stage_cap, stage.own.used)) return r;
    HIPCHK(c, stage.copy(c->d_stage, s));
  }

  // ---- layout of the scratch: tables (mirrored in pinned memory), then arrays ----
  JobArena& A = c->build;
  A.reset();
  const auto t_bjobs = A.take_head<BuildJob>(nj);
  const auto t_rjobs = A.take_head<RefitJob>(nj);
  const auto t_offsets = A.take_head<uint32_t>(nj + 1);
  // phase 1 uploads [0, m_rec) and reads back [m_status, m_jobs2); phase 2
  // uploads [m_jobs2, head)
  const size_t m_status = A.mark();
  const auto t_status = A.take_head<uint32_t>(nj);
  const size_t m_rec = A.mark();
  const auto t_rec = A.take_head<BuildRec>(nj);
  const size_t m_jobs2 = A.mark();
  const auto t_jobs2 = A.take_head<RefitJob>(nj);
  const auto t_copies = A.take_head<CopyJob>(6 * nj);
  const auto t_grid = A.take<QGrid>(nj);
  const auto t_keys = A.take<uint64_t>(size_t(total_tris));
  const auto t_sorted = A.take<uint64_t>(size_t(total_tris));
  struct Scratch {
    Take<float> part;
    Take<uint32_t> prims, order, level;
    Take<BvhNode> nodes;
    Take<QNode4> sq;
    Take<uint2> range, qlist;
    Take<uint8_t> hgt;
    Take<int32_t> qsrc;
    uint32_t cap;
  };
  std::vector<Scratch> sk(nj);
  uint32_t max_tris = 0, max_verts = 0, max_cap = 0;
  for (int i = 0; i < n; ++i) {
    Scratch& k = sk[size_t(i)];
    const uint32_t nt = uint32_t(nfaces[i]);
    k.cap = nt > 1 ? nt - 1 : 1;
    k.part = A.take<float>(size_t(kBuildParts) * 6);
    k.prims = A.take<uint32_t>(nt);
    A.take<char>(64 + size_t(k.cap) * sizeof(QNode4));  // QNode4s backwards, then 64 B
    k.nodes = A.take<BvhNode>(k.cap);                   // directly behind them
    k.sq = A.take<QNode4>(k.cap);
    k.range = A.take<uint2>(k.cap);
    k.qlist = A.take<uint2>(k.cap);
    k.hgt = A.take<uint8_t>(k.cap);
    k.order = A.take<uint32_t>(k.cap);
    k.level = A.take<uint32_t>(size_t(kRefitLevels));
    k.qsrc = A.take<int32_t>(4 * size_t(k.cap));
    max_tris = std::max(max_tris, nt);
    max_verts = std::max(max_verts, uint32_t(nverts[i]));
    max_cap = std::max(max_cap, k.cap);
  }
  if (const int r = arena_reserve(c, &A)) return r;
  BuildJob* bjobs = A.host(t_bjobs);
  RefitJob* rjobs = A.host(t_rjobs);
  uint32_t* offsets = A.host(t_offsets);
  uint32_t* h_status = A.host(t_status);
  const BuildRec* h_rec = A.host(t_rec);
  uint32_t first = 0;
  for (int i = 0; i < n; ++i) {
    const Scratch& k = sk[size_t(i)];
    BuildJob B{};
    B.verts = stage.dev<float>(4 * size_t(i) + kVerts);
    B.faces = stage.dev<uint32_t>(4 * size_t(i) + kFaces);
    B.keys = A.dev(t_keys) + first;
    B.sorted = A.dev(t_sorted) + first;
    B.part = A.dev(k.part);
    B.prims = A.dev(k.prims);
    B.nodes = A.dev(k.nodes);
    B.range = A.dev(k.range);
    B.hgt = A.dev(k.hgt);
    B.qlist = A.dev(k.qlist);
    B.order = A.dev(k.order);
    B.level = A.dev(k.level);
    B.qsrc = A.dev(k.qsrc);
    B.rec = A.dev(t_rec) + i;
    B.ntris = uint32_t(nfaces[i]);
    B.nverts = uint32_t(nverts[i]);
    B.cap = k.cap;
    bjobs[i] = B;
    // the refit's view of the scratch image: topology and fitted boxes share
    // one array (a node's refs are read before its boxes are written)
    RefitJob R{};
    R.nodes = B.nodes;
    R.prims = B.prims;
    R.faces = B.faces;
    R.order = B.order;
    R.level = B.level;
    R.qsrc = B.qsrc;
    R.verts = B.verts;
    R.s_nodes = B.nodes;
    R.s_q = A.dev(k.sq);
    R.s_grid = A.dev(t_grid) + i;
    R.ntris = B.ntris;
    R.nverts = B.nverts;
    rjobs[i] = R;  // nnodes, nq, height: the topology and collapse launches'
    offsets[i] = first;
    h_status[i] = 0;
    first += B.ntris;
    // an upload still in flight into a slot of the call comes first
    if (size_t(slots[i]) < c->slots.size() && c->slots[size_t(slots[i])].ready)
      HIPCHK(c, hipStreamWaitEvent(s, c->slots[size_t(slots[i])].ready, 0));
  }
  offsets[n] = first;
  HIPCHK(c, arena_copy(A, 0, m_rec, true, s));
  const BuildJob* d_bjobs = A.dev(t_bjobs);
  RefitJob* d_rjobs = A.dev(t_rjobs);
  uint32_t* d_status = A.dev(t_status);

  // ---- phase 1: the whole image into scratch ----
  HIPCHK(c, launch_build_check(s, d_bjobs, n, max_tris, d_status));
  HIPCHK(c, launch_build_keys(s, d_bjobs, n, max_tris, d_status));
  if (first) {
    const uint64_t* d_keys = A.dev(t_keys);
    uint64_t* d_sorted = A.dev(t_sorted);
    const uint32_t* d_offsets = A.dev(t_offsets);
    size_t tmp_bytes = 0;
    HIPCHK(c, build_sort(s, nullptr, &tmp_bytes, d_keys, d_sorted, first, n, d_offsets));
    const int r = ensure(c, &c->d_sort, &c->sort_cap, std::max<size_t>(tmp_bytes, 256));
    if (r) return r;
    HIPCHK(c, build_sort(s, c->d_sort, &tmp_bytes, d_keys, d_sorted, first, n, d_offsets));
  }
  HIPCHK(c, launch_build_topology(s, d_bjobs, d_rjobs, n, d_status));
  // a BFS level holds at most ntris / (kLeafMax + 1) inner ranges
  for (int lv = 1; lv <= kMaxDepth; ++lv)
    HIPCHK(c, launch_refit_fit_level(s, d_rjobs, n, lv, max_tris / (kLeafMax + 1) + 1));
  HIPCHK(c, launch_refit_grid(s, d_rjobs, n, d_status));
  HIPCHK(c, launch_build_collapse(s, d_bjobs, d_rjobs, n));
  HIPCHK(c, launch_refit_quant(s, d_rjobs, n, max_cap, d_status));
  HIPCHK(c, arena_copy(A, m_status, m_jobs2, false, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the records: the call's read of its own results
  for (int i = 0; i < n; ++i) {
    const uint32_t st = h_status[i];
    if (st & build::kBadFace)
      return fail_job(i, SPRAY_RT_ERR_ARG, "build (slot %d): face index out of range", slots[i]);
    if (st & refit::kBadVertex)
      return fail_job(i, SPRAY_RT_ERR_ARG,
                  "build (slot %d): non-finite coordinate of a referenced vertex", slots[i]);
    if (st)
      return fail_job(i, SPRAY_RT_ERR_LIMIT,
                  "build (slot %d): boxes beyond the range of the quantized node grid", slots[i]);
    if (h_rec[i].depth > kMaxDepth || h_rec[i].stack_bound > kQ4Stack ||
        h_rec[i].nnodes > sk[size_t(i)].cap || h_rec[i].nq > sk[size_t(i)].cap)
      return fail_job(i, SPRAY_RT_ERR_LIMIT, "build (slot %d): tree deeper than kMaxDepth", slots[i]);
  }

  // ---- the exact images: every allocation before any slot changes ----
  std::vector<SlotImage> img(nj);
  std::vector<void*> fresh(nj, nullptr);
  int maxslot = 0;
  for (int i = 0; i < n; ++i) maxslot = std::max(maxslot, slots[i]);
  for (int i = 0; i < n; ++i) {
    layout_slot_image(&img[size_t(i)], h_rec[i].nnodes, nfaces[i], nverts[i], h_rec[i].nq,
                      colors_of(i) != nullptr, normals_of(i) != nullptr, true);
    const size_t have = size_t(slots[i]) < c->slots.size() ? c->slots[size_t(slots[i])].bytes : 0;
    if (have >= img[size_t(i)].nbytes) continue;
    const hipError_t e = hipMalloc(&fresh[size_t(i)], img[size_t(i)].nbytes);
    if (e != hipSuccess) {
      for (void* p : fresh)
        if (p) (void)hipFree(p);
      return fail_job(i, SPRAY_RT_ERR_HIP, "build (slot %d): hipMalloc of %zu bytes: %s", slots[i],
                  img[size_t(i)].nbytes, hipGetErrorString(e));
    }
  }
  if (size_t(maxslot) >= c->slots.size()) c->slots.resize(size_t(maxslot) + 1);
  RefitJob* jobs2 = A.host(t_jobs2);
  CopyJob* copies = A.host(t_copies);
  int ncopies = 0;
  size_t max_words = 0;
  uint32_t max_nodes = 0;
  for (int i = 0; i < n; ++i) {
    SlotHost& sh = c->slots[size_t(slots[i])];
    const SlotImage& im = img[size_t(i)];
    const BuildRec& rec = h_rec[i];
    // the stream is idle (the read above); a pending upload of the old image too
    if (sh.ready) HIPCHK(c, hipEventSynchronize(sh.ready));
    if (fresh[size_t(i)]) {
      if (sh.dmem) HIPCHK(c, hipFree(sh.dmem));
      sh.dmem = fresh[size_t(i)];
      sh.bytes = im.nbytes;
      fresh[size_t(i)] = nullptr;
    }
    char* base = static_cast<char*>(sh.dmem);
    sh.desc = im.desc_at(base);
    sh.depth = rec.depth;
    sh.refit = im.refit;
    sh.refit.height = rec.height;
    std::memcpy(sh.refit.level, rec.level, sizeof(rec.level));
    const BuildJob& B = bjobs[i];
    RefitJob R = rjobs[i];
    R.nodes = const_cast<BvhNode*>(sh.desc.nodes);
    R.tris = const_cast<float*>(sh.desc.tris);
    R.normals = const_cast<float*>(sh.desc.normals);
    R.vnormals = normals_of(i);
    R.nnodes = rec.nnodes;
    R.nq = rec.nq;
    R.height = rec.height;
    jobs2[i] = R;
    max_nodes = std::max(max_nodes, rec.nnodes);
    auto copy = [&](const void* dst, const void* src, size_t nwords) {
      if (!nwords) return;
      copies[ncopies++] = CopyJob{static_cast<uint32_t*>(const_cast<void*>(dst)),
                                  static_cast<const uint32_t*>(src), nwords};
      max_words = std::max(max_words, nwords);
    };
    copy(sh.desc.prims, B.prims, B.ntris);
    copy(sh.desc.faces, B.faces, 3 * size_t(B.ntris));
    if (sh.desc.colors) copy(sh.desc.colors, colors_of(i), B.nverts);
    copy(base + sh.refit.offset, B.order, rec.nnodes);
    copy(base + sh.refit.o_level(rec.nnodes), B.level, size_t(kRefitLevels));
    copy(base + sh.refit.o_qsrc(rec.nnodes), B.qsrc, 4 * size_t(rec.nq));
  }
  c->slots_dirty = true;

  // ---- phase 2: commit ----
  HIPCHK(c, arena_copy(A, m_jobs2, A.head, true, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the pinned tables are free for the next call
  if (ncopies)
    HIPCHK(c, launch_build_copy(s, A.dev(t_copies), ncopies, max_words));
  HIPCHK(c, launch_refit_commit(s, A.dev(t_jobs2), n, max_nodes, max_tris, max_verts, d_bounds));
  if (stage.any) HIPCHK(c, hipStreamSynchronize(s));  // host arrays: done on return
  return SPRAY_RT_OK;
}

}  // namespace detail
}  // namespace spray_rt

extern "C" int spray_rt_domains_build(spray_rt_ctx_t c, int n, const int* slots,
                                      const float* const* verts, const size_t* nverts,
                                      const uint32_t* const* faces, const size_t* nfaces,
                                      const uint32_t* const* colors_rgb,
                                      const float* const* vnormals, float* d_bounds) {
  if (!c) return SPRAY_RT_ERR_ARG;
  int failed_job;
  return domains_build(c, n, slots, verts, nverts, faces, nfaces, colors_rgb, vnormals, d_bounds,
                       &failed_job);
}
