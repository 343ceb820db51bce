// rt_ctx.h -- the engine context behind spray_rt_ctx_t and the internal
// helpers shared by the C ABI translation units (rt_api.cpp, ooc.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "job_arena.h"
#include "rt_common.h"
#include "rt_kernels.h"
#include "spray_rt.h"

namespace spray_rt {
namespace detail {

// Refit metadata of a slot image (spray_rt_domains_refit), appended behind
// the image's arrays at byte `offset`, 256-B aligned:
//   order : uint32[nnodes]        nodes by height (bvh_build.h refit_order)
//   level : uint32[kRefitLevels]  first entry of each height
//   qsrc  : int32[4 * nq]         BVH2 (node << 1 | side) of each QNode4 child
// Images built without the quantized copy (OOC) carry none.
struct RefitInfo {
  size_t offset = SIZE_MAX;  // SIZE_MAX: absent
  uint32_t nq = 0;           // QNode4 count
  int height = 0;            // BVH2 height (levels of the bottom-up fit)
  uint32_t level[kRefitLevels] = {};
  size_t o_level(size_t nnodes) const { return offset + nnodes * 4; }
  size_t o_qsrc(size_t nnodes) const { return o_level(nnodes) + size_t(kRefitLevels) * 4; }
};

struct SlotHost {
  void* dmem = nullptr;  // one allocation: nodes|tris|prims|faces|colors|normals|refit metadata
  size_t bytes = 0;
  SlotDesc desc{};
  int depth = 0;
  RefitInfo refit;
  hipEvent_t ready = nullptr;  // async upload completion
  void* pinned = nullptr;      // staging for async uploads
  size_t pinned_bytes = 0;
};

}  // namespace detail
}  // namespace spray_rt

struct spray_rt_ctx {
  using SlotHost = spray_rt::detail::SlotHost;
  using SlotDesc = spray_rt::SlotDesc;
  using DomTrav = spray_rt::DomTrav;
  using BvhNode = spray_rt::BvhNode;

  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t user_stream = nullptr;
  bool user_stream_set = false;
  hipStream_t upload_stream = nullptr;
  std::vector<SlotHost> slots;
  SlotDesc* d_slots = nullptr;
  size_t d_slots_cap = 0;
  bool slots_dirty = true;
  // scene path
  int ndom = 0;
  float* d_boxes = nullptr;
  std::vector<float> h_boxes;  // the same boxes on the host (ooc drain views)
  int* d_dom2slot = nullptr;
  DomTrav* d_domtrav = nullptr;  // per-domain traversal descriptors
  int* d_owner = nullptr;        // in-situ domain -> rank map
  std::vector<int> h_owner;      // the same map on the host
  BvhNode* d_tlas = nullptr;  // top-level tree over the domain boxes
  int ntlas = 0;
  int tlas_depth = 0;
  int coherence = SPRAY_RT_RAYS_ADAPTIVE;
  std::vector<int> dom2slot;
  bool dom_dirty = true;
  // segment tables
  int* d_seg_slot = nullptr;
  size_t* d_seg_off = nullptr;
  size_t seg_cap = 0;
  // host-pointer staging
  void* d_stage = nullptr;
  size_t stage_cap = 0;
  void* d_stage2 = nullptr;
  size_t stage2_cap = 0;
  void* d_stage3 = nullptr;
  size_t stage3_cap = 0;
  // scratch of the batched slot calls (job_arena.h), one arena per call kind
  spray_rt::detail::JobArena refit;  // job table, status words | grids, scratch image
  spray_rt::detail::JobArena build;  // job tables, records | grids, keys, scratch images
  spray_rt::detail::JobArena iso;    // job tables, records | staged fields, per-point scratch
  spray_rt::detail::JobArena recolor;  // job table | staged colours (spray_rt_domains_recolor)
  hipEvent_t recolor_copied = nullptr;  // the last recolor's job table has left pinned memory
  spray_rt::detail::JobArena tet;  // job tables, records | staged mesh arrays, per-tet scratch
  void* d_tetinst = nullptr;       // tet isosurface: the per-instance scratch (keys, ids)
  size_t tetinst_cap = 0;
  // spray_rt_tet_set_timing / spray_rt_tet_phase_times: wall clock to host
  // read 1, to host read 2, to the end of the extraction's enqueue; the sort's
  // device time between the two events
  bool tet_timing = false;
  double tet_ms[4] = {};
  hipEvent_t tet_ev[2] = {nullptr, nullptr};
  spray_rt::detail::JobArena cell;  // job tables, records | staged mesh arrays, per-cell scratch
  void* d_celltets = nullptr;       // cell isosurface: the tets of the crossing cells
  size_t celltets_cap = 0;
  double cell_ms = 0.0;  // spray_rt_cell_phase_times: wall clock to the cell pass's host read
  spray_rt::detail::JobArena surf;  // job tables, records | staged mesh arrays, cell and point scratch
  void* d_surfinst = nullptr;       // cell surface: the per-face-instance scratch (keys, flags)
  size_t surfinst_cap = 0;
  double surf_ms[4] = {};  // spray_rt_cell_surface_phase_times, as tet_ms
  spray_rt::detail::JobArena clip;  // cell clip: the skin's job tables, records | staged arrays, scratch
  double clip_ms[6] = {};           // spray_rt_cell_clip_phase_times
  spray_rt::detail::JobArena stream;  // streamlines: job tables, records | staged arrays, per-lane scratch
  double stream_ms[3] = {};           // spray_rt_stream_phase_times
  spray_rt::detail::JobArena glyph;  // glyphs: job tables, counts | sphere tables, staged arrays, per-point scratch
  double glyph_ms[3] = {};           // spray_rt_glyph_phase_times
  spray_rt::detail::JobArena bstream;  // block streamlines: job and block tables, records | staged arrays, per-lane scratch
  double bstream_ms[3] = {};           // spray_rt_block_stream_phase_times
  double* d_sah = nullptr;  // spray_rt_slot_sah's result
  void* d_sort = nullptr;  // device build: temporary storage of the segmented sort
  size_t sort_cap = 0;
  void* d_isomesh = nullptr;  // isosurface into slots: the extracted meshes
  size_t isomesh_cap = 0;
  uint32_t* d_block_counts = nullptr;
  // work-queue heads of the persistent launches: [0, kHeadsBytes) zeroed by
  // each launch, [kHeadsBytes, 2 kHeadsBytes) zeroed by a frame's launch_clear
  uint32_t* d_heads = nullptr;
  void* d_sel = nullptr;        // selected indices + count + select scratch
  size_t sel_cap = 0;
  size_t block_cap = 0;
  // frame layer
  spray_rt_bsdf* d_bsdf = nullptr;  // per-domain BSDFs (Scene::getBsdf)
  int nbsdf = 0;
  bool bsdf_delta = false;  // some domain's BSDF is not diffuse
  void* d_frame = nullptr;  // render_tile path buffers
  size_t frame_cap = 0;
  unsigned long long* d_fstats = nullptr;  // render_tile totals (shade stats)
  // render_tiles' footprint-culled frame: the run table of the last
  // (camera, tiles, boxes) -- runs then first, frame.cpp -- and its key
  std::vector<float> ftab_key;
  void* d_ftab = nullptr;
  size_t ftab_cap = 0;
  uint32_t ftab_nruns = 0, ftab_npix = 0;
  size_t ftab_first_off = 0;  // bytes from d_ftab to the first[] array
  std::string err;
  std::mutex mu;  // lanes: the lazy table rebuild (prepare) runs under it
};

// A per-host-thread submission lane of a context (spray_rt_lane_*): its own
// stream, staging buffers and one-segment table, so concurrent threads never
// share mutable state; they only read the context's device tables.
struct spray_rt_lane {
  spray_rt_ctx* ctx = nullptr;
  hipStream_t stream = nullptr;
  void* d_buf = nullptr;
  size_t cap = 0;
  int* d_seg_slot = nullptr;
  size_t* d_seg_off = nullptr;
  std::string err;
};

namespace spray_rt {
namespace detail {

// Device image of one domain, packed on the host: [quantized nodes + grid]
// | BVH2 nodes | triangle records | leaf->face map | faces | colors |
// normals | refit metadata, 256-B aligned (the HBM slot layout of
// rt_common.h).  The quantized copy (QNode, in front of the nodes) and the
// refit metadata are built for scene slots only (quantized = true): the OOC
// drains do not read them, so its images stream without them.
struct SlotImage {
  std::vector<char> bytes;  // may be released once a pinned copy exists
  size_t nbytes = 0;        // the image's size (== bytes.size() while held)
  size_t o_nodes = 0, o_tris = 0, o_prims = 0, o_faces = 0;
  size_t o_colors = SIZE_MAX, o_normals = SIZE_MAX;  // SIZE_MAX: absent
  uint32_t nnodes = 0, ntris = 0, nverts = 0;
  int depth = 0;
  RefitInfo refit;
  // descriptor of the image once copied to device address base
  SlotDesc desc_at(const void* base) const;
};
// Offsets, counts and size of an image of these counts (bytes stays empty):
// the layout build_slot_image packs and the device build commits into.
void layout_slot_image(SlotImage* out, size_t nnodes, size_t nfaces, size_t nverts, size_t nq,
                       bool colors, bool normals, bool quantized);
// Builds the canonical BVH2 (bvh_build.h) and packs the image.  Returns
// nullptr on success, else what is wrong with the mesh (face index out of
// range, too many faces, non-finite vertex, coordinates beyond the range of
// the quantized node grid).
const char* build_slot_image(const float* verts, size_t nverts, const uint32_t* faces,
                      size_t nfaces, const uint32_t* colors, const float* normals,
                      SlotImage* out, bool quantized = true);

// Copies a packed image into cache slot `slot` (allocating it), after the
// queued work that may read the slot's previous image.  From pinned_src
// (pinned host memory holding img.bytes, kept alive by the caller) or with
// async = true: an async copy on the upload stream, ordered before the next
// query by the slot's ready event; else a synchronous copy.
int upload_slot_image(spray_rt_ctx* c, int slot, const SlotImage& img, const void* pinned_src,
                      bool async);

// Records a message in the context; returns code.
int fail(spray_rt_ctx* c, int code, const char* fmt, ...);
hipStream_t stream_of(spray_rt_ctx* c);
bool is_device_ptr(const void* p);
// grows *buf to at least bytes (device memory)
int ensure(spray_rt_ctx* c, void** buf, size_t* cap, size_t bytes);
// Storage of a laid-out arena: the device side through ensure, the pinned
// mirror of the head grow-only from 64 KiB.  A failed growth leaves the side
// it was growing empty.
int arena_reserve(spray_rt_ctx* c, JobArena* a);
void arena_release(JobArena* a);
// Async copy of the mirrored bytes [from, to) between marks: up = host to device.
inline hipError_t arena_copy(const JobArena& a, size_t from, size_t to, bool up, hipStream_t s) {
  assert(from <= to && to <= a.head);
  char *d = static_cast<char*>(a.d) + from, *h = static_cast<char*>(a.h) + from;
  return up ? hipMemcpyAsync(d, h, to - from, hipMemcpyHostToDevice, s)
            : hipMemcpyAsync(h, d, to - from, hipMemcpyDeviceToHost, s);
}

// Caller arrays of a batched call, in host or in device memory: place() each
// before anything is enqueued, make room, copy() once.  A call that staged
// anything synchronizes before it returns.
struct Stager {
  struct Item {
    const void* p;      // where the kernels read it (a host array: after copy())
    size_t bytes, off;  // off == SIZE_MAX: used where it is
  };
  std::vector<Item> items;  // every placed array, null and empty ones too
  Layout own;               // room for host arrays placed without a layout
  bool any = false;         // some array is staged
  // A host array gets a take of `in` (nullptr: own).
  void place(const void* p, size_t bytes, Layout* in = nullptr) {
    Item it{bytes ? p : nullptr, bytes, SIZE_MAX};  // an empty array reads as a null one
    if (it.p && !is_device_ptr(p)) {
      it.off = (in ? in : &own)->take<char>(bytes).off;
      any = true;
    }
    items.push_back(it);
  }
  // One async copy per host array to base + its offset.
  hipError_t copy(void* base, hipStream_t s) {
    for (Item& it : items) {
      if (it.off == SIZE_MAX) continue;
      char* dst = static_cast<char*>(base) + it.off;
      const hipError_t e = hipMemcpyAsync(dst, it.p, it.bytes, hipMemcpyHostToDevice, s);
      if (e != hipSuccess) return e;
      it.p = dst;
    }
    return hipSuccess;
  }
  template <class T>
  const T* dev(size_t k) const { return static_cast<const T*>(items[k].p); }
};

// spray_rt_domains_build; *failed_job = the index of the job a failure names,
// -1 where it names none.
int domains_build(spray_rt_ctx* c, int n, const int* slots, const float* const* verts,
                  const size_t* nverts, const uint32_t* const* faces, const size_t* nfaces,
                  const uint32_t* const* colors_rgb, const float* const* vnormals,
                  float* d_bounds, int* failed_job);
// scene-path entry checks + lazy rebuild of the device scene tables
int scene_common(spray_rt_ctx* c, const void* rays, size_t M, const void* out);
// the kernels' view of the resident scene (coherence = the context's)
SceneView view(const spray_rt_ctx* c);
// the whole shading of a bounce is the point-light term of camera rays (PT,
// one point light, diffuse surfaces, bounces = 1): it fuses into the
// closest-hit launch (launch_scene_frame_pt)
bool fused_pt_shading(const spray_rt_ctx* c, const spray_rt_shader* P);

}  // namespace detail
}  // namespace spray_rt

#define HIPCHK(ctx, expr)                                                   \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess)                                                   \
      return ::spray_rt::detail::fail(ctx, SPRAY_RT_ERR_HIP, "%s: %s", #expr, \
                                      hipGetErrorString(_e));               \
  } while (0)
