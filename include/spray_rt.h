/*
 * spray_rt.h -- C ABI of the MI355X (gfx950) BVH traversal + ray/triangle
 * intersection engine that drops in behind SpRay's scene intersect/occluded
 * surface.
 *
 * Reference interface each entry point replaces (paths relative to the
 * hyungman/SpRay tree):
 *   spray_rt_domain_upload   TriMeshBuffer::load + mapEmbreeBuffer
 *                            (src/render/trimesh_buffer.cc:117-169, :189-225):
 *                            rtcNewTriangleMesh/rtcSetBuffer2/rtcCommit per
 *                            cache block, here a device BVH per slot.
 *   spray_rt_domain_bounds   WbvhEmbree::init/build
 *                            (src/render/wbvh_embree.cc:31-111).
 *   spray_rt_intersect1M     Scene::intersect (src/render/scene.h:157-173,
 *                            scene.inl:189-199): rtcIntersect + the
 *                            TriMeshBuffer::updateIntersection epilogue
 *                            (trimesh_buffer.cc:328-360), over a stream of
 *                            RTCRayIntersection records.
 *   spray_rt_occluded1M      Scene::occluded (scene.h:175-195,
 *                            scene.inl:201-209): rtcOccluded over RTCRay
 *                            records.
 *   spray_rt_domains1M       Scene::intersectDomains -> WbvhEmbree::intersect
 *                            (scene.h:197, wbvh_embree.cc:126-148) +
 *                            DomainList::sort (src/render/rays.h:71-79).
 *   spray_rt_*_segments      the per-domain queue drains of the schedulers
 *                            (src/ooc/ooc_tcontext.inl:28-100,
 *                            src/insitu/insitu_tcontext.inl:125-186) in one
 *                            launch.
 *   spray_rt_*_scene         the speculative resolution of a ray over every
 *                            domain of its list (ooc_isector.h:126-145 +
 *                            ooc_vbuf.cc:54-112): nearest hit over all
 *                            listed domains in one launch.
 *
 * Conventions
 *  - Every function returns SPRAY_RT_OK (0) or a negative status; nothing
 *    throws across the boundary.  spray_rt_last_error() gives the message.
 *  - Ray/hit buffers may be host or device pointers.  With host pointers the
 *    call is synchronous (results are in place on return), as Embree's is.
 *    With device pointers the work is enqueued on the context's stream
 *    (spray_rt_set_stream) and spray_rt_sync() waits for it.
 *  - Result semantics: tfar is written only on a hit;
 *    geomID becomes 0 on a hit / occlusion and is otherwise left as the
 *    caller set it (0xFFFFFFFF); instID is never touched; color (byte
 *    offset 60) and Ns (offset 84) are filled by the fused epilogue.
 *  - One context per GPU; a context is driven by one host thread at a time,
 *    except through lanes (spray_rt_lane_*): one lane per host thread, run
 *    concurrently.
 */
#ifndef SPRAY_RT_H_
#define SPRAY_RT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPRAY_RT_OK 0
#define SPRAY_RT_ERR_ARG (-1)
#define SPRAY_RT_ERR_HIP (-2)
#define SPRAY_RT_ERR_STATE (-3)
#define SPRAY_RT_ERR_NOMEM (-4)
#define SPRAY_RT_ERR_LIMIT (-5)
#define SPRAY_RT_ERR_UNSUPPORTED (-6) /* a case the reference aborts on */

#define SPRAY_RT_INVALID_ID 0xFFFFFFFFu
#define SPRAY_RT_MAX_SCENE_DOMAINS 256

typedef struct spray_rt_ctx* spray_rt_ctx_t;

/* Embree-2 record layouts the stream calls accept (src/render/rays.h:246-274
 * and embree2/rtcore_ray.h).  Only these byte offsets are read or written:
 * org 0, dir 16, tnear 32, tfar 36, Ng 48, color 60, u 64, v 68, geomID 72,
 * primID 76, Ns 84 (RTCRayIntersection; sizeof = 96). */
typedef struct spray_rt_ray_intersection {
  float org[3];
  float align0;
  float dir[3];
  float align1;
  float tnear;
  float tfar;
  float time;
  uint32_t mask;
  float Ng[3];
  uint32_t color;
  float u;
  float v;
  uint32_t geomID;
  uint32_t primID;
  uint32_t instID;
  float Ns[3];
} spray_rt_ray_intersection;

/* Compact ray of the fused scene path: 32 B, two 16-B loads per lane.
 * Every scene launch honours the record's own extents: a hit satisfies
 * tnear < t <= tfar (t == tfar is accepted), in every domain the ray visits.
 * The ray's domain list ignores them (intersectAabb with 0.001 and +inf).
 * A record holding a NaN or an infinity in org or dir, an all-zero dir, a NaN
 * tnear or a NaN tfar is a miss and not occluded; its neighbours are
 * unaffected. */
typedef struct spray_rt_ray {
  float org[3];
  float tnear;
  float dir[3];
  float tfar;
} spray_rt_ray;

/* Scene-path hit record (48 B): t = +inf, prim = 0xFFFFFFFF, domain = -1 on
 * a miss; ng = Embree 2 unnormalised geometry normal (v0-v1)x(v2-v0);
 * color/ns = updateIntersection epilogue. */
typedef struct spray_rt_hit {
  float t, u, v;
  uint32_t prim;
  float ng[3];
  uint32_t color;
  float ns[3];
  int32_t domain;
} spray_rt_hit;

/* ---- context ---- */
int spray_rt_create(int hip_device, spray_rt_ctx_t* out);
int spray_rt_destroy(spray_rt_ctx_t ctx);
const char* spray_rt_last_error(spray_rt_ctx_t ctx);
/* Enqueue all further work on hip_stream (a hipStream_t; NULL = the null
 * stream).  A new context uses a private non-blocking stream. */
int spray_rt_set_stream(spray_rt_ctx_t ctx, void* hip_stream);
int spray_rt_sync(spray_rt_ctx_t ctx);

/* ---- domains / cache slots ---- */
/* Uploads one domain mesh (world-space vertices) into cache slot `slot`
 * (SceneInfo.cache_block): builds the BVH on the host and copies BVH,
 * triangles and the epilogue arrays (faces, colors 0xRRGGBB per vertex,
 * unnormalised vertex normals; either may be NULL) to the device.  async=0:
 * returns after the copy completed; async=1: copies are enqueued on the
 * context's upload stream and ordered before the next query. */
int spray_rt_domain_upload(spray_rt_ctx_t ctx, int slot, const float* verts_xyz,
                           size_t nverts, const uint32_t* faces, size_t nfaces,
                           const uint32_t* colors_rgb, const float* vnormals,
                           int async);
/* Releases a slot's device memory. */
int spray_rt_domain_release(spray_rt_ctx_t ctx, int slot);
/* Domain world bounds [n][6] = lo.xyz hi.xyz (Domain::world_aabb). */
int spray_rt_domain_bounds(spray_rt_ctx_t ctx, int ndomains,
                           const float* aabb_min_max);
/* Which slot holds domain `domain_id` for the scene path (-1 = none). */
int spray_rt_map_domain(spray_rt_ctx_t ctx, int domain_id, int slot);
/* BVH statistics of a slot: nodes, depth, triangles. */
int spray_rt_slot_info(spray_rt_ctx_t ctx, int slot, size_t* nnodes,
                       int* depth, size_t* ntris);

/* Host-only: the canonical BVH2 a slot upload would build (no GPU needed).
 * Call with NULL outputs for sizes.  nodes_out: 64-B nodes (padded boxes),
 * tris_out: [ntris][12] v0 e1 e2 Ng, prims_out: leaf order -> face index. */
int spray_rt_bvh_build_host(const float* verts_xyz, size_t nverts,
                            const uint32_t* faces, size_t nfaces,
                            size_t* nnodes, int* depth, void* nodes_out,
                            float* tris_out, uint32_t* prims_out);

/* Host-only: the 16-bit quantized copy of that BVH2 (32-B nodes: u16 l_lo xyz, l_hi xyz, r_lo xyz, r_hi xyz, int32
 * left, right; decoded bound = base + q * scale, grid_out = base xyz, scale
 * xyz).  SPRAY_RT_ERR_LIMIT if the coordinates exceed the grid's range. */
int spray_rt_qnodes_host(const float* verts_xyz, size_t nverts, const uint32_t* faces,
                         size_t nfaces, size_t* nnodes, float grid_out[6], void* qnodes_out);

/* Host-only: the 4-wide quantized collapse of that BVH2 the per-lane any-hit
 * walk reads (64-B nodes: u16 child boxes [4][lo xyz, hi xyz], int32 child
 * refs [4], >= 0 node index, < 0 leaf ~((first << 2) | (count - 1)), INT32_MIN
 * empty; same grid as above), and the walk's stack bound (entries).
 * SPRAY_RT_ERR_LIMIT if the coordinates exceed the grid's range. */
int spray_rt_qnodes4_host(const float* verts_xyz, size_t nverts, const uint32_t* faces,
                          size_t nfaces, size_t* nnodes, int* stack_bound, float grid_out[6],
                          void* qnodes_out);

/* ---- moving geometry: refit of resident slots ---- */
/* New vertex positions for resident slots whose topology (faces) is unchanged.
 * verts[i]: [nverts of slots[i]][3] floats, world space; vnormals[i]: the new
 * unnormalised vertex normals, required iff the slot was uploaded with normals
 * (vnormals itself may be NULL when no slot has any).  Pointers may be device or
 * host memory (host: staged, and the call returns with the work completed), as
 * for ray buffers.  d_bounds (optional, device float[n][6]) receives each
 * slot's new exact, unpadded lo.xyz hi.xyz: the caller re-issues
 * spray_rt_domain_bounds when the geometry left its domain box (then
 * spray_rt_map_domain and spray_rt_set_owners again: that call resets both).
 * One host read of n status words per call, however many slots; ordered after
 * queued work on the context's stream and before the next query.
 *
 * What is kept: faces, the leaf order, leaf ranges, child refs, the 4-wide
 * collapse and its child refs, the tree depth and the walks' stack bound.
 * What is recomputed on the device with the builder's own arithmetic: every
 * BVH2 child box (exact min/max of its subtree's new vertices, then the
 * builder's padding), every triangle record, the quantization grid, every
 * 4-wide child box, the normals.  Closest hits do not depend on the tree
 * (the minimum of (t, primID)), so queries after a refit return the bits a
 * fresh spray_rt_domain_upload of the new vertices returns; a refit with the
 * vertices a slot was built from reproduces its image byte for byte (up to
 * the sign of a zero box bound of a mesh that holds both +0 and -0).  The
 * tree is only as good as the old topology allows on the new positions:
 * watch spray_rt_slot_sah and rebuild with spray_rt_domain_upload when it
 * has grown too far.
 *
 * A failed call leaves every slot of the call exactly as it was (all
 * validation happens before any slot memory is written): SPRAY_RT_ERR_ARG
 * for an unloaded slot, a slot listed twice, a NULL vertex pointer, a
 * missing normal array where the slot has normals, or a non-finite
 * coordinate (or edge) of a referenced vertex; SPRAY_RT_ERR_LIMIT when a box
 * cannot be quantized.  spray_rt_last_error names the slot.
 *
 * Deliberately left out: the images of the out-of-core cache
 * (spray_rt_ooc_set_domain; they carry no refit metadata), the scene layer's
 * domain cache (include/spray_scene.h, spray_scene.hpp: a cache miss uploads
 * the image built from the file again).  A new triangle list is what
 * spray_rt_domains_build below is for.  Not for use while lanes run (they read
 * the slot tables). */
int spray_rt_domains_refit(spray_rt_ctx_t ctx, int n, const int* slots,
                           const float* const* verts, const float* const* vnormals,
                           float* d_bounds);
/* Host-only restatement (no GPU): the image a refit produces from the canonical
 * build of (verts0, faces) and new_verts.  Same output conventions as
 * spray_rt_bvh_build_host / spray_rt_qnodes4_host (any output may be NULL;
 * sizes as those calls report them for (verts0, faces)).  SPRAY_RT_ERR_ARG /
 * SPRAY_RT_ERR_LIMIT as spray_rt_domains_refit. */
int spray_rt_bvh_refit_host(const float* verts0, const float* new_verts, size_t nverts,
                            const uint32_t* faces, size_t nfaces, void* nodes_out,
                            float* tris_out, float grid_out[6], void* qnodes4_out);
/* ---- changing topology: slots built on the device ---- */
/* New triangle lists for n slots in one batched call on the context's stream,
 * without the host builder: verts[i] [nverts[i]][3] floats, faces[i]
 * [nfaces[i]][3] indices, colors_rgb[i] / vnormals[i] per vertex (either array,
 * or single entries, may be NULL).  Every array pointer may be device or host
 * memory (host: staged, and the call returns with the work completed).  A slot
 * may be empty or loaded; a loaded slot's image is replaced after the queued
 * work that reads it.  d_bounds (optional, device float[n][6]) receives each
 * slot's exact, unpadded lo.xyz hi.xyz, as in spray_rt_domains_refit; per time
 * step: build, then spray_rt_domain_bounds, spray_rt_map_domain,
 * spray_rt_set_owners.
 *
 * Afterwards the slot is a slot of spray_rt_domain_upload for every call that
 * takes one -- the 1M streams, every scene launch, spray_rt_slot_info / _export
 * / _sah, spray_rt_domain_release, a later spray_rt_domains_refit -- and, since
 * closest hits are the minimum of (t, primID) and any hits a flag, every query
 * returns the bits it returns on the uploaded slot.  The tree differs: ranges
 * over the triangles sorted by (30-bit Morton code of the box centroid, face)
 * split at the highest differing code bit (the median under the host builder's
 * depth rule), nodes and QNode4s numbered level by level; it is a function of
 * the mesh alone, and spray_rt_bvh_build_device_host restates it byte for byte.
 * It costs more to trace than the host builder's binned-SAH tree (DESIGN.md
 * section 11 has the figures): prefer spray_rt_domain_upload for geometry that
 * stays, this call for geometry that is replaced every time step.  One
 * workgroup per slot builds the topology: made for many small domains, correct
 * but slow for one huge one.
 *
 * At most two host reads per call, however many slots (the sort's partition of
 * the segments by size, and one record per slot).  A failed call leaves every
 * slot of the call exactly as it was: SPRAY_RT_ERR_ARG for NULL arrays, a slot
 * listed twice, nfaces >= 2^29, a face index >= nverts, or a non-finite
 * coordinate (or edge) of a referenced vertex; SPRAY_RT_ERR_LIMIT when a box
 * cannot be quantized.  spray_rt_last_error names the slot.  An empty mesh gives
 * the empty slot an upload gives.  Not for use while lanes run. */
int spray_rt_domains_build(spray_rt_ctx_t ctx, int n, const int* slots,
                           const float* const* verts, const size_t* nverts,
                           const uint32_t* const* faces, const size_t* nfaces,
                           const uint32_t* const* colors_rgb, const float* const* vnormals,
                           float* d_bounds);
/* Host-only restatement (no GPU) of the same algorithm: the arrays
 * spray_rt_domains_build leaves in a slot, byte for byte.  Any output may be
 * NULL; a call with NULL outputs reports the sizes (nodes_out BvhNode[*nnodes],
 * tris_out float[nfaces][12], prims_out uint32[nfaces], qnodes4_out
 * QNode4[*nq]).  depth: deepest leaf (the root is depth 0); stack_bound: pending
 * entries of the 4-wide walk; nmedian: the splits the depth rule forced to the
 * median.  SPRAY_RT_ERR_ARG / SPRAY_RT_ERR_LIMIT as spray_rt_domains_build. */
int spray_rt_bvh_build_device_host(const float* verts, size_t nverts, const uint32_t* faces,
                                   size_t nfaces, size_t* nnodes, size_t* nq, int* depth,
                                   int* stack_bound, int* nmedian, void* nodes_out,
                                   float* tris_out, uint32_t* prims_out, float grid_out[6],
                                   void* qnodes4_out);
/* ---- isosurfaces of scalar grids, extracted on the device ---- */
/* One structured grid of scalars and the isovalue to contour it at. */
typedef struct spray_rt_grid {
  const float* values;  /* [nz][ny][nx], x fastest; device or host memory */
  int32_t dims[3];      /* points per axis (nx, ny, nz), each >= 2 */
  float origin[3];      /* point (i,j,k) at origin + (i,j,k) * spacing */
  float spacing[3];     /* > 0 */
  float isovalue;
  uint32_t color_rgb;   /* one colour for every vertex ... */
  int32_t has_color;    /* ... or none (spray_rt_domains_isosurface only) */
} spray_rt_grid;
/* The algorithm is fixed, so that the kernels and the host restatement agree
 * byte for byte: marching tetrahedra over the Kuhn split
 * of each cell (six tetrahedra, one per permutation of the axes in
 * lexicographic order, each walking from the cell's corner (0,0,0) to (1,1,1));
 * a sample is inside when f >= isovalue.  The mesh is welded and indexed:
 * every vertex lies on a lattice edge that starts at its componentwise-smaller
 * endpoint a and has one of 7 types (+x +y +z +xy +xz +yz +xyz), at
 * pa + t * (pb - pa) per axis with t = (isovalue - fa) / (fb - fa), in float
 * without contraction -- a function of the lattice edge alone, so the mesh is
 * watertight within a grid, and two grids that share a sample plane and their
 * origin arithmetic agree on it bit for bit.  Vertices are ordered by (point,
 * x fastest; edge type), faces by (cell, x fastest; tetrahedron; triangle);
 * Ng = (v0 - v1) x (v2 - v0) points toward decreasing values.  Normals are
 * unnormalised: the negated gradient (central differences, one-sided on the
 * grid boundary, divided by the spacing) of the edge's endpoints, interpolated
 * with t.  A sample equal to the isovalue puts vertices on lattice points and
 * may give zero-area triangles; they are kept (dropping them would break the
 * numbering, and every later stage accepts them).  At most 12 triangles per
 * cell; no atomic and no hash decides an index, two runs give the same bytes.
 *
 * spray_rt_isosurface extracts n grids into the caller's device buffers in one
 * batched call on the context's stream: verts[i] float [cap_verts[i]][3],
 * vnormals[i] the same (the array, or single entries, may be NULL), faces[i]
 * uint32 [cap_faces[i]][3].  nverts_out / nfaces_out (host arrays, either may
 * be NULL) are written on return: the call's one host read.  verts == NULL
 * only counts.  A capacity that is too small gives SPRAY_RT_ERR_LIMIT with the
 * counts reported and no buffer written.  Errors as
 * spray_rt_domains_isosurface. */
int spray_rt_isosurface(spray_rt_ctx_t ctx, int n, const spray_rt_grid* grids,
                        float* const* verts, float* const* vnormals, uint32_t* const* faces,
                        const size_t* cap_verts, const size_t* cap_faces, size_t* nverts_out,
                        size_t* nfaces_out);
/* Grids in, resident slots out: count, one host read, emit into context
 * scratch grown on demand, then the device build of spray_rt_domains_build on
 * those device arrays.  Afterwards slots[i] is a slot of spray_rt_domains_build
 * of the extracted mesh of grids[i] (with its normals if with_normals, its
 * colour if has_color), byte for byte, for every call that takes a slot, a
 * later spray_rt_domains_refit included.  d_bounds as in spray_rt_domains_build;
 * nfaces_out (optional, host size_t[n]) receives the triangle counts.
 *
 * At most three host reads per call, however many slots (the counts, and the
 * build's two).  A failed call leaves every slot as it was: SPRAY_RT_ERR_ARG
 * for a NULL pointer, dims < 2, a non-positive or non-finite spacing, a
 * non-finite origin or isovalue, a non-finite sample, a bad slot or a slot
 * listed twice; SPRAY_RT_ERR_LIMIT for 2^31 or more points, 2^29 or more faces,
 * or a box that cannot be quantized.  spray_rt_last_error names the grid.  An
 * empty surface gives the empty slot an empty upload gives.  Not for use while
 * lanes run. */
int spray_rt_domains_isosurface(spray_rt_ctx_t ctx, int n, const int* slots,
                                const spray_rt_grid* grids, int with_normals, float* d_bounds,
                                size_t* nfaces_out);
/* Host-only restatement (no GPU; grid->values is host memory): the arrays the
 * kernels write, byte for byte.  *nverts / *nfaces are always reported; any
 * output may be NULL (verts_out float[*nverts][3], vnormals_out the same,
 * faces_out uint32[*nfaces][3]). */
int spray_rt_isosurface_host(const spray_rt_grid* grid, size_t* nverts, size_t* nfaces,
                             float* verts_out, float* vnormals_out, uint32_t* faces_out);
/* ---- isosurfaces coloured by a second field through a colour map ---- */
/* The colour map of one grid: entry i of an array parallel to the spray_rt_grid
 * array.  field == NULL: the grid keeps the constant-colour rule (color_rgb /
 * has_color), so one batch may mix mapped, constant-colour and colourless
 * grids. */
typedef struct spray_rt_grid_color {
  const float* field;        /* the grid's dims and layout; device or host memory */
  const uint32_t* table_rgb; /* [ntable] 0x00RRGGBB, host memory, copied verbatim */
  int32_t ntable;            /* 1 .. 4096 */
  float lo, hi;              /* lo < hi, both finite */
} spray_rt_grid_color;
/* The rule is fixed like the extraction's, in float
 * without contraction: scale = float(ntable) / (hi - lo), evaluated once on
 * the host (it must be a finite, normal float); a scalar g maps to
 * table_rgb[idx], x = (g - lo) * scale, idx = !(x >= 0) ? 0 : (x >=
 * float(ntable) ? ntable - 1 : int(x)) -- the nearest bin, clamped at both
 * ends, no interpolation between entries (use a finer table).  The vertex on
 * the lattice edge (a, b) at the extraction's t gets map(ga + t * (gb - ga)),
 * ga / gb the colour field's samples at the edge's endpoints: a function of
 * the lattice edge alone, like the position, so two grids that share a sample
 * plane and the colour samples on it agree on the shared vertices' colours.  A
 * slice is the isosurface of a plane-distance field coloured by the data.
 *
 * spray_rt_isosurface_mapped is spray_rt_isosurface plus colors[i] uint32
 * [cap_verts[i]]: the mapped colour per vertex, color_rgb for a grid without a
 * colour field.  verts / vnormals / colors / faces, or single entries of them,
 * may be NULL independently (cap_verts is read where a grid has a per-vertex
 * array, cap_faces where it has faces); all NULL only counts.  Positions,
 * normals and faces are spray_rt_isosurface's, byte for byte.  With colors
 * alone the call skips the position, normal and face work: the form that
 * recolours a slot (spray_rt_domains_recolor below).
 *
 * Errors on top of spray_rt_isosurface's, all SPRAY_RT_ERR_ARG, naming the grid,
 * before anything is written: a colour field with a NULL table, ntable out of
 * range, lo >= hi or non-finite, a scale that is not a finite normal float, a
 * non-finite colour sample (found by the count pass, reported at the call's one
 * host read). */
int spray_rt_isosurface_mapped(spray_rt_ctx_t ctx, int n, const spray_rt_grid* grids,
                               const spray_rt_grid_color* gcolors, float* const* verts,
                               float* const* vnormals, uint32_t* const* colors,
                               uint32_t* const* faces, const size_t* cap_verts,
                               const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out);
/* spray_rt_domains_isosurface with mapped colours: a slot carries colours when
 * its grid has a colour field or has_color.  The same host reads (at most
 * three) and the same all-or-nothing failure; the errors of
 * spray_rt_isosurface_mapped on top.  Not for use while lanes run. */
int spray_rt_domains_isosurface_mapped(spray_rt_ctx_t ctx, int n, const int* slots,
                                       const spray_rt_grid* grids,
                                       const spray_rt_grid_color* gcolors, int with_normals,
                                       float* d_bounds, size_t* nfaces_out);
/* Host-only restatement (no GPU; the fields are host memory): as
 * spray_rt_isosurface_host, plus colors_out uint32[*nverts].  gcolor may be
 * NULL. */
int spray_rt_isosurface_mapped_host(const spray_rt_grid* grid, const spray_rt_grid_color* gcolor,
                                    size_t* nverts, size_t* nfaces, float* verts_out,
                                    float* vnormals_out, uint32_t* colors_out,
                                    uint32_t* faces_out);
/* The map alone, for meshes that carry per-vertex data of their own:
 * colors_out[i] = map(scalars[i]) for n scalars on the context's stream.
 * scalars: device or host memory (host: staged); colors_out: device memory.
 * SPRAY_RT_ERR_ARG for a bad map or a non-finite scalar (one status-word read:
 * the call synchronises; colors_out is then unspecified). */
int spray_rt_colormap_apply(spray_rt_ctx_t ctx, const float* scalars, size_t n,
                            const uint32_t* table_rgb, int32_t ntable, float lo, float hi,
                            uint32_t* colors_out);
/* Host-only restatement of spray_rt_colormap_apply (no GPU). */
int spray_rt_colormap_host(const float* scalars, size_t n, const uint32_t* table_rgb,
                           int32_t ntable, float lo, float hi, uint32_t* colors_out);
/* New per-vertex colours for n resident slots in one batched call, ordered
 * after the queued work on the context's stream and before the next query:
 * colors_rgb[i] uint32 [nverts[i]], device or host memory (host: staged, and
 * the call returns with the work completed).  Only the slots' colour arrays
 * are written: trees, records, faces, normals and refit metadata keep their
 * bytes, and a later spray_rt_domains_refit keeps the new colours.
 *
 * All validation happens on the host before anything is enqueued, so a failed
 * call leaves every slot as it was and the call reads no device state:
 * SPRAY_RT_ERR_ARG for an unloaded slot, a slot listed twice, a slot uploaded or
 * built without colours (a slot is one allocation: a colour array cannot be
 * added), a NULL pointer, or nverts[i] different from the slot's.
 * spray_rt_last_error names the slot.  Not for use while lanes run.
 *
 * Recolouring an isosurface slot (another colour field, another table) is
 * spray_rt_isosurface_mapped with colors alone on the same grids, then this
 * call with those device pointers: a colour pass instead of a build.  That
 * relies on the geometry field and the isovalue being the ones the slot was
 * extracted from; the nverts check catches most mismatches, not all. */
int spray_rt_domains_recolor(spray_rt_ctx_t ctx, int n, const int* slots,
                             const uint32_t* const* colors_rgb, const size_t* nverts);
/* ---- isosurfaces of unstructured tetrahedral meshes ---- */
/* One tetrahedral mesh with a scalar per point and the isovalue to contour it
 * at: what a finite-element or finite-volume code leaves in HBM. */
typedef struct spray_rt_tetmesh {
  const float*    points;        /* [npoints][3]; device or host memory */
  const uint32_t* tets;          /* [ntets][4] point indices; device or host */
  const float*    values;        /* [npoints], the field to contour */
  const float*    point_normals; /* optional [npoints][3], unnormalised, e.g. the
                                    negated gradient; NULL: the mesh has no normals */
  size_t   npoints, ntets;
  float    isovalue;
  uint32_t color_rgb;            /* as spray_rt_grid */
  int32_t  has_color;
} spray_rt_tetmesh;
/* The rule is fixed like the grid extraction's, so that the kernels and the
 * host restatement agree byte for byte, in float
 * without contraction.  A point is inside when f >= isovalue.  There is one
 * vertex per distinct unordered point pair {a, b}, a < b by point index, that
 * is an edge of at least one tetrahedron and whose endpoints differ in sign:
 * t = (isovalue - f[a]) / (f[b] - f[a]), position p[a] + t * (p[b] - p[a]) per
 * axis, normal and colour scalar interpolated the same way, colour
 * map(g[a] + t * (g[b] - g[a])) with spray_rt_grid_color's rule (its field is
 * [npoints] here) or color_rgb -- all a function of the pair alone, so the
 * mesh is watertight, and two meshes that share points with equal
 * coordinates, samples and relative index order agree bit for bit on the
 * shared vertices.  Vertices are ascending by (a << 32) | b.  Faces come per
 * tetrahedron in input order, then triangle 0..1: marching tetrahedra with the
 * tet's four listed points as the walk, and the orientation from the
 * geometry, not from the caller's vertex order: odd when det = dot(cross(p1 -
 * p0, p2 - p0), p3 - p0) < 0, evaluated term by term in float, left to right
 * (det == 0 and NaN count as even), so a mesh of mixed tet orientations still
 * gives Ng = (v0 - v1) x (v2 - v0) pointing toward decreasing values.  A
 * sliver whose float det has the wrong sign flips its one or two triangles.
 * A sample equal to the isovalue gives t of 0 or 1 and possibly zero-area
 * triangles; they are kept.  A tet that lists a point twice never crosses on
 * that pair; duplicate tets give duplicate faces.  No atomic and no hash
 * decides an index: two runs give the same bytes.
 *
 * spray_rt_tet_isosurface extracts n meshes into the caller's device buffers
 * in one batched call on the context's stream, with the argument shapes of
 * spray_rt_isosurface_mapped: gcolors may be NULL; verts / vnormals / colors /
 * faces, or single entries of them, may be NULL independently; all NULL only
 * counts.  Two host reads, however many meshes: status and the instance /
 * face totals after the count pass, the vertex counts after the sort.  A
 * capacity that is too small gives SPRAY_RT_ERR_LIMIT with the counts
 * reported and no buffer written.
 *
 * SPRAY_RT_ERR_ARG, before anything is written and naming the mesh: a NULL
 * pointer (ntets == 0 is allowed, reads nothing and gives the empty surface),
 * a non-finite isovalue, a bad colour map (spray_rt_isosurface_mapped's
 * checks), vnormals[i] non-NULL for a mesh without point_normals, a point
 * index >= npoints, or a non-finite value among what the call reads of a
 * point some tet references: coordinates, sample, colour sample of a mapped
 * mesh, normal where normals are written (points no tet references are never
 * read).  SPRAY_RT_ERR_LIMIT: ntets >= 2^29, npoints >= 2^32, or 2^32 or more
 * crossing (tet, edge) instances in one call. */
int spray_rt_tet_isosurface(spray_rt_ctx_t ctx, int n, const spray_rt_tetmesh* meshes,
                            const spray_rt_grid_color* gcolors, float* const* verts,
                            float* const* vnormals, uint32_t* const* colors,
                            uint32_t* const* faces, const size_t* cap_verts,
                            const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out);
/* Meshes in, resident slots out: the extraction into context scratch at the
 * exact sizes, then the device build of spray_rt_domains_build on those device
 * arrays.  Afterwards slots[i] is a slot of spray_rt_domains_build of the
 * extracted mesh of meshes[i] (with its normals if with_normals and the mesh
 * has point_normals, its colours if it is mapped or has_color), byte for byte,
 * for every call that takes a slot, a later spray_rt_domains_refit and
 * spray_rt_domains_recolor included.  At most four host reads per call (the
 * extraction's two and the build's two).  A failed call leaves every slot as
 * it was; errors as spray_rt_tet_isosurface, plus a bad slot or a slot listed
 * twice and the build's limits.  Not for use while lanes run. */
int spray_rt_domains_tet_isosurface(spray_rt_ctx_t ctx, int n, const int* slots,
                                    const spray_rt_tetmesh* meshes,
                                    const spray_rt_grid_color* gcolors, int with_normals,
                                    float* d_bounds, size_t* nfaces_out);
/* Where the last tet extraction of the context spent its time: out_ms[0..2]
 * wall clock from entry to host read 1, from there to host read 2, from there
 * to the end of the vertex and face passes' enqueue; out_ms[3] the device time
 * of the segmented sort (HIP events on the context's stream), recorded only
 * while timing is on (spray_rt_tet_set_timing; off by default), else 0. */
int spray_rt_tet_set_timing(spray_rt_ctx_t ctx, int on);
int spray_rt_tet_phase_times(spray_rt_ctx_t ctx, double out_ms[4]);
/* Host-only restatement (no GPU; every array is host memory): the arrays the
 * kernels write, byte for byte.  *nverts / *nfaces are reported where the
 * input is valid; any output may be NULL (as spray_rt_isosurface_mapped_host);
 * vnormals_out needs point_normals.  gcolor may be NULL. */
int spray_rt_tet_isosurface_host(const spray_rt_tetmesh* mesh, const spray_rt_grid_color* gcolor,
                                 size_t* nverts, size_t* nfaces, float* verts_out,
                                 float* vnormals_out, uint32_t* colors_out, uint32_t* faces_out);
/* ---- isosurfaces of hexahedral, wedge, pyramid and tetrahedral cells ---- */
/* Cell types and the order of points within a cell are VTK's. */
#define SPRAY_RT_CELL_TET     10  /* 4 points */
#define SPRAY_RT_CELL_HEX     12  /* 8: 0-1-2-3 one face in cyclic order, 4-5-6-7 the opposite
                                     face, 4 above 0 */
#define SPRAY_RT_CELL_WEDGE   13  /* 6: 0-1-2 a triangle, 3-4-5 the opposite one, 3 above 0 */
#define SPRAY_RT_CELL_PYRAMID 14  /* 5: 0-1-2-3 the base in cyclic order, 4 the apex */
/* One mixed unstructured mesh with a scalar per point and the isovalue to
 * contour it at. */
typedef struct spray_rt_cellmesh {
  const float*    points;        /* [npoints][3]; device or host memory */
  const uint8_t*  types;         /* [ncells] SPRAY_RT_CELL_* */
  const uint32_t* offsets;       /* [ncells + 1]; cell i lists conn[offsets[i] .. offsets[i+1]) */
  const uint32_t* conn;          /* [nconn] point indices */
  const float*    values;        /* [npoints] */
  const float*    point_normals; /* optional [npoints][3], as spray_rt_tetmesh */
  size_t   npoints, ncells, nconn;
  float    isovalue;
  uint32_t color_rgb;
  int32_t  has_color;
} spray_rt_cellmesh;
/* The surface is spray_rt_tet_isosurface's of a tet list that a fixed rule
 * makes of the cells.  A tet cell is its four points as
 * listed.  Any other cell is the cone from its apex over the faces that do
 * not contain the apex.  With faces as local positions, quads in cyclic order,
 *   hex      (0,1,2,3) (4,5,6,7) (0,1,5,4) (1,2,6,5) (2,3,7,6) (3,0,4,7)
 *   wedge    (0,1,2) (3,4,5) (0,1,4,3) (1,2,5,4) (2,0,3,5)
 *   pyramid  (0,1,2,3) (0,1,4) (1,2,4) (2,3,4) (3,0,4)
 * the apex m is the local position of the cell's smallest point index (the
 * lowest position on ties); each face in table order that does not contain m
 * gives, as a triangle (q0,q1,q2), the tet (P[m], P[q0], P[q1], P[q2]), and as
 * a quad, with j the position within the face of its smallest point index
 * (lowest j on ties) and r_d = q[(j + d) mod 4], the tets (P[m], P[r0], P[r1],
 * P[r2]) then (P[m], P[r0], P[r2], P[r3]): 6 tets per hex, 3 per wedge, 2 per
 * pyramid, ordered by cell, then by face, then by the two triangles of a quad.
 * Every quad face of the mesh is cut through its smallest point index from
 * both sides, so the split is conforming whatever the cell types, and a hex
 * mesh of a lattice numbered x fastest has the Kuhn split of
 * spray_rt_isosurface.  A collapsed cell that lists a point twice goes
 * through the same rule.
 *
 * spray_rt_cell_isosurface has the argument shapes and NULL conventions of
 * spray_rt_tet_isosurface (gcolors fields are [npoints]).  Only the cells the
 * surface crosses become tets on the device; the bytes are those of the full
 * list.  At most three host reads per call: the cell pass's status and tet
 * totals, then the tet extraction's two.
 *
 * SPRAY_RT_ERR_ARG, before anything is written and naming the mesh: a NULL
 * pointer (ncells == 0 reads nothing and gives the empty surface), a
 * non-finite isovalue, a bad colour map, vnormals[i] non-NULL for a mesh
 * without point_normals, an unknown cell type, offsets[i+1] - offsets[i]
 * different from the type's point count, offsets[i+1] > nconn, a point index
 * >= npoints, or a non-finite value among what the call reads of a point some
 * cell references, whether the surface crosses that cell or not (points no
 * cell references are never read).  SPRAY_RT_ERR_LIMIT: ncells >= 2^29,
 * nconn >= 2^32, npoints >= 2^32, 2^29 or more tets from crossing cells in
 * one mesh, 2^32 or more crossing (tet, edge) instances in one call, more
 * than 65,535 meshes. */
int spray_rt_cell_isosurface(spray_rt_ctx_t ctx, int n, const spray_rt_cellmesh* meshes,
                             const spray_rt_grid_color* gcolors, float* const* verts,
                             float* const* vnormals, uint32_t* const* colors,
                             uint32_t* const* faces, const size_t* cap_verts,
                             const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out);
/* Meshes in, resident slots out, as spray_rt_domains_tet_isosurface: slots[i]
 * is byte for byte a slot of spray_rt_domains_build of the extracted mesh.  At
 * most five host reads (the extraction's three and the build's two).  A failed
 * call leaves every slot as it was; messages name the mesh and its slot.  Not
 * for use while lanes run. */
int spray_rt_domains_cell_isosurface(spray_rt_ctx_t ctx, int n, const int* slots,
                                     const spray_rt_cellmesh* meshes,
                                     const spray_rt_grid_color* gcolors, int with_normals,
                                     float* d_bounds, size_t* nfaces_out);
/* Where the last cell extraction of the context spent its time: out_ms[0]
 * wall clock from entry to the cell pass's host read, out_ms[1..4] from there
 * on as spray_rt_tet_phase_times' four. */
int spray_rt_cell_phase_times(spray_rt_ctx_t ctx, double out_ms[5]);
/* Host-only (no GPU; every array is host memory).  spray_rt_cell_split_host
 * writes the full tet list of the rule, [*ntets][4] point indices (tets_out
 * NULL: the count alone); it reads types, offsets and conn only.
 * spray_rt_cell_isosurface_host is spray_rt_tet_isosurface_host of that list,
 * and what the kernels write, byte for byte. */
int spray_rt_cell_split_host(const spray_rt_cellmesh* mesh, size_t* ntets, uint32_t* tets_out);
int spray_rt_cell_isosurface_host(const spray_rt_cellmesh* mesh, const spray_rt_grid_color* gcolor,
                                  size_t* nverts, size_t* nfaces, float* verts_out,
                                  float* vnormals_out, uint32_t* colors_out, uint32_t* faces_out);
/* ---- boundary surfaces and thresholds of cell meshes ---- */
/* Which cells of a spray_rt_cellmesh a surface extraction keeps. */
#define SPRAY_RT_SELECT_ALL    0  /* every cell */
#define SPRAY_RT_SELECT_POINTS 1  /* cells all of whose points have lo <= values[p] <= hi */
#define SPRAY_RT_SELECT_CELLS  2  /* cells with lo <= cell_values[i] <= hi */
typedef struct spray_rt_cell_select {
  const float* cell_values;  /* [ncells], device or host; read in mode CELLS only */
  float lo, hi;              /* lo <= hi, both finite (modes POINTS, CELLS) */
  int32_t mode;
} spray_rt_cell_select;
/* The outer surface of the kept cells of a mesh, as an indexed triangle mesh
 * over the mesh's own points: with SPRAY_RT_SELECT_ALL the mesh's boundary,
 * with a range the threshold solid with its cut faces.  The rule is fixed, so
 * that the kernels and the host restatement agree byte for byte (DESIGN.md
 * section 16).  mesh.isovalue is ignored; mesh.values is read, and may be NULL
 * otherwise, only in mode POINTS.
 *
 * Kept cells: all; those whose listed points all have lo <= values[p] &&
 * values[p] <= hi; those with lo <= cell_values[i] && cell_values[i] <= hi.
 * Only kept cells have faces: a hex, wedge or pyramid those of the tables of
 * spray_rt_cell_isosurface in their order, a tet (0,1,2) (0,1,3) (1,2,3)
 * (2,0,3).  With c[i] = P[q[i]] the point indices of a face and j the position
 * of the smallest (the lowest j on ties), a triangle has a = c[(j+1)%3], b =
 * c[(j+2)%3], a quad a = c[(j+1)%4], b = c[(j+3)%4], and the face's key is its
 * corner count with the triple (c[j], min(a,b), max(a,b)).  A face is on the
 * surface when its key occurs exactly once among the kept cells' faces of its
 * mesh; keys that occur twice or more are dropped, duplicate cells included.
 * Faces match only as whole faces: a triangle never matches a quad, so where a
 * quad of one cell meets the two triangles of a split neighbour (a
 * non-conforming interface), along either diagonal, all three faces are
 * emitted, as VTK's surface filter does.
 *
 * Vertices are the distinct points the surviving faces use, ascending by point
 * index: position and normal are the point's own bytes, the colour is
 * map(g[p]) with spray_rt_grid_color's rule (its field is [npoints]) or
 * color_rgb, and point_ids[v] is the point's index, so that a caller can gather
 * another field, map it with spray_rt_colormap_apply and recolour the slot with
 * spray_rt_domains_recolor.  Triangles come per cell in input order, then per
 * face in table order: a triangle face is (c0,c1,c2); a quad gives (r0,r1,r2)
 * then (r0,r2,r3) with r_d = c[(j+d)%4], the diagonal of the tet split of
 * spray_rt_cell_isosurface, so the surface is exactly the boundary of that
 * split and an isosurface of the same mesh meets it without cracks.  Faces are
 * turned outward from the geometry: with pref the cell's point at the lowest
 * local position not on the face and det = dot(cross(p1 - p0, p2 - p0), pref -
 * p0) on the face's first triangle, term by term in float as for the tets'
 * parity, det < 0 swaps the last two corners of the face's one or two
 * triangles; then Ng = (v0 - v1) x (v2 - v0) points away from pref.  det == 0
 * and NaN leave the listed order; one decision per face.  A cell that lists a
 * point twice goes through the same rule; zero-area triangles are kept.  No
 * atomic and no hash decides an index: two runs give the same bytes.
 *
 * spray_rt_cell_surface has the argument shapes and NULL conventions of
 * spray_rt_cell_isosurface, with selects (NULL: every cell of every mesh) and
 * point_ids beside them: any output or single entry may be NULL, all NULL only
 * counts, a capacity that is too small gives SPRAY_RT_ERR_LIMIT with the
 * counts reported and no buffer written.  Two host reads per call: status and
 * the face-instance totals, then the vertex and triangle counts.
 *
 * SPRAY_RT_ERR_ARG, before anything is written and naming the mesh: an unknown
 * mode, lo > hi or a non-finite bound (modes POINTS and CELLS), a NULL array
 * the mode reads (ncells == 0 reads nothing and gives the empty surface), a
 * bad colour map, vnormals[i] non-NULL for a mesh without point_normals, and
 * for every cell, kept or not: an unknown type, offsets that do not match it
 * or pass nconn, a point index >= npoints, a non-finite value among what the
 * call reads of a referenced point (coordinates, values in mode POINTS, the
 * colour sample of a mapped mesh, the normal where normals are written), a
 * non-finite cell_values[i] in mode CELLS.  Points no cell references are
 * never read.  SPRAY_RT_ERR_LIMIT: npoints > 2^21 (the three-index key must
 * fit 64 bits; a two-pass sort for larger meshes is left out on purpose),
 * ncells >= 2^29, nconn >= 2^32, 2^32 or more face instances in one call, more
 * than 65,535 meshes. */
int spray_rt_cell_surface(spray_rt_ctx_t ctx, int n, const spray_rt_cellmesh* meshes,
                          const spray_rt_cell_select* selects, const spray_rt_grid_color* gcolors,
                          float* const* verts, float* const* vnormals, uint32_t* const* colors,
                          uint32_t* const* point_ids, uint32_t* const* faces,
                          const size_t* cap_verts, const size_t* cap_faces, size_t* nverts_out,
                          size_t* nfaces_out);
/* Meshes in, resident slots out, as spray_rt_domains_cell_isosurface: slots[i]
 * is byte for byte a slot of spray_rt_domains_build of the extracted mesh.  At
 * most four host reads (the extraction's two and the build's two).  A failed
 * call leaves every slot as it was; messages name the mesh and its slot.  Not
 * for use while lanes run. */
int spray_rt_domains_cell_surface(spray_rt_ctx_t ctx, int n, const int* slots,
                                  const spray_rt_cellmesh* meshes,
                                  const spray_rt_cell_select* selects,
                                  const spray_rt_grid_color* gcolors, int with_normals,
                                  float* d_bounds, size_t* nfaces_out);
/* Host-only restatement (no GPU; every array is host memory): the arrays the
 * kernels write, byte for byte.  select and gcolor may be NULL; any output may
 * be NULL; vnormals_out needs point_normals. */
int spray_rt_cell_surface_host(const spray_rt_cellmesh* mesh, const spray_rt_cell_select* select,
                               const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                               float* verts_out, float* vnormals_out, uint32_t* colors_out,
                               uint32_t* point_ids_out, uint32_t* faces_out);
/* Where the last surface extraction of the context spent its time, as
 * spray_rt_tet_phase_times (the sort's device time while
 * spray_rt_tet_set_timing is on). */
int spray_rt_cell_surface_phase_times(spray_rt_ctx_t ctx, double out_ms[4]);
/* ---- clips of cell meshes by a level of their scalar field ---- */
/* The surface of the part of a spray_rt_cellmesh on one side of values ==
 * isovalue, as one indexed triangle mesh with a smooth cut face.  The rule is
 * fixed, so that the kernels and the host restatement agree byte for byte
 * (DESIGN.md section 17).
 *
 * Kept points: point p is kept when values[p] >= isovalue, with invert[i] != 0
 * when it is not.  The solid is the kept side of the piecewise-linear
 * interpolant over the tet split of spray_rt_cell_isosurface; its surface is a
 * cap, the isosurface, and a skin, the part of the mesh's boundary on the kept
 * side.
 *
 * Vertices come in two groups.  The first ncap_verts are exactly the vertices
 * of spray_rt_cell_isosurface of the same mesh, byte for byte (positions,
 * normals, colours), ascending by pair, whatever invert says; vert_pairs[v] =
 * (a, b), a < b, the vertex's point pair, and vert_t[v] = (isovalue -
 * values[a]) / (values[b] - values[a]).  Then come the kept points that some
 * skin piece uses, ascending by point index: position and normal are the
 * point's own bytes, the colour is map(g[p]) or color_rgb as for
 * spray_rt_cell_surface, vert_pairs[v] = (p, p) and vert_t[v] = 0.  Another
 * field h gathered as h[a] + t * (h[b] - h[a]) in float and mapped with
 * spray_rt_colormap_apply recolours the slot through spray_rt_domains_recolor.
 *
 * Faces come in two groups.  The first ncap_faces are the faces of
 * spray_rt_cell_isosurface, byte for byte, with corners 1 and 2 of each swapped
 * where invert is set: Ng = (v0 - v1) x (v2 - v0) points out of the solid in
 * both cases.  Then comes the skin.  A cell takes part when at least one of its
 * listed points is kept; the skin's source is the triangles of
 * spray_rt_cell_surface (SPRAY_RT_SELECT_ALL) over the cells that take part:
 * face tables, keys, "occurs exactly once", the quad diagonal and the outward
 * turn decided once per face are all that call's.  (A face that a cell without
 * a kept point would have cancelled has no kept corner and gives nothing.)
 * Each such triangle (v0, v1, v2), after the outward turn, is cut by the kept
 * bits of its corners; with P_i the vertex of the kept point v_i, X(i,j) the
 * cap vertex of the pair of corners i and j, and indices mod 3:
 *   3 kept       (P_0, P_1, P_2)
 *   0 kept       nothing
 *   only k       (P_k, X(k,k+1), X(k,k+2))
 *   all but k    (P_{k+1}, P_{k+2}, X(k+2,k)) then (P_{k+1}, X(k+2,k), X(k,k+1))
 * Skin faces are ordered by cell in input order, then face in table order,
 * then the triangle of a quad, then the piece.  Zero-area pieces are kept (a
 * value equal to the isovalue gives t of 0 or 1); a cell that lists a point
 * twice goes through the same rule.  Every edge of a boundary triangle is an
 * edge of a tet of the split, so every X is one of the cap's welded vertices.
 * No atomic and no hash decides an index: two runs give the same bytes.
 *
 * Normals: cap and skin share the vertices along the cut, so with point
 * normals the shading normal there is the interpolated one on both sides;
 * callers who want a crease along the cut pass with_normals = 0 (vnormals
 * NULL).
 *
 * spray_rt_cell_clip has the argument shapes and NULL conventions of
 * spray_rt_cell_surface, with invert (int32 [n], NULL: no mesh inverted),
 * vert_pairs ([nverts][2] uint32) and vert_t ([nverts] float) beside them: any
 * output or single entry may be NULL, all NULL only counts, a capacity (cap and
 * skin together) that is too small gives SPRAY_RT_ERR_LIMIT with the four
 * counts reported and no buffer written.  nverts_out / nfaces_out are the
 * totals, ncap_verts_out / ncap_faces_out the cap's share of them.  Five host
 * reads per call: spray_rt_cell_isosurface's three, the skin's status and
 * face-instance totals, its vertex and piece counts.
 *
 * Errors, before anything is written and naming the mesh: every
 * SPRAY_RT_ERR_ARG and SPRAY_RT_ERR_LIMIT of spray_rt_cell_isosurface and of
 * spray_rt_cell_surface (npoints > 2^21 among them), checked for every cell
 * whether it takes part or not; values is required.  A cut edge without a cap
 * vertex cannot occur on input that passed these checks; the lookup is bounded
 * all the same, never indexes with a miss, and reports SPRAY_RT_ERR_STATE. */
int spray_rt_cell_clip(spray_rt_ctx_t ctx, int n, const spray_rt_cellmesh* meshes,
                       const int32_t* invert, const spray_rt_grid_color* gcolors,
                       float* const* verts, float* const* vnormals, uint32_t* const* colors,
                       uint32_t* const* vert_pairs, float* const* vert_t, uint32_t* const* faces,
                       const size_t* cap_verts, const size_t* cap_faces, size_t* nverts_out,
                       size_t* nfaces_out, size_t* ncap_verts_out, size_t* ncap_faces_out);
/* Meshes in, resident slots out, as spray_rt_domains_cell_surface: slots[i] is
 * byte for byte a slot of spray_rt_domains_build of the clipped mesh.  At most
 * seven host reads (the extraction's five and the build's two).  A failed call
 * leaves every slot as it was; messages name the mesh and its slot.  Not for
 * use while lanes run. */
int spray_rt_domains_cell_clip(spray_rt_ctx_t ctx, int n, const int* slots,
                               const spray_rt_cellmesh* meshes, const int32_t* invert,
                               const spray_rt_grid_color* gcolors, int with_normals,
                               float* d_bounds, size_t* nfaces_out);
/* Host-only restatement (no GPU; every array is host memory): the arrays the
 * kernels write, byte for byte.  gcolor may be NULL; any output may be NULL;
 * vnormals_out needs point_normals. */
int spray_rt_cell_clip_host(const spray_rt_cellmesh* mesh, int32_t invert,
                            const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                            size_t* ncap_verts, size_t* ncap_faces, float* verts_out,
                            float* vnormals_out, uint32_t* colors_out, uint32_t* vert_pairs_out,
                            float* vert_t_out, uint32_t* faces_out);
/* Where the last clip of the context spent its time.  out_ms[0..4] are
 * spray_rt_cell_phase_times' boundaries for the cap: [0] wall clock from entry
 * to the cell pass's host read, [1] from there to the tet count's read, [2] to
 * the weld's read, [3] the enqueue of the cap's and the skin's emit passes,
 * [4] the device time of the two sorts, the cap's pairs and the skin's faces
 * (0 unless spray_rt_tet_set_timing is on).  out_ms[5] is the wall clock of
 * the skin passes between the weld's read and the skin's second read: count,
 * keys, sort, unique, skin count and both reads. */
int spray_rt_cell_clip_phase_times(spray_rt_ctx_t ctx, double out_ms[6]);
/* The signed distance field of a plane, scaled by the normal's length, as the
 * values of a clip ("clip by a plane": spray_rt_cell_clip at isovalue 0 keeps
 * the side the normal points to) or of an isosurface ("slice by a plane":
 * spray_rt_cell_isosurface at isovalue 0):
 *   values[p] = ((px - ox) * nx + (py - oy) * ny) + (pz - oz) * nz
 * in float, term by term.  points ([npoints][3]) may be device or host memory;
 * values_out is device memory.  SPRAY_RT_ERR_ARG for a non-finite origin or
 * normal, a zero normal, or a NULL pointer with npoints > 0.  The host form
 * writes host memory. */
int spray_rt_plane_values(spray_rt_ctx_t ctx, const float* points, size_t npoints,
                          const float origin[3], const float normal[3], float* values_out);
int spray_rt_plane_values_host(const float* points, size_t npoints, const float origin[3],
                               const float normal[3], float* values_out);
/* ---- streamlines of vector grids, as polylines and as tubes ---- */
#define SPRAY_RT_STREAM_FORWARD 0
#define SPRAY_RT_STREAM_BACKWARD 1
#define SPRAY_RT_STREAM_BOTH 2
#define SPRAY_RT_LINE_END_GRID 0  /* a stage point or the new point left the grid (or was not finite) */
#define SPRAY_RT_LINE_END_STEPS 1 /* max_steps taken */
#define SPRAY_RT_LINE_END_SPEED 2 /* speed unusable at the point, or the step moved nothing */
#define SPRAY_RT_LINE_END_SEED 3  /* the seed is outside the grid: the line has no points */
/* One structured grid of vectors, the seeds to trace from and how. */
typedef struct spray_rt_vecfield {
  const float* vectors; /* [nz][ny][nx][3], x fastest; device or host memory */
  int32_t dims[3];      /* as spray_rt_grid */
  float origin[3];
  float spacing[3];
  const float* seeds;   /* [nseeds][3] world positions; device or host memory */
  size_t nseeds;
  float step;           /* > 0, time units: fixed-step classical RK4 of dx/dt = v(x) */
  int32_t max_steps;    /* 0 .. 65535 per direction */
  int32_t direction;    /* SPRAY_RT_STREAM_* */
  float min_speed;      /* > 0, min_speed * min_speed a normal float */
} spray_rt_vecfield;
/* The tube drawn round every line of a field. */
typedef struct spray_rt_tube {
  float radius;         /* > 0, finite */
  int32_t nsides;       /* 3 .. 16 */
  uint32_t color_rgb;   /* one colour for every vertex ... */
  int32_t has_color;    /* ... or none (spray_rt_domains_stream_tubes only) */
} spray_rt_tube;
/* The rule is fixed, so that the kernels and the host restatement agree byte
 * for byte: float, no contraction, division and square
 * root correctly rounded; lerp(a, b, t) = a + t * (b - a).
 *
 * Sample v(p).  Per axis g = (p - origin) / spacing; p is inside when g >= 0 &&
 * g <= float(n - 1) on all three axes (a NaN fails).  i = min(int(floorf(g)),
 * n - 2), f = g - float(i): a point on the upper face uses the last cell with
 * f == 1.  The trilinear value per component: the four x-lerps of the cell's
 * corner pairs (in the order y0z0, y1z0, y0z1, y1z1), the two y-lerps, the
 * z-lerp.
 *
 * Step.  h = +step forward, -step backward, hh = 0.5f * h, h6 = h / 6.0f;
 * k1 = v(p); q2 = p + hh * k1, k2 = v(q2); q3 = p + hh * k2, k3 = v(q3);
 * q4 = p + h * k3, k4 = v(q4); p' = p + h6 * (((k1 + 2 * k2) + 2 * k3) + k4).
 * The speed at p is usable when msq <= d < inf, d = (k1x * k1x + k1y * k1y) +
 * k1z * k1z, msq = min_speed * min_speed.  The step is taken when the speed is
 * usable, q2, q3, q4 and p' are inside, p' differs from p in some bit and
 * fewer than max_steps steps have been taken; otherwise the half-line ends at
 * p, with the first reason that applies of SPEED, GRID, SPEED (no motion),
 * STEPS, in that order.
 *
 * Lines.  Seed s of a field gives line s: the backward half's points in reverse
 * order, the seed, the forward half's points.  A seed outside the grid gives an
 * empty line with both end reasons SEED; a half the direction leaves out has
 * no points and the end reason STEPS.  line_offsets[s] is the line's first
 * point, line_offsets[nseeds] the number of points; line_info[s] = {nback,
 * end_back | end_fwd << 8}, nback the points in front of the seed.
 *
 * Tangent and frame.  T = k1 / sqrtf(d) per component at a point whose speed
 * is usable, else the tangent of the neighbouring point nearer the seed.  At
 * the seed N is the normalised e - T_a * T, e the unit vector of the axis a
 * with the smallest |T_a| (the lowest axis on a tie); along each half
 * w = N_prev - dot(N_prev, T) * T, and N is the normalised w if dot(w, w) >=
 * 0.25f, else the axis rule again.  dot(a, b) = (ax * bx + ay * by) + az * bz,
 * normalised x = x / sqrtf(dot(x, x)) per component, B = T x N (each
 * component a difference of two products).
 *
 * Tube.  A line of m >= 2 points gives m * nsides + 2 vertices and 2 * nsides *
 * m faces, lines of fewer points nothing.  Ring vertex k of point j is vertex
 * j * nsides + k: off = c_k * N + s_k * B per component, position p_j + radius *
 * off, normal off, colour map(g(p_j)) with the colour field g sampled like v
 * (spray_rt_grid_color), else color_rgb; (c_k, s_k) = spray_rt_tube_ring_host.
 * Then the cap centres m * nsides (p_first, normal -T) and m * nsides + 1
 * (p_last, normal +T).  Faces: for segment j and side k, with a = (j, k), b =
 * (j, k + 1 mod nsides), c = (j + 1, k), d = (j + 1, k + 1 mod nsides), the
 * triangles (a, c, b) and (b, c, d); then the first cap's fan (centre, (0, k),
 * (0, k + 1)) for every k, then the last cap's (centre, (m - 1, k + 1), (m - 1,
 * k)): Ng = (v0 - v1) x (v2 - v0) points away from the tube.  Vertex numbers
 * count through a field: output order is line, point, side.  No atomic decides
 * an index, two runs give the same bytes.
 *
 * spray_rt_streamlines traces n fields in one batched call on the context's
 * stream into the caller's device buffers: points[i] float [cap_points[i]][3],
 * line_offsets[i] uint32 [nseeds + 1], line_info[i] uint32 [nseeds][2]; any of
 * the arrays, or single entries, may be NULL.  npoints_out (host, optional) is
 * written on return: the call's one host read.  points == NULL only counts.  A
 * capacity that is too small gives SPRAY_RT_ERR_LIMIT with the counts reported
 * and nothing written.
 *
 * Errors, before anything is written, naming the field: SPRAY_RT_ERR_ARG for a
 * NULL pointer with a nonzero count, dims < 2, a bad spacing, origin, step,
 * min_speed, radius, nsides or direction, max_steps out of range, a non-finite
 * seed coordinate, vector sample or colour sample (found by a check pass,
 * reported at the host read), the colour map errors of
 * spray_rt_isosurface_mapped; SPRAY_RT_ERR_LIMIT for 2^31 or more points in a
 * grid, 2^31 or more seeds, 2^32 or more points of lines, 2^32 or more
 * vertices, 2^29 or more faces. */
int spray_rt_streamlines(spray_rt_ctx_t ctx, int n, const spray_rt_vecfield* fields,
                         float* const* points, uint32_t* const* line_offsets,
                         uint32_t* const* line_info, const size_t* cap_points,
                         size_t* npoints_out);
/* The tubes of n fields into the caller's device buffers, with the conventions
 * of spray_rt_isosurface_mapped: verts / vnormals / colors / faces, or single
 * entries, may be NULL independently, all NULL only counts; gcolors (optional)
 * is an array of colour maps over the fields' dims, a field without one takes
 * color_rgb.  One host read. */
int spray_rt_stream_tubes(spray_rt_ctx_t ctx, int n, const spray_rt_vecfield* fields,
                          const spray_rt_tube* tubes, const spray_rt_grid_color* gcolors,
                          float* const* verts, float* const* vnormals, uint32_t* const* colors,
                          uint32_t* const* faces, const size_t* cap_verts, const size_t* cap_faces,
                          size_t* nverts_out, size_t* nfaces_out);
/* Fields in, resident slots out: afterwards slots[i] is a slot of
 * spray_rt_domains_build of the tube mesh of fields[i] (with its normals if
 * with_normals, its colours if it has a colour field or has_color), byte for
 * byte.  d_bounds and nfaces_out as in spray_rt_domains_isosurface.  At most
 * three host reads (the counts, and the build's two).  A failed call leaves
 * every slot as it was; the errors above, a bad slot or a slot listed twice
 * (SPRAY_RT_ERR_ARG), and the build's.  spray_rt_last_error names the field and
 * the slot.  A field without tubes gives the empty slot an empty upload gives.
 * Not for use while lanes run. */
int spray_rt_domains_stream_tubes(spray_rt_ctx_t ctx, int n, const int* slots,
                                  const spray_rt_vecfield* fields, const spray_rt_tube* tubes,
                                  const spray_rt_grid_color* gcolors, int with_normals,
                                  float* d_bounds, size_t* nfaces_out);
/* Host-only restatements (no GPU; the arrays are host memory): the arrays the
 * kernels write, byte for byte.  The sizes are always reported; any output may
 * be NULL (points_out float[*npoints][3], line_offsets_out uint32[nseeds + 1],
 * line_info_out uint32[nseeds][2]; verts_out / vnormals_out float[*nverts][3],
 * colors_out uint32[*nverts], faces_out uint32[*nfaces][3]).  gcolor may be
 * NULL. */
int spray_rt_streamlines_host(const spray_rt_vecfield* field, size_t* npoints, float* points_out,
                              uint32_t* line_offsets_out, uint32_t* line_info_out);
int spray_rt_stream_tubes_host(const spray_rt_vecfield* field, const spray_rt_tube* tube,
                               const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                               float* verts_out, float* vnormals_out, uint32_t* colors_out,
                               uint32_t* faces_out);
/* The cross-section table the tubes use: out[k] = {(float)cos(a), (float)sin(a)},
 * a = (6.283185307179586 * k) / nsides evaluated in double, k < nsides (3 ..
 * 16): exposed so that a restatement need not reproduce libm. */
int spray_rt_tube_ring_host(int32_t nsides, float out[][2]);
/* Wall-clock milliseconds of the last streamline call of the context:
 * out_ms[0] to the end of the host read (staging, the check pass, the count
 * pass: the first integration), [1] the second integration and the expansion
 * (their enqueue; completed where an array was staged from the host), [2] the
 * device build of the domains form (its two host reads wait for [1]'s work). */
int spray_rt_stream_phase_times(spray_rt_ctx_t ctx, double out_ms[3]);
/* ---- streamlines across the blocks of a multi-block vector field ---- */
/* One block of a set: a structured grid of vectors as in spray_rt_vecfield. */
typedef struct spray_rt_vecblock {
  const float* vectors;     /* [nz][ny][nx][3], x fastest; device or host memory */
  const float* color_field; /* optional [nz][ny][nx]; all blocks of a set have one, or none */
  int32_t dims[3];          /* each >= 2 */
  float origin[3];
  float spacing[3];
} spray_rt_vecblock;
/* A set of blocks, the seeds to trace from and how.  Blocks may differ in dims
 * and spacing, share a face plane, overlap or leave gaps. */
typedef struct spray_rt_blockfield {
  const spray_rt_vecblock* blocks; /* host array */
  int32_t nblocks;                 /* 1 .. 65535 */
  const float* seeds;              /* [nseeds][3] world positions; device or host memory */
  size_t nseeds;
  float step;                      /* the four as in spray_rt_vecfield */
  int32_t max_steps;
  int32_t direction;
  float min_speed;
} spray_rt_blockfield;
/* The colour map of a set whose blocks have colour fields: the table of
 * spray_rt_grid_color. */
typedef struct spray_rt_block_color {
  const uint32_t* table_rgb; /* NULL: the set has no map */
  int32_t ntable;
  float lo, hi;
} spray_rt_block_color;
/* The rule is the streamlines' above, unchanged: sample, step, end reasons and
 * their order, lines, tangent and frame, tube, ring table.  Only "which grid"
 * changes.  A half-line carries a current block b.  A
 * sample at q is taken in b if q is inside b by the test above (0 <= g <=
 * float(n - 1) on all axes with b's origin, spacing and dims; a NaN fails);
 * otherwise in the lowest-indexed block of the set that q is inside, and that
 * block becomes the current one; if q is inside no block the sample fails as a
 * sample outside the grid does above: a seed inside no block gives SEED, a
 * stage point or p' inside no block gives GRID.  The current block is updated
 * at every successful locate in program order q2, q3, q4, p', so the block
 * that p's frame, colour and next k1 are sampled in is the one p was located
 * in as p'.  Both halves of a line start from the lowest-indexed block that
 * contains the seed.  The colour of a point is map(g(p)), g the trilinear
 * sample of its block's color_field, else color_rgb.
 *
 * A set of one block gives the bytes of spray_rt_streamlines and
 * spray_rt_stream_tubes on that grid.  Index sub-boxes of a grid with origin 0
 * and power-of-two spacings, sharing planes, give the unsplit grid's bytes as
 * long as no located point lies exactly on a shared plane: p - origin is then
 * exact, so g, the cell and f are the same real numbers in either.
 *
 * spray_rt_block_streamlines, spray_rt_block_stream_tubes and
 * spray_rt_domains_block_stream_tubes are spray_rt_streamlines,
 * spray_rt_stream_tubes and spray_rt_domains_stream_tubes over n sets, with
 * their conventions: NULL arrays or entries, counting only, one host read (at
 * most three for the domains form), SPRAY_RT_ERR_LIMIT with the counts reported
 * and nothing written, failed calls leaving buffers and slots as they were.
 * point_blocks[i] (optional) is uint32 [cap_points[i]]: the block each point
 * was sampled in.  bcolors (optional) is one spray_rt_block_color per set.  A
 * whole set's tubes go into one slot.
 *
 * Errors are the streamlines', spray_rt_last_error naming the set and, where
 * one is at fault, the block; also SPRAY_RT_ERR_ARG for nblocks outside 1 ..
 * 65535, NULL blocks or block vectors, colour fields on some blocks of a set
 * but not on all, a bcolors entry with a table for a set whose blocks have no
 * colour field; SPRAY_RT_ERR_LIMIT for 2^31 or more points in one block. */
int spray_rt_block_streamlines(spray_rt_ctx_t ctx, int n, const spray_rt_blockfield* sets,
                               float* const* points, uint32_t* const* line_offsets,
                               uint32_t* const* line_info, uint32_t* const* point_blocks,
                               const size_t* cap_points, size_t* npoints_out);
int spray_rt_block_stream_tubes(spray_rt_ctx_t ctx, int n, const spray_rt_blockfield* sets,
                                const spray_rt_tube* tubes, const spray_rt_block_color* bcolors,
                                float* const* verts, float* const* vnormals,
                                uint32_t* const* colors, uint32_t* const* faces,
                                const size_t* cap_verts, const size_t* cap_faces,
                                size_t* nverts_out, size_t* nfaces_out);
int spray_rt_domains_block_stream_tubes(spray_rt_ctx_t ctx, int n, const int* slots,
                                        const spray_rt_blockfield* sets,
                                        const spray_rt_tube* tubes,
                                        const spray_rt_block_color* bcolors, int with_normals,
                                        float* d_bounds, size_t* nfaces_out);
/* Host-only restatements of one set (no GPU; every array is host memory): the
 * arrays the kernels write, byte for byte, as spray_rt_streamlines_host and
 * spray_rt_stream_tubes_host; point_blocks_out uint32[*npoints].  bcolor may be
 * NULL. */
int spray_rt_block_streamlines_host(const spray_rt_blockfield* set, size_t* npoints,
                                    float* points_out, uint32_t* line_offsets_out,
                                    uint32_t* line_info_out, uint32_t* point_blocks_out);
int spray_rt_block_stream_tubes_host(const spray_rt_blockfield* set, const spray_rt_tube* tube,
                                     const spray_rt_block_color* bcolor, size_t* nverts,
                                     size_t* nfaces, float* verts_out, float* vnormals_out,
                                     uint32_t* colors_out, uint32_t* faces_out);
/* spray_rt_stream_phase_times of the last block streamline call. */
int spray_rt_block_stream_phase_times(spray_rt_ctx_t ctx, double out_ms[3]);
/* ---- glyphs of point sets: spheres and arrows ---- */
#define SPRAY_RT_GLYPH_SPHERE 0
#define SPRAY_RT_GLYPH_ARROW  1
/* One set of points, what a particle code leaves in HBM, and which of them to
 * draw. */
typedef struct spray_rt_pointset {
  const float* points;   /* [npoints][3]; device or host memory */
  size_t npoints;
  const float* vectors;  /* [npoints][3] or NULL; required for ARROW */
  const float* scales;   /* [npoints] or NULL: per-point factor, finite, >= 0 */
  const float* select;   /* [npoints] or NULL: kept when select_lo <= v <= select_hi */
  float select_lo, select_hi; /* read with select only */
  uint32_t stride;       /* >= 1: only points with i % stride == 0 are candidates */
} spray_rt_pointset;
/* The glyph drawn at every kept point of a set. */
typedef struct spray_rt_glyph {
  int32_t shape;            /* SPRAY_RT_GLYPH_* */
  float size;               /* > 0, finite: sphere radius / arrow length unit */
  int32_t level;            /* SPHERE: icosphere level 0..3 (20, 80, 320, 1280 faces) */
  int32_t nsides;           /* ARROW: 3..16 */
  int32_t scale_by_vector;  /* ARROW: length = size * |v| instead of size */
  float min_speed;          /* ARROW: > 0, its square a normal float (as spray_rt_vecfield) */
  uint32_t color_rgb;       /* one colour for every vertex ... */
  int32_t has_color;        /* ... or none (spray_rt_domains_glyphs only) */
} spray_rt_glyph;
/* The rule is fixed, so that the kernels and the host restatement agree byte
 * for byte: float, no contraction, division and square
 * root correctly rounded.  dot, normalised, the cross product and the axis
 * rule are the streamlines' above.
 *
 * Keep.  Point i is a candidate when i % stride == 0 and, with select, when
 * select_lo <= select[i] && select[i] <= select_hi.  Its factor is s = size *
 * scales[i] (size without scales); for an arrow d = (vx * vx + vy * vy) + vz *
 * vz, and with scale_by_vector s = (size * scales[i]) * sqrtf(d).  A candidate
 * is kept when 0 < s && s < inf, and for an arrow when also msq <= d && d <
 * inf, msq = min_speed * min_speed.  A subnormal s is kept; an s that
 * overflows, or is zero, drops the point without an error.
 *
 * Order.  Glyph g is the g-th kept point in point order; point_ids[g] is that
 * point.  Every glyph of a set has V vertices and F faces; its vertex k is
 * vertex g * V + k of the set, its face r face g * F + r = its table row +
 * g * V.  Ng = (v0 - v1) x (v2 - v0) points away from the glyph.  The colour
 * of all V vertices is map(field[i]) (spray_rt_grid_color, field one float per
 * point), else color_rgb.
 *
 * Sphere.  V = 10 * 4^level + 2, F = 20 * 4^level, (u_k, faces) =
 * spray_rt_glyph_sphere_host(level).  Vertex k is at p + s * u_k per
 * component, its normal u_k.
 *
 * Arrow.  T = v / sqrtf(d) per component, N = the axis rule's normal of T, B =
 * T x N, L = s.  rs = 0.03f * L, rh = 0.1f * L, hl = 0.35f * L, ls = L - hl;
 * (c_k, s_k) = spray_rt_tube_ring_host(nsides), off_k = c_k * N + s_k * B per
 * component; cone_k = cn * off_k + ct * T with cn = (float)(0.35 / hypot(0.35,
 * 0.1)), ct = (float)(0.1 / hypot(0.35, 0.1)), both evaluated in double on the
 * host.  V = 4 * nsides + 1; vertex j * nsides + k is
 *   j = 0   p + rs * off_k                normal off_k
 *   j = 1   (p + ls * T) + rs * off_k     normal off_k
 *   j = 2   (p + ls * T) + rh * off_k     normal cone_k
 *   j = 3   p + L * T (for every k)       normal cone_k
 * and vertex 4 * nsides is the tail centre p with normal -T.  F = 6 * nsides:
 * with (j, k) = vertex j * nsides + k and k' = k + 1 mod nsides, for k = 0 ..
 * nsides - 1 the shaft's ((0, k), (1, k), (0, k')) and ((0, k'), (1, k), (1,
 * k')); then the annulus' ((1, k), (2, k), (1, k')) and ((1, k'), (2, k), (2,
 * k')); then the cone's ((2, k), (3, k), (2, k')); then the tail fan's
 * (centre, (0, k), (0, k')).  The nsides tip vertices share one position and
 * differ in their normals.
 *
 * No atomic decides an index, two runs give the same bytes.
 *
 * spray_rt_glyphs expands n sets in one batched call on the context's stream
 * into the caller's device buffers, with the conventions of
 * spray_rt_stream_tubes: verts / vnormals / colors / faces / point_ids, or
 * single entries, may be NULL independently, all NULL only counts; point_ids[i]
 * is uint32 [cap_verts[i] / V] and counts as a per-vertex array for the
 * capacity.  gcolors (optional) is an array of colour maps, field one float per
 * point; a set without one takes color_rgb.  nverts_out / nfaces_out (host,
 * optional) are written on return: the call's one host read.  A capacity that
 * is too small gives SPRAY_RT_ERR_LIMIT with the counts reported and nothing
 * written.
 *
 * Errors, before anything is written, naming the set: SPRAY_RT_ERR_ARG for a
 * NULL pointer with a nonzero count, stride == 0, a bad size, shape, level,
 * nsides or min_speed, with select a range that is not lo <= hi, both finite,
 * ARROW without vectors, the colour map errors of spray_rt_isosurface_mapped;
 * and, found by a check pass and reported at the host read, a non-finite
 * point, vector, scale, select value or colour sample or a negative scale,
 * anywhere in an array the call uses (a sphere set may carry vectors: they are
 * not read).  SPRAY_RT_ERR_LIMIT for 2^31 or more points, 2^32 or more
 * vertices, 2^29 or more faces; a sphere set without select and scales keeps
 * every candidate, so its totals are checked from the counts before an array
 * is read. */
int spray_rt_glyphs(spray_rt_ctx_t ctx, int n, const spray_rt_pointset* sets,
                    const spray_rt_glyph* glyphs, const spray_rt_grid_color* gcolors,
                    float* const* verts, float* const* vnormals, uint32_t* const* colors,
                    uint32_t* const* faces, uint32_t* const* point_ids, const size_t* cap_verts,
                    const size_t* cap_faces, size_t* nverts_out, size_t* nfaces_out);
/* Point sets in, resident slots out: afterwards slots[i] is a slot of
 * spray_rt_domains_build of the glyph mesh of sets[i] (with its normals if
 * with_normals, its colours if it has a colour field or has_color), byte for
 * byte.  d_bounds and nfaces_out as in spray_rt_domains_isosurface.  At most
 * three host reads (the counts, and the build's two).  A failed call leaves
 * every slot as it was; the errors above, a bad slot or a slot listed twice
 * (SPRAY_RT_ERR_ARG), and the build's.  spray_rt_last_error names the set and
 * the slot.  A set that keeps no point gives the empty slot an empty upload
 * gives.  Not for use while lanes run.
 *
 * Moving particles: when the kept set is unchanged from one timestep to the
 * next, the cheap path is spray_rt_glyphs with verts (and vnormals) alone on
 * the new positions, then spray_rt_domains_refit with those device pointers: a
 * refit instead of a build.  That relies on the keep decisions (stride, select,
 * scales, speeds) being the ones the slot was built from; the nverts check
 * catches most mismatches, not all.  Recolouring by another field is the same
 * pattern: spray_rt_glyphs with colors alone, then spray_rt_domains_recolor. */
int spray_rt_domains_glyphs(spray_rt_ctx_t ctx, int n, const int* slots,
                            const spray_rt_pointset* sets, const spray_rt_glyph* glyphs,
                            const spray_rt_grid_color* gcolors, int with_normals, float* d_bounds,
                            size_t* nfaces_out);
/* Host-only restatement (no GPU; the arrays are host memory): the arrays the
 * kernels write, byte for byte.  The sizes are always reported; any output may
 * be NULL (verts_out / vnormals_out float[*nverts][3], colors_out
 * uint32[*nverts], faces_out uint32[*nfaces][3], point_ids_out uint32[*nverts /
 * V]).  gcolor may be NULL. */
int spray_rt_glyphs_host(const spray_rt_pointset* set, const spray_rt_glyph* glyph,
                         const spray_rt_grid_color* gcolor, size_t* nverts, size_t* nfaces,
                         float* verts_out, float* vnormals_out, uint32_t* colors_out,
                         uint32_t* faces_out, uint32_t* point_ids_out);
/* The unit icosphere table the spheres use, level 0 .. 3: exposed so that a
 * restatement need not reproduce it.  Built in double.  Level 0 is the
 * icosahedron on (0, +-1, +-t), (+-1, +-t, 0), (+-t, 0, +-1), t = (1 + sqrt(5)) /
 * 2, in the order (-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t),
 * (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t,
 * 0, 1), each divided by its length, with the faces (0 5 11) (0 1 5) (0 7 1)
 * (0 10 7) (0 11 10) (1 9 5) (5 4 11) (11 2 10) (10 6 7) (7 8 1) (3 4 9)
 * (3 2 4) (3 6 2) (3 8 6) (3 9 8) (4 5 9) (2 11 4) (6 10 2) (8 7 6) (9 1 8).
 * A subdivision keeps the vertices and walks the faces in order: face (a, b,
 * c) asks for the midpoints ab, bc, ca in that order, a new midpoint takes the
 * next vertex number and is 0.5 * (v_lo + v_hi) of the edge's lower- and
 * higher-numbered end divided by its length, and the face becomes (a, ab, ca),
 * (b, bc, ab), (c, ca, bc), (ab, bc, ca).  Every coordinate is cast to float
 * at the end.  *nverts = 10 * 4^level + 2, *nfaces = 20 * 4^level; either
 * output may be NULL.  SPRAY_RT_ERR_ARG for another level. */
int spray_rt_glyph_sphere_host(int32_t level, size_t* nverts, size_t* nfaces, float* verts_out,
                               uint32_t* faces_out);
/* Wall-clock milliseconds of the last glyph call of the context: out_ms[0] to
 * the end of the host read (staging, the check, count and scan passes), [1]
 * the place pass and the expansion (their enqueue; completed where an array
 * was staged from the host), [2] the device build of the domains form (its two
 * host reads wait for [1]'s work). */
int spray_rt_glyph_phase_times(spray_rt_ctx_t ctx, double out_ms[3]);
/* Read back one array of a resident slot (tests, debugging): *nbytes = its
 * size; with out, copied there (cap_bytes >= the size) after the queued work
 * on the context's stream.  Slots without the quantized copy report 0 bytes
 * for QNODES4 and QGRID, slots without normals 0 for NORMALS, slots without
 * colours 0 for COLORS. */
#define SPRAY_RT_SLOT_NODES 0   /* BvhNode[]  */
#define SPRAY_RT_SLOT_TRIS 1    /* float[ntris][12] */
#define SPRAY_RT_SLOT_PRIMS 2   /* uint32[ntris] leaf order -> face */
#define SPRAY_RT_SLOT_QNODES4 3 /* QNode4[], index order */
#define SPRAY_RT_SLOT_QGRID 4   /* float[6] base, scale */
#define SPRAY_RT_SLOT_NORMALS 5 /* float[nverts][3] */
#define SPRAY_RT_SLOT_COLORS 6  /* uint32[nverts] */
#define SPRAY_RT_SLOT_FACES 7   /* uint32[ntris][3] */
int spray_rt_slot_export(spray_rt_ctx_t ctx, int slot, int what, void* out, size_t cap_bytes,
                         size_t* nbytes);
/* SAH cost of the slot's current BVH2, so a caller can tell when refits have
 * degraded the tree enough to rebuild with spray_rt_domain_upload.
 * Sum over nodes, over each non-empty child c, of
 * half_area(c) * (c is a leaf ? its triangle count : 1), divided by half_area of
 * the union of node 0's child boxes.  half_area on the stored padded boxes in
 * float as (dx*dy + dy*dz) + dz*dx; the sum in double, in a fixed order
 * (deterministic).  Synchronises the context's stream. */
int spray_rt_slot_sah(spray_rt_ctx_t ctx, int slot, double* out);

/* ---- Embree-1M-style streams (drop-in) ---- */
int spray_rt_intersect1M(spray_rt_ctx_t ctx, int slot, void* rays, size_t M,
                         size_t stride);
int spray_rt_occluded1M(spray_rt_ctx_t ctx, int slot, void* rays, size_t M,
                        size_t stride);
/* TriMeshBuffer::updateIntersection (src/render/trimesh_buffer.cc:328-360;
 * Scene::updateIntersection, src/render/scene.h:203) over a stream: color
 * (offset 60) and Ns (offset 84) of every record whose geomID marks a hit,
 * from its primID, u and v and slot's mesh -- the epilogue intersect1M
 * fuses.  stride >= 96. */
int spray_rt_update_intersection1M(spray_rt_ctx_t ctx, int slot, void* rays, size_t M,
                                   size_t stride);
/* nseg segments: rays [offsets[i], offsets[i+1]) against slots[i];
 * offsets has nseg+1 entries (host memory). */
int spray_rt_intersect_segments(spray_rt_ctx_t ctx, const int* slots,
                                const size_t* offsets, int nseg, void* rays,
                                size_t stride);
int spray_rt_occluded_segments(spray_rt_ctx_t ctx, const int* slots,
                               const size_t* offsets, int nseg, void* rays,
                               size_t stride);
/* Sorted domain lists: org/dir are [M][3]; ids/ts are [M][maxhits],
 * counts[M] (truncated at maxhits). */
int spray_rt_domains1M(spray_rt_ctx_t ctx, const float* org, const float* dir,
                       size_t M, int* ids, float* ts, int* counts, int maxhits);

/* ---- lanes: concurrent per-thread submission (Scene's const queries) ---- */
/* The reference calls Scene::intersect / occluded / intersectDomains from
 * every OpenMP thread at once against the loaded domain
 * (src/ooc/ooc_pcontext.h:144-157, ooc_tcontext.inl:28-100).  A lane is one
 * host thread's private stream + staging: calls on different lanes of one
 * context may run concurrently; one lane is driven by one thread at a time.
 * They read the context's slot and domain tables, which must not change
 * while lanes run (the reference loads domains inside omp single between
 * barriers).  Host or device ray buffers; the call returns with the results
 * in place (host) or completed on the lane's stream (device). */
typedef struct spray_rt_lane* spray_rt_lane_t;
int spray_rt_lane_create(spray_rt_ctx_t ctx, spray_rt_lane_t* out);
/* The calling thread's last spray_rt_lane_create failure ("" after a
 * success): lane creation never writes the context's shared message, so
 * threads creating lanes concurrently do not race on it. */
const char* spray_rt_lane_create_error(void);
int spray_rt_lane_destroy(spray_rt_lane_t lane);
const char* spray_rt_lane_last_error(spray_rt_lane_t lane);
int spray_rt_lane_intersect1M(spray_rt_lane_t lane, int slot, void* rays, size_t M,
                              size_t stride);
int spray_rt_lane_occluded1M(spray_rt_lane_t lane, int slot, void* rays, size_t M,
                             size_t stride);
int spray_rt_lane_update_intersection1M(spray_rt_lane_t lane, int slot, void* rays, size_t M,
                                        size_t stride);
int spray_rt_lane_domains1M(spray_rt_lane_t lane, const float* org, const float* dir, size_t M,
                            int* ids, float* ts, int* counts, int maxhits);

/* ---- fused scene path (all listed domains in one launch) ---- */
int spray_rt_intersect_scene(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                             size_t M, spray_rt_hit* hits);
int spray_rt_occluded_scene(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                            size_t M, uint8_t* occluded);
/* Same, with per-launch traversal counters (device uint64[3]: node fetches,
 * triangle tests, (ray, domain) visits) accumulated atomically -- the
 * counting build used to verify the canonical traversal against the oracle. */
int spray_rt_intersect_scene_counted(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                     size_t M, spray_rt_hit* hits,
                                     unsigned long long* d_counters);
int spray_rt_occluded_scene_counted(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                    size_t M, uint8_t* occluded,
                                    unsigned long long* d_counters);
/* Closest hit with the point-light shadow spawn of ooc::ShaderPt fused into
 * the epilogue (shade as for spray_rt_spawn_shadows_pt), written
 * positionally: out_valid[i] = 1 and out_rays[i] = the shadow ray when
 * source ray i spawns one, out_valid[i] = 0 otherwise.  *d_count (device
 * uint32, may be NULL) receives the number spawned.  Deterministic.  Device
 * buffers only. */
int spray_rt_intersect_scene_spawn_pt(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                      size_t M, spray_rt_hit* hits,
                                      const float shade[10], spray_rt_ray* out_rays,
                                      uint8_t* out_valid, uint32_t* d_count);
/* Closest hit, PT shadow spawn and the shadow rays' any hit in ONE launch:
 * hits[i] as spray_rt_intersect_scene; sh_valid[i] = 1 when ray i spawned a
 * point-light shadow ray (as spray_rt_intersect_scene_spawn_pt's out_valid),
 * occluded[i] = its any-hit result (written where sh_valid[i]), *d_count
 * (optional, device) = number of shadow rays.  The shadow rays never leave
 * the chip: each wave queues its spawned rays in LDS and traces them as
 * 64-ray packets.  Results equal spawn_pt + occluded_scene_masked.  Device
 * buffers only. */
int spray_rt_intersect_scene_shadow_pt(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                       size_t M, spray_rt_hit* hits, const float shade[10],
                                       uint8_t* occluded, uint8_t* sh_valid,
                                       uint32_t* d_count);
/* Any hit over the rays i < M with valid[i] != 0 (e.g. the positional spawn
 * output): occluded[i] is written for those rays only.  The valid rays are
 * first compacted into an ascending index list (device select), so the
 * traversal runs on full wavefronts in source order.  Device buffers only. */
int spray_rt_occluded_scene_masked(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                   size_t M, const uint8_t* valid,
                                   uint8_t* occluded);
/* Occlusion of the first *d_count (device uint32, e.g. written by
 * spray_rt_spawn_shadows_pt) of at most max_rays device-resident rays, with
 * no host round trip.  d_counters may be NULL. */
int spray_rt_occluded_scene_devcount(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                     size_t max_rays, const uint32_t* d_count,
                                     uint8_t* occluded,
                                     unsigned long long* d_counters);
/* Any hit of the rays order[j], j < *d_count (device count, <= max_rays),
 * lanes taking them in that order; occluded[order[j]] is written (order =
 * NULL: the identity, rays 0 .. *d_count - 1).  The
 * results equal the positional launch's -- only the grouping of rays into
 * wavefronts changes (e.g. spray_rt_spawn_shadows_ao_ordered's order).
 * Device buffers only. */
int spray_rt_occluded_scene_order(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                  size_t max_rays, const uint32_t* order,
                                  const uint32_t* d_count, uint8_t* occluded);

/* ---- traversal form of the any-hit scene launches ---- */
/* Closest-hit scene launches walk each domain tree as a wave-wide packet
 * (one scalar fetch per node per wave).  Any-hit launches follow this
 * setting: COHERENT = packets (camera / point-light shadow rays), INCOHERENT
 * = one walk per lane (hemisphere-sampled AO rays), ADAPTIVE (default) =
 * per wave, packets when every direction is within ~8 degrees of the
 * wave's first.  Results are identical in every mode. */
#define SPRAY_RT_RAYS_ADAPTIVE 0
#define SPRAY_RT_RAYS_COHERENT 1
#define SPRAY_RT_RAYS_INCOHERENT 2
int spray_rt_set_coherence(spray_rt_ctx_t ctx, int mode);

/* What the launcher decided for the last scene launch (any of the
 * spray_rt_*_scene* calls, frames included) of the process, not of ctx: not
 * thread-safe, for tests that must prove which body of the scene kernel
 * they ran.  out = { persist (1: persistent waves over the work queues, 0:
 * one packet per wave), resident-block count of the launched kernel (0 while
 * it was never computed), rays per dequeued chunk of its persistent form,
 * W (64-domain words), stack entries, traversal (0 per lane, 1 packets,
 * 2 adaptive), any hit, epilogue }.  All zero before the first launch. */
int spray_rt_scene_launch_info(spray_rt_ctx_t ctx, int out[8]);

/* ---- in-situ (domain-sharded, one rank per GPU) ---- */
/* Domain -> rank map of the partition (InsituPartition::rank,
 * src/render/data_partition.h:48-56): owner[ndomains] host array, ranks in
 * [0, 64), -1 = nobody.  Reset by spray_rt_domain_bounds. */
int spray_rt_set_owners(spray_rt_ctx_t ctx, const int* owner);
/* Routing of a ray batch (insitu::Isector::intersect,
 * src/insitu/insitu_isector.h:164-224, speculative: every domain on the
 * list): rank_mask[i] = OR of (1 << owner[d]) over the domains d whose box
 * the ray enters.  Device buffers only. */
int spray_rt_route(spray_rt_ctx_t ctx, const spray_rt_ray* rays, size_t M,
                   uint64_t* rank_mask);
/* Exchange plan of a routed batch (the per-destination queues of
 * insitu_comm.inl, built at once): idx = for d = 0..world-1 the ascending
 * indices i with bit d of rank_mask[i], concatenated; starts[0..world] =
 * the list bounds (int64).  idx == NULL computes the bounds only (starts
 * [world] = the capacity idx needs).  Device buffers only. */
int spray_rt_exchange_plan(spray_rt_ctx_t ctx, const uint64_t* rank_mask, size_t n,
                           int world, int64_t* idx, int64_t* starts);
/* Exchange packing: dst[j] = src[idx[j]] for rows of 4, 8, 16, 32 (a ray)
 * or 48 (a hit record) bytes; idx int64.  Device buffers only. */
int spray_rt_gather_rows(spray_rt_ctx_t ctx, const void* src, size_t row_bytes,
                         const int64_t* idx, size_t n, void* dst);
/* Closest hit over the RESIDENT domains of each ray's list (mapped slots;
 * the others are skipped) plus the composite key that orders hits the way
 * the sequential walk of the whole list does:
 *   keys[i] = (bits(t) << 32) | (list position << 16) | domain,
 *   0x7FFFFFFFFFFFFFFF on a miss.
 * The minimum key over all ranks (VBuf tbuf compositing,
 * src/insitu/insitu_vbuf.h:74-152) identifies the hit of the full scene.
 * Device buffers only. */
int spray_rt_intersect_scene_keyed(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                   size_t M, spray_rt_hit* hits, uint64_t* keys);

/* ---- out-of-core (streamed domains, config 4) ---- */
/* An LRU cache of cache_slots domain images in HBM, fed from pinned host
 * memory (LruCache::load, src/render/lru_cache.cc:65-171; Scene::load,
 * src/render/scene.inl:161-187).  Uses the context's domain boxes
 * (spray_rt_domain_bounds first), stream and device. */
typedef struct spray_rt_ooc* spray_rt_ooc_t;
int spray_rt_ooc_create(spray_rt_ctx_t ctx, int cache_slots, spray_rt_ooc_t* out);
int spray_rt_ooc_destroy(spray_rt_ooc_t ooc);
/* TriMeshBuffer::load (trimesh_buffer.cc:117-169) once per domain: the BVH
 * image is built here and kept in pinned host memory. */
int spray_rt_ooc_set_domain(spray_rt_ooc_t ooc, int domain, const float* verts_xyz,
                            size_t nverts, const uint32_t* faces, size_t nfaces,
                            const uint32_t* colors_rgb, const float* vnormals);
/* Closest hit of a device ray batch over every domain of each ray's list,
 * the domains streamed through the cache in ascending id order (queues
 * built on the device, one drain launch per domain).  Same hit records as
 * spray_rt_intersect_scene.  Device buffers only. */
int spray_rt_ooc_intersect(spray_rt_ooc_t ooc, const spray_rt_ray* rays, size_t M,
                           spray_rt_hit* hits);
/* Any hit of the rays with valid[i] != 0 (valid may be NULL), domains in
 * descending order; occluded[i] written for those rays.  Device buffers. */
int spray_rt_ooc_occluded(spray_rt_ooc_t ooc, const spray_rt_ray* rays, size_t M,
                          const uint8_t* valid, uint8_t* occluded);
/* out[4] = cache loads (misses), cache hits, bytes uploaded, drain launches */
int spray_rt_ooc_stats(spray_rt_ooc_t ooc, unsigned long long out[4]);

/* ---- ray sources on the device (caller side of the hot path) ---- */
/* cam[14] = pos[3], lowerleft[3], wvec[3], hvec[3], image_w, image_h
 * (Camera::init, src/render/camera.h:128-166).  ooc::Tracer::genMultiEyes
 * (src/ooc/ooc_tracer.inl:124-172) over blocking tile (tx,ty,tw,th):
 * rays[n], n = tw*th*spp in bufid order; pixid/samid may be NULL.  All
 * device pointers. */
int spray_rt_eye_rays_ooc(spray_rt_ctx_t ctx, const float cam[14], int image_w,
                          int spp, int tx, int ty, int tw, int th,
                          spray_rt_ray* rays, int32_t* pixid, int32_t* samid);
/* insitu::genMultiSampleEyeRays / genSingleSampleEyeRays
 * (src/insitu/insitu_ray.h:103-182): the stripe (tx,ty,tw,th) of blocking
 * tile (bx,by,bw,bh), jitter seeded by (pixid, sample); samid = the
 * blocking-tile-local sample id.  All device pointers. */
int spray_rt_eye_rays_insitu(spray_rt_ctx_t ctx, const float cam[14], int image_w,
                             int spp, int bx, int by, int bw, int bh, int tx, int ty,
                             int tw, int th, spray_rt_ray* rays, int32_t* pixid,
                             int32_t* samid);
/* Point-light shadow rays of ooc::ShaderPt (src/ooc/ooc_shader_pt.h:93-171)
 * for every hit: compacted into out_rays/out_src (source ray index); the
 * number written goes to *d_count (device int, zeroed by the call).
 * shade[8] = light pos[3], light radiance[3]... see DESIGN.md:
 * shade = {lx, ly, lz, lr, lg, lb, ks_r, ks_g, ks_b, shininess}. */
int spray_rt_spawn_shadows_pt(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                              const spray_rt_hit* hits, size_t M,
                              const float shade[10], spray_rt_ray* out_rays,
                              int32_t* out_src, uint32_t* d_count);

/* Ambient-occlusion rays of ooc::ShaderAo (src/ooc/ooc_shader_ao.h:
 * 120-146): nsamples cosine-weighted hemisphere directions per hit, sample l
 * of pixel p seeded by p * (l + 1) (pixid[i] = the ray's pixel), compacted
 * into out_rays/out_src in (source ray, sample) order; *d_count = number
 * written.  out_rays must hold M * nsamples rays.  Device buffers only. */
int spray_rt_spawn_shadows_ao(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                              const spray_rt_hit* hits, const int32_t* pixid, size_t M,
                              int nsamples, spray_rt_ray* out_rays, int32_t* out_src,
                              uint32_t* d_count);
/* The same rays, plus trace_order[0 .. *d_count) (device uint32, room for
 * M * nsamples): a permutation of the written rays for
 * spray_rt_occluded_scene_order.  The reference seeds sample l of every ray
 * of a pixel with pixid * (l + 1), so the spp rays of one pixel draw the same
 * hemisphere samples; within each aligned block of 8 source rays the order
 * is sample-major (l, then ray), which puts rays of nearly the same origin
 * and direction on neighbouring lanes.  (nsamples > 32: identity.) */
int spray_rt_spawn_shadows_ao_ordered(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                      const spray_rt_hit* hits, const int32_t* pixid,
                                      size_t M, int nsamples, spray_rt_ray* out_rays,
                                      int32_t* out_src, uint32_t* d_count,
                                      uint32_t* trace_order);
/* The same rays written directly in that trace order (out_rays[k] and
 * out_src[k] for k < *d_count: a permutation of spray_rt_spawn_shadows_ao's
 * output), for spray_rt_occluded_scene_order with order = NULL: the any-hit
 * lanes then read rays and write occlusion flags contiguously. */
int spray_rt_spawn_shadows_ao_traced(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                     const spray_rt_hit* hits, const int32_t* pixid,
                                     size_t M, int nsamples, spray_rt_ray* out_rays,
                                     int32_t* out_src, uint32_t* d_count);
/* The spawn of spray_rt_spawn_shadows_ao_traced without the rays: entry k
 * of the same trace order is out_pairs[k] = source ray << 5 | sample l,
 * k < *d_count (4 bytes per AO ray instead of 36); lv receives the local
 * hemisphere sample of every (pixel, l) those rays use (the sampler draw
 * and the double-precision sincos, once per pixel and sample), float4 at
 * pixid * nsamples + l, and rec the origin, normal and tangent frame of
 * every source ray that spawns (16 floats at 16 * i).  nsamples <= 32,
 * M < 2^27; out_pairs holds M * nsamples entries, lv npix * nsamples * 4
 * floats, rec M * 16 floats.  A ray whose pixid lies outside [0, npix)
 * spawns no AO ray (its table entries would lie outside lv). */
int spray_rt_spawn_shadows_ao_pairs(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                    const spray_rt_hit* hits, const int32_t* pixid, size_t M,
                                    int nsamples, size_t npix, uint32_t* out_pairs, float* lv,
                                    float* rec, uint32_t* d_count);
/* Scene::occluded of those AO rays (ooc_shader_ao.h:114-160 spawn +
 * scene.inl:201-209), each ray generated in its any-hit lane from
 * (rec[i], lv[pixel * nsamples + l]) with the spawn's operations --
 * the same bits as spawn_shadows_ao_traced + occluded_scene_order(order =
 * NULL), without writing and re-reading 32 B per ray.  occ[k], k <
 * *d_count <= max_n.  d_counters (optional, device u64[3]): the canonical
 * node / triangle / domain-visit counts (counting build). */
int spray_rt_occluded_ao_pairs(spray_rt_ctx_t ctx, size_t max_n, const uint32_t* pairs,
                               const float* rec, const float* lv, int nsamples,
                               const uint32_t* d_count, uint8_t* occ,
                               unsigned long long* d_counters);
/* Both, one call. */
int spray_rt_occluded_ao(spray_rt_ctx_t ctx, const spray_rt_ray* rays, const spray_rt_hit* hits,
                         const int32_t* pixid, size_t M, int nsamples, size_t npix,
                         uint32_t* out_pairs, float* lv, float* rec, uint32_t* d_count,
                         uint8_t* occ, unsigned long long* d_counters);

/* ---- frames: path shading, film, tiles (callers of the hot path) ---- */
/* The shading pass of ooc::ShaderPt (src/ooc/ooc_shader_pt.h:93-227) /
 * ooc::ShaderAo (src/ooc/ooc_shader_ao.h:92-197), the retire-to-image step
 * (ooc_tcontext.inl:123-135 + HdrImage::add, src/display/image.h:90-99), the
 * blocking-tile list (src/render/tile.cc:52-200) and the PPM writer
 * (image.h:167-204), so a whole ooc-mode frame runs on the device. */
#define SPRAY_RT_SHADER_PT 0
#define SPRAY_RT_SHADER_AO 1
#define SPRAY_RT_LIGHT_POINT 0      /* PointLight, src/render/light.h:38-62 */
#define SPRAY_RT_LIGHT_HEMISPHERE 1 /* DiffuseHemisphereLight, light.h:64-90 */
#define SPRAY_RT_BSDF_DIFFUSE 0     /* reflection.h:234-262 */
#define SPRAY_RT_BSDF_MIRROR 1      /* reflection.h:264-287 */
#define SPRAY_RT_BSDF_GLASS 2       /* p = eta_exterior, eta_interior; :292-330 */
#define SPRAY_RT_BSDF_TRANSMISSION 3 /* p = eta_exterior, eta_interior; :335-364 */
#define SPRAY_RT_MAX_LIGHTS 8

typedef struct spray_rt_light {
  int32_t type;
  float pos[3];      /* point lights */
  float radiance[3];
} spray_rt_light;

typedef struct spray_rt_bsdf {
  int32_t type;
  float p[3];
} spray_rt_bsdf;

/* Shader configuration (spray::Config: bounces, ao_samples, ks, shininess;
 * the scene's lights). */
typedef struct spray_rt_shader {
  int32_t shader;   /* SPRAY_RT_SHADER_* */
  int32_t bounces;  /* >= 1 */
  int32_t samples;  /* AO rays per hit / samples per area light */
  int32_t nlights;  /* <= SPRAY_RT_MAX_LIGHTS */
  float ks[3];
  float shininess;
  spray_rt_light lights[SPRAY_RT_MAX_LIGHTS];
} spray_rt_shader;

/* Per-domain BSDFs (Scene::getBsdf(domain), scene_loader.cc:88-130), host
 * array of n entries; domains without an entry are diffuse. */
int spray_rt_set_bsdfs(spray_rt_ctx_t ctx, int n, const spray_rt_bsdf* bsdfs);
/* Shadow rays one path slot can spawn per shading pass (the slot stride of
 * the shadow buffers). */
int spray_rt_shadow_slots(const spray_rt_shader* shader);
/* Closest hit of the rays with valid[i] != 0 (device buffers); hits of the
 * other rays are left as they were. */
int spray_rt_intersect_scene_masked(spray_rt_ctx_t ctx, const spray_rt_ray* rays,
                                    size_t M, const uint8_t* valid, spray_rt_hit* hits);
/* One shading pass over M positional path slots at bounce `bounce` (0 =
 * camera rays).  In: rays[i] (the ray that produced hits[i]), w[i] = path
 * weight (float4, xyz), valid[i].  Out: shadow k of slot i at
 * i*ns + k (ns = spray_rt_shadow_slots) in shadows / sw (float4) /
 * svalid; the next radiance ray in rays[i], w[i], valid[i].  d_stats
 * (device uint64[4], may be NULL) += {cases the reference aborts on (they
 * are skipped), shadow rays spawned, next radiance rays, live slots shaded}.
 * pixid seeds the AO sampler, samid the PT samplers.  Device buffers. */
int spray_rt_shade(spray_rt_ctx_t ctx, const spray_rt_shader* shader, int bounce,
                   spray_rt_ray* rays, const spray_rt_hit* hits, float* w,
                   uint8_t* valid, const int32_t* pixid, const int32_t* samid, size_t M,
                   spray_rt_ray* shadows, float* sw, uint8_t* svalid,
                   unsigned long long* d_stats);
/* image_rgba[pixid] += scale * sw for every unoccluded shadow of the M
 * slots (pixel groups of spp consecutive slots, ns shadows each); float +=
 * double product, in slot then shadow order.  Device buffers. */
int spray_rt_film(spray_rt_ctx_t ctx, float* image_rgba, const int32_t* pixid, size_t M,
                  int spp, int ns, const float* sw, const uint8_t* svalid,
                  const uint8_t* occluded, double scale);
/* One tile of an ooc-mode frame on the device, enqueued on the context's
 * stream (no host synchronisation): eye rays (genMultiEyes), then per
 * bounce closest hit -> shade -> any hit of the shadows -> film.
 * image_rgba: device float[image_w*image_h*4]. */
int spray_rt_render_tile(spray_rt_ctx_t ctx, const spray_rt_shader* shader,
                         const float cam[14], int image_w, int spp, int tx, int ty, int tw,
                         int th, float* image_rgba);
/* Several tiles (tiles[ntiles][4] = x, y, w, h) as one device batch: each
 * tile's eye rays keep their tile-local seeds and every later pass is per
 * sample slot or per pixel, so the image equals rendering the tiles one by
 * one -- with one launch per pass instead of one per tile (the reference's
 * 1M-samples-per-rank tile cap bounds host memory; 288 GB of HBM holds a
 * whole 1024x1024x8 frame's buffers, ~1 GB, many times over). */
int spray_rt_render_tiles(spray_rt_ctx_t ctx, const spray_rt_shader* shader,
                          const float cam[14], int image_w, int spp, const int* tiles,
                          int ntiles, float* image_rgba);
/* Totals of the tiles rendered since the last reset (synchronises the
 * stream): out[3] = radiance rays traced, shadow rays traced, shading cases
 * the reference aborts on (skipped here).  Returns SPRAY_RT_ERR_UNSUPPORTED
 * when out[2] > 0. */
int spray_rt_frame_stats(spray_rt_ctx_t ctx, unsigned long long out[3], int reset);
/* This rank's tiles of the image, tiles[cap][4] = x, y, w, h; *n = count
 * (tiles = NULL, cap = 0: count only).
 *  SPRAY_RT_TILES_IMAGE (ooc mode, ImageScheduleTileList::init, tile.cc:
 *    317-391): the rank's vertical stripe (makeVerticalStripe) cut into
 *    horizontal tiles of at most max_samples_per_rank samples;
 *  SPRAY_RT_TILES_BLOCKING (in-situ mode, TileList::init, tile.cc:52-182):
 *    square-ish blocking tiles of the image, each cut to the rank's
 *    horizontal stripe (makeHorizontalStripe; empty stripes w = h = 0). */
#define SPRAY_RT_TILES_IMAGE 0
#define SPRAY_RT_TILES_BLOCKING 1
int spray_rt_tile_list(int schedule, int image_w, int image_h, int spp, int nranks, int rank,
                       long long max_samples_per_rank, int* tiles, int cap, int* n);
/* HdrImage::writePpm (image.h:167-204): P3, max 1023, bottom row first. */
int spray_rt_write_ppm(const char* path, const float* rgba_host, int w, int h);

/* ---- in-situ frames: the domain-sharded tracer and its exchange ---- */
/* The reference's in-situ mode (src/insitu/): every domain is resident on
 * one rank, rays travel to the owners of the domains on their lists.  The
 * whole per-bounce protocol runs in the engine on the context's stream:
 *   route (Isector::intersect, insitu_isector.h:164-224) -> per-destination
 *   lists -> count exchange -> ray exchange (Comm::run, insitu_comm.inl:
 *   28-101; one grouped ncclSend/ncclRecv all-to-all-v instead of tagged
 *   Isend/Iprobe/Recv) -> keyed closest hit at the owners -> keys back, min
 *   at the ray's holder, the min forward (VBuf::compositeTbuf,
 *   insitu_vbuf.h:109-129, per ray copy) -> the one owner whose key wins
 *   shades (ShaderPt / ShaderAo, insitu_shader_*.h) -> its shadow rays are
 *   routed and exchanged the same way, their occlusion bytes OR-ed back at
 *   the spawner (compositeObuf) -> film (retireShadows) -> the spawned
 *   radiance rays are the spawner's batch of the next bounce.
 * Host round trips per bounce: three small count reads (no per-ray host
 * work).  Collectives go through RCCL (the product: one communicator per
 * in-situ context, spray_rt_insitu_unique_id on rank 0, broadcast by the
 * caller) or, for tests and CPU-side debugging, through host callbacks
 * (spray_rt_transport, buffers staged through host memory). */
typedef struct spray_rt_insitu* spray_rt_insitu_t;

/* Host-memory collectives of the rank group (every rank calls each one in
 * the same order).  Return 0 on success.
 * ABI: this is layout version 2 (SPRAY_RT_TRANSPORT_ABI), which put
 * struct_size in FRONT of `user` -- a breaking change against version 1
 * (round <= 4 callers, `user` at offset 0).  spray_rt_insitu_create reads
 * struct_size before any other field and rejects a value outside
 * [offsetof(allreduce_min_u64), SPRAY_RT_TRANSPORT_MAX_SIZE] with
 * SPRAY_RT_ERR_ARG: a version-1 caller's `user` pointer (or NULL) read as
 * struct_size fails that check instead of shifting every callback.  Within
 * version 2 the struct only grows at its end: a caller's struct_size below
 * sizeof(spray_rt_transport) leaves the later callbacks NULL. */
#define SPRAY_RT_TRANSPORT_ABI 2
#define SPRAY_RT_TRANSPORT_MAX_SIZE 4096
typedef struct spray_rt_transport {
  size_t struct_size;
  void* user;
  /* send_bytes[r] bytes to rank r (consecutive in send), recv_bytes[r] from
   * rank r (consecutive in recv) */
  int (*alltoallv)(void* user, const void* send, const size_t* send_bytes, void* recv,
                   const size_t* recv_bytes);
  int (*allreduce_u64)(void* user, unsigned long long* data, size_t n); /* SUM, in place */
  int (*reduce_f32)(void* user, float* data, size_t n, int root);       /* SUM to root */
  /* replicated-ray frames (spray_rt_insitu_trace_frame); may be NULL, the
   * frame then fails with SPRAY_RT_ERR_UNSUPPORTED */
  int (*allreduce_min_u64)(void* user, unsigned long long* data, size_t n); /* MIN, in place */
  int (*allreduce_sum_u8)(void* user, uint8_t* data, size_t n);            /* SUM, in place */
} spray_rt_transport;

/* Optional per-sample record of a trace (tests, VBuf dumps): for every copy
 * this rank shaded, its sample id, bounce, winning hit and the spawned /
 * occluded bits of its shadow slots (slot k = bit k; <= 64 slots).
 * Appended at *d_count (device, caller-zeroed) in no particular order; the
 * arrays hold cap entries (device memory). */
typedef struct spray_rt_insitu_rec {
  int32_t* samid;
  int32_t* bounce;
  spray_rt_hit* hits;
  unsigned long long* svalid;
  unsigned long long* occluded;
  size_t cap;
  uint32_t* d_count;
} spray_rt_insitu_rec;

/* ncclGetUniqueId for the group's communicator (bytes >= 128). */
int spray_rt_insitu_unique_id(void* id_out, size_t bytes);
/* One in-situ context per rank on ctx (whose domain boxes, owner map
 * (spray_rt_set_owners) and resident slots describe this rank's share).
 * nccl_id != NULL: collectives over RCCL (ncclCommInitRank, blocks until
 * every rank joined); else host != NULL: the given host collectives. */
int spray_rt_insitu_create(spray_rt_ctx_t ctx, int world, int rank, const void* nccl_id,
                           const spray_rt_transport* host, spray_rt_insitu_t* out);
int spray_rt_insitu_destroy(spray_rt_insitu_t ins);
/* InsituPartition::partition, GROUP_CLOSE_DOMAINS (src/render/
 * data_partition.h:59-137): Morton codes of the domain-box centres in the
 * scene bound, sorted by (code, id), dealt out in contiguous shares of
 * ndomains / nranks.  Host only. */
int spray_rt_insitu_partition(const float* boxes, int ndomains, const float scene_bound[6],
                              int nranks, int* owner_out);
/* The same with the partition mode of data_partition.h: GROUP_CLOSE (the
 * contiguous shares above, :118-137, the reference's compiled mode) or
 * ROUND_ROBIN (the sorted Morton order dealt out one domain per rank in
 * turn, "trying to scatter close domains", :139-155). */
#define SPRAY_RT_PARTITION_GROUP_CLOSE 0
#define SPRAY_RT_PARTITION_ROUND_ROBIN 1
int spray_rt_insitu_partition_mode(const float* boxes, int ndomains, const float scene_bound[6],
                                   int nranks, int mode, int* owner_out);
/* This rank's part of a frame: rays[n] / pixid / samid are its eye rays
 * (spray_rt_eye_rays_insitu of its stripe; samid = blocking-tile sample id;
 * tnear SPRAY_RAY_EPSILON and tfar +inf, as every radiance ray of the
 * reference: the exchange does not send the two and the receiver sets them
 * to these values, while the all-local frame of world 1 walks the records as
 * they are, so other extents give results that depend on the route),
 * traced for shader->bounces bounces across the group; the contributions
 * of the samples this rank shades are added to image_rgba (device float
 * [w*h*4], scaled 1/spp).  totals (host, optional): the group's radiance
 * rays, shadow rays and reference-abort cases (the same on every rank).
 * rec (optional): see spray_rt_insitu_rec.  Device buffers only. */
int spray_rt_insitu_trace(spray_rt_insitu_t ins, const spray_rt_shader* shader,
                          const spray_rt_ray* rays, const int32_t* pixid, const int32_t* samid,
                          size_t n, int spp, float* image_rgba, const spray_rt_insitu_rec* rec,
                          unsigned long long totals[3]);
/* The whole frame with replicated eye rays: rays[n] / pixid / samid are
 * EVERY eye ray of the frame (spray_rt_eye_rays_insitu over the whole
 * blocking tile; tnear SPRAY_RAY_EPSILON and tfar +inf, as every radiance
 * ray of the reference), the same on every rank.  Instead of moving rays to
 * their domains' owners, each rank
 *   1. selects C' = the rays that enter the scene's bounding box (a
 *      superset of the rays with a domain on their list, the same ascending
 *      list on every rank);
 *   2. traces C' over its own domains in one launch: keyed closest hit (t,
 *      list position, domain) and the point-light shading of its own hit;
 *   3. joins a MIN all-reduce of the t bits, then of the list positions at
 *      that t (a byte each, beside step 4) -- the sequential walk's winner
 *      of every ray on every rank (VBuf::compositeTbuf, insitu_vbuf.h:
 *      109-129, per ray instead of per tile);
 *   4. any-hits the point-light shadow ray of every hit, built in the lanes
 *      from (org, dir, minimum t) -- the winner's bits -- over its domains;
 *   5. joins one SUM all-reduce of the occlusion bytes over C', the frame
 *      totals riding behind them (compositeObuf + WorkStats::reduce);
 *   6. films the unoccluded shadows of the rays it won into per-run sums
 *      (a run = consecutive rays of C' with one pixel: the spp samples of a
 *      pixel), which one RCCL reduce (12 B per run instead of the 16-B-per-
 *      pixel image) brings to rank 0, where they are added to image_rgba.
 * The WHOLE frame lands in rank 0's image; the other ranks' images are not
 * touched (no spray_rt_insitu_composite needed).  No ray, hit or shadow
 * record crosses the wire and no count is exchanged: three all-reduces, one
 * reduce and one host read per frame.  Results per sample are the
 * protocol's (the same winner, shading and occlusion).
 * AO (ooc::ShaderAo, one bounce, <= 32 samples, diffuse surfaces): after 3.
 * the winners publish their hits' shading normal and colour (one SUM
 * all-reduce, 16 B per ray of C), every rank spawns the same AO rays of
 * every hit and any-hits them over its own domains, one SUM all-reduce of
 * per-sample occlusion count fields (2 / 4 / 8 bits for world <= 3 / 15 /
 * 64) ORs the group's results, and rank 0 films the WHOLE frame (the other
 * ranks' images are not touched: no composite needed).  Three all-reduces
 * and one host read per frame; totals without a collective.
 * Needs one of those two cases and, with host collectives,
 * allreduce_min_u64 / allreduce_sum_u8; SPRAY_RT_ERR_UNSUPPORTED otherwise
 * (trace with spray_rt_insitu_trace).  World 1: the all-local frame. */
int spray_rt_insitu_trace_frame(spray_rt_insitu_t ins, const spray_rt_shader* shader,
                                const spray_rt_ray* rays, const int32_t* pixid,
                                const int32_t* samid, size_t n, int spp, float* image_rgba,
                                const spray_rt_insitu_rec* rec, unsigned long long totals[3]);
/* The replicated-ray frame of a camera (the N > 1 in-situ frame of
 * bench.py): the frame of spray_rt_insitu_trace_frame for the eye rays of
 * the whole image_w x image_h x spp image as one blocking tile
 * (insitu::genMultiSampleEyeRays, insitu_ray.h:103-182; the rays, pixel and
 * sample ids spray_rt_eye_rays_insitu writes for tile = stripe = image),
 * generated in the lanes from cam (spray_camera_init's 14 floats, for
 * that image size) -- no ray buffer.  Each rank's work follows its own
 * domains instead of the frame: the pixels whose eye rays may enter one of
 * its resident domain boxes (the boxes' conservative screen footprints) are
 * the closest-hit launch, the pixels whose hit points' point-light shadow
 * rays may cross one of its boxes the any-hit launch; the ranks agree
 * through the same collectives over U (the pixels any domain box may be
 * seen through, the same on every rank), with no host read.  Same results
 * per sample as spray_rt_insitu_trace_frame on those rays.  AO: U's eye rays
 * generated in one pass, then the replicated AO frame over them.  World 1:
 * the eye rays, then the all-local frame. */
int spray_rt_insitu_trace_camera(spray_rt_insitu_t ins, const spray_rt_shader* shader,
                                 const float cam[14], int image_w, int image_h, int spp,
                                 float* image_rgba, const spray_rt_insitu_rec* rec,
                                 unsigned long long totals[3]);
/* The image-parallel frame of a camera (the reference's ooc
 * mode shards as replicas -- any rank may hold any domain -- and only the
 * image is composited): EVERY domain resident on every rank (ERR_STATE
 * otherwise), the image_h rows cut into world * bands horizontal bands,
 * band b = rows [b image_h / (world bands), (b + 1) image_h / (world bands)),
 * rank r owns bands r, r + world, ... (bands = 1, world | image_h:
 * makeHorizontalStripe, tile.cc:187-209).  Band heights may differ by one row, except where
 * world > 1, bands > 1 and the bands are traced whole (spp does not divide
 * 64, or SPRAY_IMAGE_CULL=0): that gather copies equal bands, so image_h
 * must be divisible by world * bands -- ERR_ARG otherwise, decided from the
 * arguments before anything is launched, written or sent (the image and
 * the collective log stay as they were, on every rank alike).  Each rank generates its bands' eye rays
 * (insitu::genMultiSampleEyeRays seeds: (pixel, sample), so any split
 * gives every pixel the same bits), traces them with the all-local frame of
 * world 1 (any shading spray_rt_insitu_trace supports: the fused PT launch,
 * or bounces, area lights, AO, delta BSDFs through the frame passes), adds
 * its film to its own rows of image_rgba, and the rows go to rank 0 in one
 * gather (HdrImage::composite, image.h:167-181, an MPI_Reduce SUM of
 * disjoint pixels there; here each rank sends only its own rows, 1/world of
 * the image -- when only the eye rays of pixels some domain box's footprint
 * covers are traced, see SPRAY_IMAGE_CULL, only those pixels' RGB, 12 B
 * each): rank 0's image holds the whole frame, its other ranks' pixels
 * REPLACED by theirs (clear the images first, HdrImage::clear).  One
 * gather (the data all-to-all-v, every rank but 0 sending) and one totals
 * all-reduce per frame; totals = the group's. */
int spray_rt_insitu_trace_image(spray_rt_insitu_t ins, const spray_rt_shader* shader,
                                const float cam[14], int image_w, int image_h, int spp, int bands,
                                float* image_rgba, const spray_rt_insitu_rec* rec,
                                unsigned long long totals[3]);
/* A view-aligned partition of n domain boxes (float[n][6]) over nranks for
 * camera cam: the box centres projected to the image and dealt by recursive
 * median splits (image x, then y, alternating; ties by domain id) into
 * groups of n / nranks (+1) -- each rank the domains along neighbouring
 * lines of sight, so that a ray's domain list mostly stays on one rank.  An
 * addition to InsituPartition's modes (data_partition.h:59-155) for a fixed
 * camera; results do not depend on the partition. */
int spray_rt_insitu_partition_view(const float* boxes, int n, const float cam[14], int nranks,
                                   int* owner);
/* Footprint primitives of the camera frames (tests): per image row y the
 * inclusive pixel range [x0[y], x1[y]] holding every eye ray of cam that
 * may enter box (x0 > x1: none; returns 0 = no pixel, 1 = rows, 2 = the
 * whole image; -1 bad arguments); the k slice boxes (out float[k][6])
 * whose union holds every hit point inside scene whose shadow ray toward
 * the point light may cross box (returns their count, -1 = everywhere). */
int spray_rt_camera_box_rows(const float cam[14], int image_w, int image_h, const float box[6],
                             int* x0, int* x1);
int spray_rt_camera_shadow_boxes(const float box[6], const float scene[6], const float light[3],
                                 int k, float* out);
/* Measurement: one rank of an N-rank group rehearsed alone on one GPU.  A
 * replay context's collectives do not communicate: the camera frame's
 * t-bits and list-position MINs copy the group results given by
 * spray_rt_insitu_replay_set (device arrays over U, as
 * spray_rt_insitu_replay_capture reads them after a one-rank replicated
 * camera frame with every domain resident, SPRAY_INSITU_REPLICATED=1), the
 * SUMs and the reduce keep the rank's own values.  Its device work is the
 * rank's exact share of the N-rank frame (its launches, their sizes and the
 * rays they walk), back to back on its stream; the film and totals it
 * produces are not the frame's.  PT camera frames with split keys, and AO
 * camera frames (spray_rt_insitu_replay_set_ao). */
int spray_rt_insitu_create_replay(spray_rt_ctx_t ctx, int world, int rank,
                                  spray_rt_insitu_t* out);
int spray_rt_insitu_replay_set(spray_rt_insitu_t ins, const uint32_t* d_tmin,
                               const uint8_t* d_lpmin, size_t n);
/* *n = U slots of the last camera PT frame; with d_tmin / d_lpmin (device,
 * cap entries) copies its group t-bits minima and list-position minima. */
int spray_rt_insitu_replay_capture(spray_rt_insitu_t ins, uint32_t* d_tmin, uint8_t* d_lpmin,
                                   size_t cap, size_t* n);
/* The same for AO camera frames: the 64-bit key minima over U (d_kmin, n)
 * and the winners' published normals and colours (d_pub, 2 n uint64 --
 * the publish step's SUM); capture after a one-rank replicated AO camera
 * frame with every domain resident. */
int spray_rt_insitu_replay_set_ao(spray_rt_insitu_t ins, const uint64_t* d_kmin,
                                  const uint64_t* d_pub, size_t n);
int spray_rt_insitu_replay_capture_ao(spray_rt_insitu_t ins, uint64_t* d_kmin, uint64_t* d_pub,
                                      size_t cap, size_t* n);
/* The AO frame's first-round occlusion bits (a pair occluded by its home
 * rank, which depend on the partition): with d_out, copies the last frame's
 * own bits (*n bytes; rehearse every rank once, OR them); else sets d_bits
 * (nbytes, the group's OR) as the result of that SUM; *n = the byte count. */
int spray_rt_insitu_replay_bits_ao(spray_rt_insitu_t ins, const uint8_t* d_bits, uint8_t* d_out,
                                   size_t nbytes, size_t* n);
/* Per-phase device time of the traces since the last call (then reset),
 * HIP events on the context's stream, when phase timing is on
 * (spray_rt_insitu_set_timing).  out_ms[9]; *nphases = phases of the last
 * trace's form: replicated frame {lists, keyed closest hit, shadows, film,
 * totals}; protocol {route + plan, ray exchange, keyed closest hit, key
 * composite, shading, shadow route + exchange, shadow any hit + return,
 * film + totals}; all-local {frame}.  out_ms[8]: the time inside the
 * collectives (and the host reads of their counts), whatever the form. */
int spray_rt_insitu_set_timing(spray_rt_insitu_t ins, int on);
int spray_rt_insitu_phase_times(spray_rt_insitu_t ins, double out_ms[9], int* nphases);
/* HdrImage::composite (src/display/image.h:167-181): SUM of the ranks'
 * images at rank 0 (device float[nfloats], in place). */
int spray_rt_insitu_composite(spray_rt_insitu_t ins, float* image_rgba, size_t nfloats);
/* out[6] = bytes sent to other ranks, bytes received, exchanges, host
 * count reads, collectives issued, traces -- since creation. */
int spray_rt_insitu_stats(spray_rt_insitu_t ins, unsigned long long out[6]);
/* The issue log of the group's collectives since creation or the last
 * clear, in host call order -- what every rank must enqueue identically for
 * RCCL (per communicator, across its streams).  Entry = op << 56 | side << 51
 * | element count (48 bits); op: 1 count all-to-all (int64[world]), 2 data
 * all-to-all-v (bytes; count 0: per-peer counts differ by rank and match
 * pairwise), 3 all-reduce SUM u64, 4 reduce SUM f32 to rank 0, 5 all-reduce
 * MIN u64, 6 all-reduce SUM u8, 7 all-reduce MIN u32, 8 all-reduce MIN u8;
 * side = enqueued on the engine's second stream.  *n = entries logged (the
 * first min(cap, 65536) are copied to out); clear != 0 empties the log. */
int spray_rt_insitu_collective_log(spray_rt_insitu_t ins, uint64_t* out, size_t cap, size_t* n,
                                   int clear);

#ifdef __cplusplus
}
#endif
#endif
