// glyph_kernels.h -- host-side launchers of the glyph filter
// (glyph_kernels.hip): point sets in HBM to spheres and arrows as indexed
// triangle meshes, batched over all sets of a call.
//
// One lane per point in the count and place passes, blocks of glyph::kBlock
// lanes; one thread per output vertex and per face in the expansion.  Nothing
// is handed between workgroups inside a launch: the count pass leaves per-block
// sums, one workgroup per set turns them into block bases, the place pass reads
// them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spray_rt {

// What the host reads back per set: the glyphs it keeps.
struct GlyphCount {
  uint64_t kept, pad;
};

// One kept point, as the expansion reads it (three 16-B loads).
struct alignas(16) GlyphRec {
  float p[3], s;   // the point, its factor
  float T[3];      // arrows: the tangent
  uint32_t id;     // the source point
  float N[3];      // arrows: the frame normal
  uint32_t color;  // already mapped
};
static_assert(sizeof(GlyphRec) == 48, "three 16-B loads");

// One set of a call (device table).
struct alignas(16) GlyphJob {
  const float* points;     // [npoints][3]
  const float* vectors;    // [npoints][3], arrows only
  const float* scales;     // [npoints] or nullptr
  const float* select;     // [npoints] or nullptr
  const float* cfield;     // [npoints] colour field, nullptr: color
  const uint32_t* ctable;  // [ntable] device copy of the table
  const float* tverts;     // spheres: the unit table [V][3]
  const uint32_t* tfaces;  // spheres: its faces [F][3]
  uint32_t* word;          // [npoints] glyph::kKept | the lane's exclusive rank in its block
  uint32_t* bbase;         // [nblocks] kept points of each block, then its base
  GlyphCount* count;
  uint32_t npoints, nblocks, stride;
  float select_lo, select_hi;
  float size, msq;
  int32_t shape, nsides, scale_by_vector;
  uint32_t V, F;  // vertices and faces per glyph
  int32_t ntable;
  float clo, cscale;
  uint32_t color;
  float cn, ct;       // arrows: the cone normal's constants
  float ring[16][2];  // arrows: cos, sin of 2 pi k / nsides
  uint32_t pad[2];
};
static_assert(sizeof(GlyphJob) % 16 == 0, "job table entries stay 16-B aligned");

// Where the place and the expansion pass write one set's arrays (device
// table); a null array is not written, the capacities bound every store.
struct alignas(16) GlyphOut {
  GlyphRec* recs;       // [nglyphs] scratch
  uint32_t* point_ids;  // [nglyphs]
  float* verts;         // [nverts][3]
  float* vnormals;      // [nverts][3]
  uint32_t* colors;     // [nverts]
  uint32_t* faces;      // [nfaces][3]
  uint64_t nglyphs;     // the host read's count: bounds recs and point_ids
  uint64_t cap_verts, cap_faces, pad;
};
static_assert(sizeof(GlyphOut) % 16 == 0, "job table entries stay 16-B aligned");

// Check pass: glyph::kBad* / kNegScale into status[set], over the arrays in use;
// max_blocks = the largest set's blocks of glyph::kBlock points.
hipError_t launch_glyph_check(hipStream_t s, const GlyphJob* jobs, int njobs, uint32_t max_blocks,
                              uint32_t* status);
// Count pass: the keep rule per point, lane words, block sums.
hipError_t launch_glyph_count(hipStream_t s, const GlyphJob* jobs, int njobs, uint32_t max_blocks);
// Block sums to exclusive block bases, the total into count (one workgroup per set).
hipError_t launch_glyph_scan(hipStream_t s, const GlyphJob* jobs, int njobs);
// Place pass: kept lanes write their record and point id at base + rank.
hipError_t launch_glyph_place(hipStream_t s, const GlyphJob* jobs, const GlyphOut* outs, int njobs,
                              uint32_t max_blocks);
// Expansion: one thread per output vertex and per face; max_items = the largest
// vertex or face count a set writes.
hipError_t launch_glyph_expand(hipStream_t s, const GlyphJob* jobs, const GlyphOut* outs,
                               int njobs, uint64_t max_items);

}  // namespace spray_rt
