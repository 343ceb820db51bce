// iso_kernels.h -- host-side launchers of the isosurface extraction
// (iso_kernels.hip): structured grids of scalars in HBM to welded, indexed
// triangle meshes, batched over all grids of a call.
//
// One thread per lattice point, blocks of iso::kIsoBlock consecutive points.
// Nothing is handed between workgroups inside a launch: the count pass leaves
// per-block sums, one workgroup per grid turns them into block bases, the emit
// pass reads them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spray_rt {

// What the host reads back per grid: the mesh's sizes.
struct IsoRec {
  uint64_t nverts, nfaces;
};

// One grid of a call (device table).
struct alignas(16) IsoJob {
  const float* values;  // [nz][ny][nx]
  uint32_t* code;       // [npoints] iso::code_word per point
  uint32_t* vblock;     // [nblocks] vertices of each block, then its first vertex
  uint32_t* fblock;     // [nblocks] the same for faces
  IsoRec* rec;
  int32_t nx, ny, nz;
  uint32_t npoints, nblocks;
  float origin[3], spacing[3], isovalue;
  uint32_t color;
  // the colour map of a mapped grid (color_common.h); cfield == nullptr: color
  const float* cfield;     // [nz][ny][nx] colour field
  const uint32_t* ctable;  // [ntable] device copy of the table
  int32_t ntable;
  float clo, cscale;
  uint32_t pad[3];
};
static_assert(sizeof(IsoJob) % 16 == 0, "job table entries stay 16-B aligned");

// Where the emit pass writes one grid's mesh (device table); the capacities
// bound every store.
struct alignas(16) IsoOut {
  float* verts;      // [nverts][3]
  float* normals;    // [nverts][3] or nullptr
  uint32_t* colors;  // [nverts] or nullptr
  uint32_t* faces;   // [nfaces][3]
  uint64_t cap_verts, cap_faces;
};
static_assert(sizeof(IsoOut) % 16 == 0, "job table entries stay 16-B aligned");

// Count pass: code words and per-block sums; a non-finite sample sets
// iso::kBadSample in status[grid], a non-finite colour sample iso::kBadColor.
hipError_t launch_iso_count(hipStream_t s, const IsoJob* jobs, int njobs, uint32_t max_blocks,
                            uint32_t* status);
// Block sums to exclusive block bases, totals into rec (one workgroup per grid).
hipError_t launch_iso_scan(hipStream_t s, const IsoJob* jobs, int njobs);
// Emit pass: positions, normals and colors per (point, edge), faces per cell;
// a null array of an IsoOut is not written.  colors_only: no grid of the call
// has another array than colors, and the launch does the colour work alone.
hipError_t launch_iso_emit(hipStream_t s, const IsoJob* jobs, const IsoOut* outs, int njobs,
                           uint32_t max_blocks, bool colors_only = false);

// spray_rt_colormap_apply: colors[i] = table[bin(scalars[i])], one thread per
// four elements; a non-finite scalar sets cmap::kBadScalar in *status.
hipError_t launch_colormap_apply(hipStream_t s, const float* scalars, size_t n,
                                 const uint32_t* table, int ntable, float lo, float scale,
                                 uint32_t* colors, uint32_t* status);

// One slot of a spray_rt_domains_recolor call (device table).
struct alignas(16) RecolorJob {
  uint32_t* dst;        // the slot's colour array
  const uint32_t* src;  // [n] the new colours
  uint32_t n;
  uint32_t pad[3];
};
static_assert(sizeof(RecolorJob) % 16 == 0, "job table entries stay 16-B aligned");
// Copies every job's colours into its slot, one launch for all jobs.
hipError_t launch_recolor(hipStream_t s, const RecolorJob* jobs, int njobs, uint32_t max_n);

}  // namespace spray_rt
