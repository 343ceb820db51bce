// surf_kernels.h -- host-side launchers of the boundary-surface and threshold
// extraction from meshes of hexahedra, wedges, pyramids and tets
// (surf_kernels.hip), batched over all meshes of a call.
//
// One thread per cell in blocks of surf::kSurfBlock consecutive cells, one
// thread per point in blocks of as many points, one thread per sorted face
// instance.  Nothing is handed between workgroups inside a launch: the count
// passes leave per-block sums, tet_scan (tet_kernels.h) turns them into block
// bases through TetJob views of the mesh, the next launch reads them; the sort
// is tet_sort.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spray_rt {

// One mesh of a call (device table).
struct alignas(16) SurfJob {
  const float* points;       // [npoints][3]
  const uint8_t* types;      // [ncells]
  const uint32_t* offsets;   // [ncells + 1]
  const uint32_t* conn;      // [nconn]
  const float* values;       // [npoints]; mode kPoints only
  const float* cell_values;  // [ncells]; mode kCells only
  const float* normals;      // [npoints][3]; nullptr: none, or not wanted
  const float* cfield;       // [npoints] colour field; nullptr: color
  const uint32_t* ctable;    // [ntable] device copy of the table
  uint32_t* word;            // [ncells] surf::cell_word per cell
  uint32_t* iblock;          // [nblocks] face instances of each block, then its first
  uint32_t* tblock;          // [nblocks] the same for triangles
  uint32_t* pword;           // [npoints] use flag, then surf::point_word
  uint32_t* pblock;          // [npblocks] vertices of each block of points, then its first
  // the instance scratch, set after the first host read
  uint64_t* keys;   // [ninst] face keys in (cell, face) order
  uint64_t* skeys;  // [ninst] sorted
  uint32_t* vals;   // [ninst] cell << 3 | face beside keys
  uint32_t* svals;  // [ninst] ... beside skeys
  uint8_t* alive;   // [ninst] in (cell, face) order: the face is on the surface
  uint64_t npoints, nconn;
  uint32_t ncells, nblocks, npblocks;
  uint32_t ninst;  // bounds the stores of keys, unique
  int32_t mode;
  float lo, hi;
  uint32_t color;
  int32_t ntable;
  float clo, cscale;
  int32_t shift;  // surf::face_key's w
};
static_assert(sizeof(SurfJob) % 16 == 0, "job table entries stay 16-B aligned");

// Where the last passes write one mesh (device table); the capacities bound
// every store.
struct alignas(16) SurfOut {
  float* verts;      // [nverts][3] or nullptr
  float* normals;    // [nverts][3] or nullptr
  uint32_t* colors;  // [nverts] or nullptr
  uint32_t* ids;     // [nverts] point index of each vertex, or nullptr
  uint32_t* faces;   // [nfaces][3] or nullptr
  uint64_t cap_verts, cap_faces;
  uint64_t pad;
};
static_assert(sizeof(SurfOut) % 16 == 0, "job table entries stay 16-B aligned");

// Count pass: every check, the kept cells' face counts block-scanned into a
// word per cell and per-block sums; the points' use flags cleared.  What is
// wrong with a cell sets status bits in status[mesh].
hipError_t launch_surf_count(hipStream_t s, const SurfJob* jobs, int njobs, uint32_t max_blocks,
                             uint32_t max_pblocks, uint32_t* status);
// (key, cell << 3 | face) of every face of a kept cell at its scanned offset.
hipError_t launch_surf_keys(hipStream_t s, const SurfJob* jobs, int njobs, uint32_t max_blocks);
// Sorted instances whose key occurs once: alive[] of every instance, the use
// flags of the surviving faces' points.
hipError_t launch_surf_unique(hipStream_t s, const SurfJob* jobs, int njobs, uint32_t max_iblocks);
// Triangles of the surviving faces per cell and vertices per point, both
// block-scanned.
hipError_t launch_surf_tri_count(hipStream_t s, const SurfJob* jobs, int njobs,
                                 uint32_t max_blocks, uint32_t max_pblocks);
// Position, normal, colour and point index of every used point; the triangles
// of every surviving face.
hipError_t launch_surf_emit(hipStream_t s, const SurfJob* jobs, const SurfOut* outs, int njobs,
                            uint32_t max_blocks, uint32_t max_pblocks);

}  // namespace spray_rt
