// clip_kernels.h -- host-side launchers of the clip of cell meshes by a level
// of their scalar field (clip_kernels.hip), batched over all meshes of a call.
//
// The cap is the tet extraction's (tet_kernels.h) and the skin's source the
// surface extraction's (surf_kernels.h): the kernels here read a mesh through
// its SurfJob, find cap vertices through its TetInst and add what the clip
// needs on top.  One thread per cell or per point in blocks of
// surf::kSurfBlock, one per sorted crossing-edge instance in blocks of
// tet::kTetBlock.  Nothing is handed between workgroups inside a launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "surf_kernels.h"
#include "tet_kernels.h"

namespace spray_rt {

// What the clip knows of a mesh beside its SurfJob (device table).
struct alignas(16) ClipJob {
  float isovalue;
  uint32_t invert;
  uint32_t pad[2];
};
static_assert(sizeof(ClipJob) % 16 == 0, "job table entries stay 16-B aligned");

// Where the last passes write one mesh (device table): the cap's ncap_verts
// vertices and ncap_faces faces lie in front; the capacities, cap and skin
// together, bound every store.
struct alignas(16) ClipOut {
  float* verts;      // [nverts][3] or nullptr
  float* normals;    // [nverts][3] or nullptr
  uint32_t* colors;  // [nverts] or nullptr
  uint32_t* pairs;   // [nverts][2] or nullptr
  float* vt;         // [nverts] or nullptr
  uint32_t* faces;   // [nfaces][3] or nullptr
  uint64_t cap_verts, cap_faces;
  uint64_t ncap_verts, ncap_faces;
};
static_assert(sizeof(ClipOut) % 16 == 0, "job table entries stay 16-B aligned");

// Count pass: surf_count's checks with the values among them, the cells with a
// kept point as the select; the points' use flags cleared.
hipError_t launch_clip_count(hipStream_t s, const SurfJob* jobs, const ClipJob* cjobs, int njobs,
                             uint32_t max_blocks, uint32_t max_pblocks, uint32_t* status);
// After surf_unique: the pieces of every cell's surviving faces and the kept
// points among the flagged ones, both block-scanned.  A cut edge without a cap
// vertex sets clip::kMiss in status[mesh].
hipError_t launch_clip_skin_count(hipStream_t s, const SurfJob* jobs, const ClipJob* cjobs,
                                  const TetInst* insts, int njobs, uint32_t max_blocks,
                                  uint32_t max_pblocks, uint32_t* status);
// After the cap's vertex and face passes: pair and t of every cap vertex, the
// corner swap of an inverted mesh's cap faces, the kept points behind the cap's
// vertices and the skin pieces behind its faces.
hipError_t launch_clip_emit(hipStream_t s, const SurfJob* jobs, const ClipJob* cjobs,
                            const TetInst* insts, const ClipOut* outs, int njobs,
                            uint32_t max_blocks, uint32_t max_pblocks, uint32_t max_iblocks,
                            uint32_t max_fblocks, uint32_t* status);
// values[p] = clip::plane_value of every point.
struct Plane {
  float origin[3], normal[3];
};
hipError_t launch_plane_values(hipStream_t s, const float* points, uint64_t npoints, Plane plane,
                               float* values);

}  // namespace spray_rt
