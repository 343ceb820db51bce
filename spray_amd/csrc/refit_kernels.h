// refit_kernels.h -- host-side launchers of the refit kernels
// (refit_kernels.hip): new vertex positions into resident slots, the tree
// topology kept.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_common.h"

namespace spray_rt {

// One slot of a refit call (device table, one entry per slot).  The slot's
// arrays are read for the topology during the fit and written by the commit
// only; the scratch arrays hold the fitted image in between.
struct alignas(16) RefitJob {
  BvhNode* nodes;         // slot: BVH2 nodes; QGrid at nodes - 32, QNode4 i at
                          // nodes - 64 - 64 (i + 1) (rt_common.h)
  float* tris;            // slot: 12 floats per leaf-order triangle
  const uint32_t* prims;  // slot: leaf order -> face
  const uint32_t* faces;  // slot
  float* normals;         // slot (nullptr: none)
  const uint32_t* order;  // refit metadata: nodes by height
  const uint32_t* level;  // refit metadata: kRefitLevels entries
  const int32_t* qsrc;    // refit metadata: 4 per QNode4
  const float* verts;     // new vertices (device)
  const float* vnormals;  // new normals (device; nullptr with normals == nullptr)
  BvhNode* s_nodes;       // scratch: the fitted nodes, boxes exact (unpadded)
  QNode4* s_q;            // scratch: the requantized QNode4s, index order
  QGrid* s_grid;          // scratch: the new grid
  uint32_t nnodes, ntris, nverts, nq;
  int32_t height;
  uint32_t pad[3];
};
static_assert(sizeof(RefitJob) % 16 == 0, "job table entries stay 16-B aligned");

// Phase 1 (writes scratch and status only).  status[j] |= refit::kBad* bits.
// max_* = the largest count over the call's jobs (they size the grids).
hipError_t launch_refit_check_tris(hipStream_t s, const RefitJob* jobs, int njobs,
                                   uint32_t max_tris, uint32_t* status);
// nodes of height h of every job (children come from earlier launches)
hipError_t launch_refit_fit_level(hipStream_t s, const RefitJob* jobs, int njobs, int h,
                                  uint32_t max_level_nodes);
hipError_t launch_refit_grid(hipStream_t s, const RefitJob* jobs, int njobs, uint32_t* status);
hipError_t launch_refit_quant(hipStream_t s, const RefitJob* jobs, int njobs, uint32_t max_nq,
                              uint32_t* status);
// Phase 2: scratch -> slots, triangle records, normals, bounds (optional,
// float[njobs][6] exact lo.xyz hi.xyz).
hipError_t launch_refit_commit(hipStream_t s, const RefitJob* jobs, int njobs,
                               uint32_t max_nodes, uint32_t max_tris, uint32_t max_verts,
                               float* bounds);
// SAH cost of a slot's BVH2 (spray_rt.h, spray_rt_slot_sah) into *out
hipError_t launch_slot_sah(hipStream_t s, const BvhNode* nodes, uint32_t nnodes, double* out);

}  // namespace spray_rt
