// build_kernels.h -- host-side launchers of the device BVH build
// (build_kernels.hip): a new triangle list into a slot, built on the GPU.
//
// The topology and the collapse run one workgroup per slot (levels looped
// under __syncthreads(), nothing handed between workgroups inside a launch):
// the shape of the project's scenes, many small domains.  A large domain is
// built correctly, only more slowly -- its levels are walked by one
// workgroup in strides.
#pragma once

#include <hip/hip_runtime.h>

#include "refit_kernels.h"
#include "rt_common.h"

namespace spray_rt {

// What the host reads back per slot of a build call.
struct alignas(16) BuildRec {
  uint32_t nnodes, nq;
  int32_t depth;        // deepest leaf range (the root range is depth 0)
  int32_t height;       // BFS levels of inner nodes == groups of the bottom-up fit
  int32_t stack_bound;  // pending entries of the 4-wide walk
  uint32_t pad[3];
  uint32_t level[kRefitLevels];  // the refit level table
};

// One slot of a build call (device table).  Everything but verts / faces is
// scratch of the call; `cap` = max(ntris - 1, 1) bounds nnodes and nq.
struct alignas(16) BuildJob {
  const float* verts;
  const uint32_t* faces;
  uint64_t* keys;    // [ntris] (code << 32) | face, face order
  uint64_t* sorted;  // [ntris] the same, ascending
  float* part;       // [kBuildParts][6] per-block centroid bounds
  uint32_t* prims;   // [ntris] sorted order -> face
  BvhNode* nodes;    // [cap] refs, then the exact boxes fitted in place; QNode4 i's
                     // child refs at nodes - 64 - 64 (i + 1) as in a slot
  uint2* range;      // [cap] sorted-triangle range of each node
  uint8_t* hgt;      // [cap] BVH2 height of each node
  uint2* qlist;      // [cap] (BVH2 node, pending entries) of each QNode4
  uint32_t* order;   // [cap] refit metadata
  uint32_t* level;   // [kRefitLevels]
  int32_t* qsrc;     // [4 cap]
  BuildRec* rec;
  uint32_t ntris, nverts, cap, pad;
};
static_assert(sizeof(BuildJob) % 16 == 0, "job table entries stay 16-B aligned");

constexpr int kBuildParts = 64;  // blocks per slot of the code pass

// One array copy of the commit: nwords 32-bit words.
struct CopyJob {
  uint32_t* dst;
  const uint32_t* src;
  size_t nwords;
};

// Code pass 1: face indices and finiteness into status[j] (refit::kBad*,
// build::kBadFace), per-block centroid bounds into part.
hipError_t launch_build_check(hipStream_t s, const BuildJob* jobs, int njobs, uint32_t max_tris,
                              uint32_t* status);
// Code pass 2: the sort keys (slots with a status bit get keys they never read).
hipError_t launch_build_keys(hipStream_t s, const BuildJob* jobs, int njobs, uint32_t max_tris,
                             const uint32_t* status);
// All slots' keys in one segmented sort: keys / sorted are the concatenated
// arrays, offsets[njobs + 1] the slots' first triangles (device).  tmp == nullptr:
// only *tmp_bytes is set.  May read the segment-size partition back (rocPRIM).
hipError_t build_sort(hipStream_t s, void* tmp, size_t* tmp_bytes, const uint64_t* keys,
                      uint64_t* sorted, uint32_t total, int njobs, const uint32_t* offsets);
// Ranges, node numbering, heights and the refit metadata; writes rec and the
// counts of rjobs[j] (nnodes, height; a slot with a status bit becomes empty).
hipError_t launch_build_topology(hipStream_t s, const BuildJob* jobs, RefitJob* rjobs, int njobs,
                                 const uint32_t* status);
// The 4-wide collapse over the fitted boxes: QNode4 child refs, qsrc, nq.
hipError_t launch_build_collapse(hipStream_t s, const BuildJob* jobs, RefitJob* rjobs, int njobs);
hipError_t launch_build_copy(hipStream_t s, const CopyJob* copies, int ncopies, size_t max_words);

}  // namespace spray_rt
