// block_stream_kernels.h -- host-side launchers of the multi-block streamline
// filter (block_stream_kernels.hip): sets of vector blocks and seeds in HBM to
// polylines that run from block to block, batched over all sets of a call.
//
// The launch shape is stream_kernels.h's: one lane per half-line, blocks of
// strm::kBlock lanes, per-workgroup sums, one workgroup per set for the bases.
// A set has a StreamJob as a field has (its grid members unused), so the scan
// and the tube expansion are stream_kernels.hip's own launches; the check, the
// count and the integrate pass are new and take the set's blocks from a second
// table.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_stream_common.h"
#include "stream_kernels.h"

namespace spray_rt {

// The blocks of one set of a call (device table, beside its StreamJob).
struct alignas(16) BlockJob {
  const bstrm::BlockRec* blocks;  // [nvb]
  const bstrm::BlockBox* boxes;   // [nvb] the inside tests of the miss path
  uint32_t nvb;                   // 1 .. 65535
  uint32_t has_color;             // every block has a colour field and the set a table
};
static_assert(sizeof(BlockJob) == 32, "job table entries stay 16-B aligned");

// What the integrate pass writes beside a set's StreamOut (device table).
struct alignas(16) BlockOut {
  uint32_t* point_blocks;  // [cap_points] the block each point was sampled in, or null
  uint64_t pad;
};

// Check pass over every block's samples and the seeds: strm::kBad* into
// status[2 * set], the lowest block with a bad sample into status[2 * set + 1]
// (the host sets it to bstrm::kNoBlock).
hipError_t launch_block_stream_check(hipStream_t s, const StreamJob* jobs, const BlockJob* bjobs,
                                     int njobs, uint32_t* status);
// Count pass: as launch_stream_count, the block rule deciding each sample's grid.
hipError_t launch_block_stream_count(hipStream_t s, const StreamJob* jobs, const BlockJob* bjobs,
                                     int njobs, uint32_t max_blocks);
// Integrate pass: as launch_stream_integrate, point_blocks as well.
hipError_t launch_block_stream_integrate(hipStream_t s, const StreamJob* jobs,
                                         const BlockJob* bjobs, const StreamOut* outs,
                                         const BlockOut* bouts, int njobs, uint32_t max_blocks,
                                         bool tubes);

}  // namespace spray_rt
