// stream_kernels.h -- host-side launchers of the streamline filter
// (stream_kernels.hip): vector grids and seeds in HBM to polylines, and to
// tubes as indexed triangle meshes, batched over all fields of a call.
//
// One lane per half-line, blocks of strm::kBlock lanes; under
// SPRAY_RT_STREAM_BOTH lanes 2 s and 2 s + 1 are the backward and the forward
// half of seed s.  Nothing is handed between workgroups inside a launch: the
// count pass leaves per-block sums, one workgroup per field turns them into
// block bases, the integrate pass reads them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spray_rt {

// What the host reads back per field: the points of its lines, the points of
// its lines of two or more points, the number of those lines.
struct StreamRec {
  uint64_t npoints, tube_points, tube_lines, pad;
};

// One field of a call (device table).
struct alignas(16) StreamJob {
  const float* vectors;    // [nz][ny][nx][3]
  const float* seeds;      // [nseeds][3]
  const float* cfield;     // [nz][ny][nx] colour field, nullptr: color
  const uint32_t* ctable;  // [ntable] device copy of the table
  uint32_t* word;          // [nlanes] strm::lane_word per lane
  uint64_t* loc;           // [nlanes] the lane's exclusive strm::scan_word sum within its block
  uint4* bbase;            // [nblocks] sums of each block (points, tube points, tube lines), then its bases
  StreamRec* rec;
  int32_t dims[3];
  float origin[3], spacing[3];
  uint32_t nseeds, nlanes, nblocks;
  float step, msq;
  int32_t max_steps, direction;
  int32_t ntable;
  float clo, cscale;
  uint32_t color;
  float radius;
  int32_t nsides;
  float ring[16][2];  // cos, sin of 2 pi k / nsides
  uint32_t pad[2];
};
static_assert(sizeof(StreamJob) % 16 == 0, "job table entries stay 16-B aligned");

// Where the integrate and the expansion pass write one field's arrays (device
// table); a null array is not written, the capacities bound every store.
struct alignas(16) StreamOut {
  float* points;           // [npoints][3]
  uint32_t* line_offsets;  // [nseeds + 1]
  uint32_t* line_info;     // [nseeds][2]
  // the tube forms: per point, then per line (exclusive sums, [nseeds + 1])
  float* pnormals;    // [npoints][3] frame normal N
  float* ptangents;   // [npoints][3] tangent T
  uint32_t* pcolors;  // [npoints]
  uint32_t* tube_points;
  uint32_t* tube_lines;
  float* verts;      // [nverts][3]
  float* vnormals;   // [nverts][3]
  uint32_t* colors;  // [nverts]
  uint32_t* faces;   // [nfaces][3]
  uint64_t cap_points, cap_verts, cap_faces, pad;
};
static_assert(sizeof(StreamOut) % 16 == 0, "job table entries stay 16-B aligned");

// Check pass: a non-finite seed coordinate, vector sample or colour sample sets
// strm::kBadSeed / kBadVector / kBadColor in status[field].
hipError_t launch_stream_check(hipStream_t s, const StreamJob* jobs, int njobs, uint32_t* status);
// Count pass: every half-line integrated, lane words, in-block sums, block sums.
hipError_t launch_stream_count(hipStream_t s, const StreamJob* jobs, int njobs,
                               uint32_t max_blocks);
// Block sums to exclusive block bases, totals into rec (one workgroup per field).
hipError_t launch_stream_scan(hipStream_t s, const StreamJob* jobs, int njobs);
// Integrate pass: the same arithmetic again, points (the backward half at
// descending indices), line offsets and info; tubes: the per-point frames and
// colours and the per-line tube sums as well.
hipError_t launch_stream_integrate(hipStream_t s, const StreamJob* jobs, const StreamOut* outs,
                                   int njobs, uint32_t max_blocks, bool tubes);
// Expansion: one thread per output vertex and per face of the tubes;
// max_items = the largest vertex or face count of a field.
hipError_t launch_stream_expand(hipStream_t s, const StreamJob* jobs, const StreamOut* outs,
                                int njobs, uint64_t max_items);

}  // namespace spray_rt
