// cell_kernels.h -- host-side launchers of the split of hexahedral, wedge,
// pyramid and tet cells into the tets the isosurface crosses
// (cell_kernels.hip), batched over all meshes of a call.
//
// One thread per cell in blocks of cell::kCellBlock consecutive cells.  Nothing
// is handed between workgroups inside a launch: the count pass leaves per-block
// sums, tet_scan (tet_kernels.h) turns them into block bases through a TetJob
// view of the mesh, the split reads them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spray_rt {

// One mesh of a call (device table).
struct alignas(16) CellJob {
  const float* points;      // [npoints][3]
  const uint8_t* types;     // [ncells]
  const uint32_t* offsets;  // [ncells + 1]
  const uint32_t* conn;     // [nconn]
  const float* values;      // [npoints]
  const float* normals;     // [npoints][3]; nullptr: none, or not wanted
  const float* cfield;      // [npoints] colour field; nullptr: none
  uint32_t* word;           // [ncells] cell::cell_word per cell
  uint32_t* tblock;         // [nblocks] tets of each block, then its first tet
  uint32_t* tets;           // [ntets][4] of the crossing cells (set after the first host read)
  uint64_t npoints, nconn;
  uint32_t ncells, nblocks;
  float isovalue;
  uint32_t ntets;  // of the crossing cells: bounds the split's stores
};
static_assert(sizeof(CellJob) % 16 == 0, "job table entries stay 16-B aligned");

// Count pass: a word per cell and per-block tet sums; what is wrong with a
// cell sets cell::kBad* / tet::kBad* bits in status[mesh].
hipError_t launch_cell_count(hipStream_t s, const CellJob* jobs, int njobs, uint32_t max_blocks,
                             uint32_t* status);
// The tets of every crossing cell at its scanned offset.
hipError_t launch_cell_split(hipStream_t s, const CellJob* jobs, int njobs, uint32_t max_blocks);

}  // namespace spray_rt
