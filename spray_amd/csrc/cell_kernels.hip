// cell_kernels.hip -- gfx950 kernels in front of the tet extraction for meshes
// of hexahedra, wedges, pyramids and tets: only the cells the isosurface
// crosses become tets.
//
//   count   one thread per cell: type and offsets against each other and
//           nconn, the indices (each < npoints), finiteness of what the call
//           reads of the cell's points, the inside bits; a cell whose points
//           are not all on one side counts its 1, 2, 3 or 6 tets; a block scan
//           leaves the cell's word and the block's sum
//   scan    tet_scan over a TetJob view: block sums to block bases, the total
//   split   one thread per crossing cell: cell::split at the cell's scanned
//           offset
//
// Data moves between workgroups only across launch boundaries on one stream.
// Every store is an ordinary vector store; the only atomic is the atomicOr of
// a status word.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "cell_common.h"
#include "cell_kernels.h"

namespace spray_rt {
namespace {

using namespace cell;

__global__ __launch_bounds__(kCellBlock) void cell_count_kernel(const CellJob* __restrict__ jobs,
                                                               uint32_t* __restrict__ status) {
  const CellJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  __shared__ uint32_t s_scan[kCellBlock];
  const uint32_t i = blockIdx.x * kCellBlock + threadIdx.x;
  uint32_t nt = 0;
  if (i < J.ncells) {
    const Cell C = classify(J.points, J.types, J.offsets, J.conn, J.values, J.cfield, J.normals,
                            J.npoints, J.nconn, i, J.isovalue);
    if (C.status) atomicOr(&status[blockIdx.y], C.status);
    nt = C.ntets;
  }
  uint32_t total;
  const uint32_t excl = block_excl_scan<kCellBlock>(nt, s_scan, &total);
  if (i < J.ncells) J.word[i] = cell_word(excl, nt);
  if (threadIdx.x == 0) J.tblock[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCellBlock) void cell_split_kernel(const CellJob* __restrict__ jobs) {
  const CellJob J = jobs[blockIdx.y];
  if (blockIdx.x >= J.nblocks) return;
  const uint32_t i = blockIdx.x * kCellBlock + threadIdx.x;
  if (i >= J.ncells) return;
  const uint32_t word = J.word[i];
  const uint32_t nt = word_ntets(word);
  if (!nt) return;
  // a counted cell passed check_cell in this call: its type is known and its
  // indices lie inside conn
  const uint32_t type = J.types[i];
  if (uint32_t(cell_tets(type)) != nt) return;
  const uint64_t first = uint64_t(J.tblock[blockIdx.x]) + word_loc(word);
  if (first + nt > J.ntets) return;
  const uint32_t o0 = J.offsets[i];
  if (uint64_t(o0) + uint64_t(cell_points(type)) > J.nconn) return;
  split(type, J.conn + o0, J.tets + 4 * first);
}

}  // namespace

hipError_t launch_cell_count(hipStream_t s, const CellJob* jobs, int njobs, uint32_t max_blocks,
                             uint32_t* status) {
  if (!max_blocks) return hipSuccess;
  hipLaunchKernelGGL(cell_count_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kCellBlock), 0, s,
                     jobs, status);
  return hipGetLastError();
}

hipError_t launch_cell_split(hipStream_t s, const CellJob* jobs, int njobs, uint32_t max_blocks) {
  if (!max_blocks) return hipSuccess;
  hipLaunchKernelGGL(cell_split_kernel, dim3(max_blocks, unsigned(njobs)), dim3(kCellBlock), 0, s,
                     jobs);
  return hipGetLastError();
}

}  // namespace spray_rt
