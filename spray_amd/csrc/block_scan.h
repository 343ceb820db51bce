// block_scan.h -- the workgroup scan of the build and isosurface kernels.
#pragma once

#include <hip/hip_runtime.h>

namespace spray_rt {

// Exclusive sum over the block's threads in thread order; *total = the sum.
// Every thread of the block calls it.
template <int B, typename T>
__device__ inline T block_excl_scan(T v, T* s, T* total) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < B; off <<= 1) {
    const T x = t >= off ? s[t - off] : T(0);
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  *total = s[B - 1];
  const T excl = s[t] - v;
  __syncthreads();
  return excl;
}

}  // namespace spray_rt
