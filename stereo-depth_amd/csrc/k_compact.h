// k_compact.h -- the row count of the ordered stream compactions (k_points.h, k_reproject.h, k_tsdf.h).  Device only.  The
// scatters' ballot-ordered slot stays written out in them: no function form of it kept their device code.
#pragma once
#include "smx_common.h"

namespace smx {

// The sum of cnt over a workgroup of 256 threads through the kernel's wsum[4]: a shuffle-down within each wave, one
// store per wave, one barrier; thread 0 alone reads the four sums and gets the total, every other thread gets 0.
__device__ __forceinline__ int block_count(int cnt, int (&wsum)[4]) {
    int *const mine = &wsum[threadIdx.x >> 6];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((threadIdx.x & 63) == 0) *mine = cnt;
    __syncthreads();
    return threadIdx.x == 0 ? wsum[0] + wsum[1] + wsum[2] + wsum[3] : 0;
}

}  // namespace smx
