// gs_blocksum_dev.hpp — the fixed-order reductions of the vertex-parallel kernels (gs_lm.hip, gs_dogleg.hip): 256 threads per workgroup,
// lanes by shuffle, waves in wave order.  Device code only; the functions are what gs_lm.hip defined for itself, moved here unchanged.
#pragma once
#include <hip/hip_runtime.h>

namespace gs {

__device__ __forceinline__ double lm_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double lm_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}
// fixed-order sum / max over the 256 threads, the result in EVERY thread (red: 5 doubles of LDS)
__device__ __forceinline__ double lm_block_sum(double v, double *red) {
    v = lm_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) red[4] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    const double r = red[4];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double lm_block_max(double v, double *red) {
    v = lm_wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) red[4] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    const double r = red[4];
    __syncthreads();
    return r;
}

}  // namespace gs
