// ctgcn_reduce.h — the fp64 block sum of ctgcn_cent.hip and ctgcn_sim.hip: a fixed-order LDS tree, so a sum does not depend on timing.
#pragma once
#include <hip/hip_runtime.h>

// Sum of v over the THREADS threads of the block (a power of two), returned to every thread; sh: THREADS doubles of LDS, free again
// on return.
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int m = THREADS / 2; m > 0; m >>= 1) {
        if (t < m) sh[t] += sh[t + m];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
