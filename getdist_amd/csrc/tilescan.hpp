// Exclusive scan of per-tile counts by one block: the ordered compactions of draw.hip and export.hip count per tile in a
// first pass, scan here, and place in a second pass.
#pragma once
#include <hip/hip_runtime.h>

// exclusive scan of the nb tile counts in place, 1024 per pass of one block; cnt[nb] receives the total
static __global__ void __launch_bounds__(1024) k_tile_scan(long long* __restrict__ cnt, int nb) {
    __shared__ long long sh[1024];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const long long v = (i < nb) ? cnt[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long long a = (threadIdx.x >= (unsigned)o) ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nb) cnt[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[nb] = carry;
}
