// The workgroup prefix scans of the ordered compactions (map.hip, search.hip, pnp.hip), for kThreads lanes in waves of 64.  Integers
// only, so the prefix is the same in any order of evaluation.  Every lane of the workgroup calls a scan; `lds` is kThreads / 64
// words of the caller's; both return the lane's exclusive prefix and leave the workgroup's sum in `total`.  Device only.
#pragma once

#include <hip/hip_runtime.h>

// exclusive prefix of `v` over the workgroup
template <int kThreads>
__device__ __forceinline__ int vs_block_excl_scan(int v, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        const int s = lds[w];
        if (w < wv) base += s;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

// exclusive prefix of a flag over the workgroup by ballots: how many lanes below this one hold it
template <int kThreads>
__device__ __forceinline__ int vs_block_flag_scan(bool f, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) lds[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        const int c = lds[w];
        before += w < wave ? c : 0;
        total += c;
    }
    __syncthreads();
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}
