// The one workgroup reduction of the f64 optimizers (refit.hip, refine.hip, resect.hip, adjust.hip), for 256 lanes = 4 waves.
// No floating-point atomics: a caller adds its items into per-lane strided partial sums and closes them here, so an item's bits
// depend on the item alone -- not on the batch, the slot or the run.  Device only.
#pragma once

#include <hip/hip_runtime.h>

struct VsBlockReduce {
    double *lds;   // [4][Nmax], Nmax the widest sum of the kernel

    // Sum of v[i] over the workgroup, in every lane.  The butterfly adds the same two partial sums in both partners (a + b and
    // b + a: the same bits), so all lanes of a wave end with one value; the wave sums are added in wave order.
    template <int N>
    __device__ __forceinline__ void sum(double (&v)[N]) const {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int i = 0; i < N; i++) v[i] += __shfl_xor(v[i], off);
        }
        __syncthreads();   // the previous sum has been read by everyone
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < N; i++) lds[(threadIdx.x >> 6) * N + i] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = ((lds[i] + lds[N + i]) + lds[2 * N + i]) + lds[3 * N + i];
    }

    // whether f holds in some lane, in every lane
    __device__ __forceinline__ bool any(bool f) const { return __syncthreads_or(f ? 1 : 0) != 0; }
};
