// The 32 x 32 tile of ransac_prune.hip's certificate on the f32 matrix cores -- n and a0 of 32 hypotheses x 32 matches -- and
// the walk over a pair's head with it.  Shared by ransac_prune_mfma_kernel (ransac_prune.hip: the matches behind the head)
// and ransac_screen_kernel (ransac_count.hip: the head itself, for the pairs vs_head_on_certificate sends that way).
// Device helpers only; no kernel lives here.  Operand layout, numerics and the certificate: ransac_prune.hip, ransac_prune_cert.h.
#pragma once

#include "ransac_prune_cert.h"
#include "ransac_residual.h"

namespace vs_prune {

typedef float v16f __attribute__((ext_vector_type(16)));
constexpr int kPruneWaves = 4;
constexpr int kPruneHyps = 32;    // per wave: the rows of a tile
constexpr int kPruneTile = 32;    // matches per tile: its columns
constexpr int kPruneOGT = 2;      // __builtin_amdgcn_fcmpf: llvm::FCmpInst::FCMP_OGT

// hypothesis row held by accumulator register r of a lane in half `half` (cdna4 ISA, 32x32 C/D layout)
__host__ __device__ constexpr int prune_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// A lane's A operands for its hypothesis: lower half even k, upper half odd k; k = 9 (n) and k = 3 (a0) are the zero padding.
struct PruneA {
    float n[5], d[2];
};
__device__ __forceinline__ PruneA prune_operands(const float *f, bool half) {
    PruneA A;
#pragma unroll
    for (int s = 0; s < 4; s++) A.n[s] = half ? f[2 * s + 1] : f[2 * s];
    A.n[4] = half ? 0.f : f[8];
    A.d[0] = half ? f[1] : f[0];
    A.d[1] = half ? 0.f : f[2];
    return A;
}

// One tile: n and a0 of 32 hypotheses x 32 matches.  The lane brings the coordinates of match (column) l & 31; phi_k for
// k = 2 s + (l >> 5) is its B operand of step s.  The last two steps of n (x1 | y1, 1 | 0) are the two steps of a0.
__device__ __forceinline__ void prune_tile(const PruneA &A, bool half, float x1, float y1, float x2, float y2, v16f &n, v16f &a0) {
    const float p = x2 * (half ? y1 : x1);   // phi_0 | phi_1
    const float q = y2 * (half ? x1 : y1);   // phi_4 | phi_3
    const float b1 = half ? q : x2, b2 = half ? y2 : q, b3 = half ? y1 : x1, b4 = half ? 0.f : 1.f;
    v16f z;
#pragma unroll
    for (int r = 0; r < 16; r++) z[r] = 0.f;
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(A.n[0], p, z, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(A.n[1], b1, n, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(A.n[2], b2, n, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(A.n[3], b3, n, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(A.n[4], b4, n, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A.d[0], b3, z, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A.d[1], b4, a0, 0, 0, 0);
}

// The head of a pair on the certificate, for the pairs vs_head_on_certificate (ransac_residual.h) sends this way -- their
// hypotheses have to miss more matches than the head holds, nearly all of them garbage the prune kernel then kills:
// pot0[h] = n0 - X[h], X the certified misses among the ranked matches [0, n0), instead of the cheap evaluation's count: an
// upper bound of the head's inliers all the same, which is all ransac_cand_kernel, the prune kernel and ransac_count_kernel
// rely on.  head[h] = (uncertified, 0): a survivor of the count kernel evaluates the head itself and takes no sum from here.
// A hypothesis outside the certificate's ranges or with a NaN in F certifies nothing: pot0 = n0.
// One wave: the 32 hypotheses from hbase on (the prune kernel's mapping), four tiles at most, no stop rule.  m >= 1.
constexpr int kHeadTiles = 4;   // the head holds at most kHeadTiles * kPruneTile matches
__device__ __forceinline__ void head_on_certificate(const float *__restrict__ rk, int kp_pad, int b, int m, int n0, int hbase, int hyp,
                                                    float threshold, float splus, const float *__restrict__ hypF,
                                                    const float *__restrict__ cmax, int32_t *__restrict__ pot0, int2 *__restrict__ head) {
    const int lane = threadIdx.x & 63, col = lane & 31;
    const bool half = lane >= 32;
    const int h = hbase + col;   // the lane's hypothesis (both halves hold the same 32)
    const size_t hi = (size_t)b * hyp + min(h, hyp - 1);
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = hypF[hi * 9 + k];
    const float c = pc_margin(f, cmax[2 * b], cmax[2 * b + 1], threshold, splus);   // +inf: no comparison of it is true
    const PruneA A = prune_operands(f, half);
    float cr[16];   // c of the hypothesis each accumulator register holds in this lane
#pragma unroll
    for (int r = 0; r < 16; r++) cr[r] = __shfl(c, half ? prune_row(r, 1) : prune_row(r, 0), 64);

    const float *r1 = rk + (size_t)b * 4 * kp_pad, *r2 = r1 + kp_pad, *r3 = r2 + kp_pad, *r4 = r3 + kp_pad;
    float x1[kHeadTiles], y1[kHeadTiles], x2[kHeadTiles], y2[kHeadTiles];
#pragma unroll
    for (int t = 0; t < kHeadTiles; t++) {
        const int j = min(t * kPruneTile + col, m - 1);   // lanes beyond n0 read a real match and are masked
        x1[t] = r1[j];
        y1[t] = r2[j];
        x2[t] = r3[j];
        y2[t] = r4[j];
    }
    int X[kPruneHyps];   // in scalar registers, as in the prune kernel
#pragma unroll
    for (int i = 0; i < kPruneHyps; i++) X[i] = 0;
#pragma unroll
    for (int t = 0; t < kHeadTiles; t++) {
        if (t * kPruneTile >= n0) break;   // wave-uniform
        v16f n, a0;
        prune_tile(A, half, x1[t], y1[t], x2[t], y2[t], n, a0);
        const unsigned long long valid = __ballot(t * kPruneTile + col < n0);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            // pc_miss (ransac_prune_cert.h) as a lane mask: |n| > fma(s+, |a0|, c), ordered
            const unsigned long long miss =
                __builtin_amdgcn_fcmpf(fabsf(n[r]), fmaf(splus, fabsf(a0[r]), cr[r]), kPruneOGT) & valid;
            X[prune_row(r, 0)] += __popc((uint32_t)miss);
            X[prune_row(r, 1)] += __popc((uint32_t)(miss >> 32));
        }
    }
    int xv = 0;   // lane l: X of hypothesis l & 31
#pragma unroll
    for (int i = 0; i < kPruneHyps; i++) xv = col == i ? X[i] : xv;
    if (!half && h < hyp) {
        pot0[hi] = n0 - xv;
        head[hi] = make_int2(kVsHeadUncertified, 0);
    }
}

}  // namespace vs_prune
