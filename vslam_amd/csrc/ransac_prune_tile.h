// The 32 x 32 tile of ransac_prune.hip's certificate on the f32 matrix cores -- n and a0 of 32 matches x 32 hypotheses -- and
// the walk over a pair's head with it.  Shared by ransac_prune_mfma_kernel (ransac_prune.hip: the matches behind the head)
// and ransac_screen_kernel (ransac_count.hip: the head itself, for the pairs vs_head_on_certificate sends that way).
// Device helpers only; no kernel lives here.  Operand layout, numerics and the certificate: ransac_prune.hip, ransac_prune_cert.h.
#pragma once

#include "ransac_prune_cert.h"
#include "ransac_residual.h"

namespace vs_prune {

typedef float v16f __attribute__((ext_vector_type(16)));
constexpr int kPruneWaves = 4;
constexpr int kPruneHyps = 32;    // per wave: the columns of a tile, one per lane of a half
constexpr int kPruneTile = 32;    // matches per tile: its rows
constexpr int kPruneOGT = 2;      // __builtin_amdgcn_fcmpf: llvm::FCmpInst::FCMP_OGT

// tile row (a match) held by accumulator register r of a lane in half `half` (cdna4 ISA, 32x32 C/D layout)
__host__ __device__ constexpr int prune_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// A lane's B operands for its hypothesis: lower half even k, upper half odd k; k = 9 (n) and k = 3 (a0) are the zero padding.
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

// One tile: n and a0 of 32 matches x 32 hypotheses.  The lane brings the coordinates of match (row) l & 31; phi_k for
// k = 2 s + (l >> 5) is its A operand of step s, and F_k of hypothesis (column) l & 31 its B operand.  The last two steps of n
// (x1 | y1, 1 | 0) are the two steps of a0.  Register r of the lane then holds match prune_row(r, half) of the tile for the
// lane's own hypothesis.
__device__ __forceinline__ void prune_tile(const PruneA &A, bool half, float x1, float y1, float x2, float y2, v16f &n, v16f &a0) {
    const float p = x2 * (half ? y1 : x1);   // phi_0 | phi_1
    const float q = y2 * (half ? x1 : y1);   // phi_4 | phi_3
    const float b1 = half ? q : x2, b2 = half ? y2 : q, b3 = half ? y1 : x1, b4 = half ? 0.f : 1.f;
    v16f z;
#pragma unroll
    for (int r = 0; r < 16; r++) z[r] = 0.f;
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(p, A.n[0], z, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, A.n[1], n, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(b2, A.n[2], n, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(b3, A.n[3], n, 0, 0, 0);
    n = __builtin_amdgcn_mfma_f32_32x32x2f32(b4, A.n[4], n, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b3, A.d[0], z, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b4, A.d[1], a0, 0, 0, 0);
}

// The certified misses of the lane's hypothesis among its sixteen matches of one tile: pc_miss (ransac_prune_cert.h) per
// register, |n| > fma(s+, |a0|, c), ordered -- each a v_cmp whose carry is added into the lane's own counter.
__device__ __forceinline__ int prune_count(const v16f &n, const v16f &a0, float splus, float c, int cnt) {
#pragma unroll
    for (int r = 0; r < 16; r++) cnt += fabsf(n[r]) > fmaf(splus, fabsf(a0[r]), c) ? 1 : 0;
    return cnt;
}
// The same for a partial tile: only rows below `rows` hold a match.  rem = rows - 4 * half, the bound on the part of prune_row
// that does not depend on the lane (one register for it, and the sixteen row numbers stay constants).
__device__ __forceinline__ int prune_count(const v16f &n, const v16f &a0, float splus, float c, int cnt, int rem) {
#pragma unroll
    for (int r = 0; r < 16; r++)
        cnt += (prune_row(r, 0) < rem && fabsf(n[r]) > fmaf(splus, fabsf(a0[r]), c)) ? 1 : 0;
    return cnt;
}

// The head of a pair on the certificate, for the pairs vs_head_on_certificate (ransac_residual.h) sends this way -- their
// hypotheses have to miss more matches than the head holds, nearly all of them garbage the prune kernel then kills:
// pot0[h] = n0 - X[h], X the certified misses among the ranked matches [0, n0), instead of the cheap evaluation's count: an
// upper bound of the head's inliers all the same, which is all ransac_cand_kernel, the prune kernel and ransac_count_kernel
// rely on.  head[h] = (uncertified, 0): a survivor of the count kernel evaluates the head itself and takes no sum from here.
// A hypothesis outside the certificate's ranges or with a NaN in F certifies nothing: pot0 = n0.
// One wave: the 32 hypotheses from hbase on (the prune kernel's mapping: a lane counts its own hypothesis, X = the counts of
// its two halves), four tiles at most, no stop rule.  m >= 1.
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

    const float *r1 = rk + (size_t)b * 4 * kp_pad, *r2 = r1 + kp_pad, *r3 = r2 + kp_pad, *r4 = r3 + kp_pad;
    float x1[kHeadTiles], y1[kHeadTiles], x2[kHeadTiles], y2[kHeadTiles];
#pragma unroll
    for (int t = 0; t < kHeadTiles; t++) {
        const int j = min(t * kPruneTile + col, m - 1);   // rows beyond n0 read a real match and are masked
        x1[t] = r1[j];
        y1[t] = r2[j];
        x2[t] = r3[j];
        y2[t] = r4[j];
    }
    int cnt = 0;   // certified misses of the lane's hypothesis among the matches its half holds
#pragma unroll
    for (int t = 0; t < kHeadTiles; t++) {
        if (t * kPruneTile >= n0) break;   // wave-uniform
        v16f n, a0;
        prune_tile(A, half, x1[t], y1[t], x2[t], y2[t], n, a0);
        if ((t + 1) * kPruneTile <= n0)   // wave-uniform: a full tile
            cnt = prune_count(n, a0, splus, c, cnt);
        else
            cnt = prune_count(n, a0, splus, c, cnt, n0 - t * kPruneTile - (half ? 4 : 0));
    }
    const int xv = cnt + __shfl_xor(cnt, 32, 64);   // X of hypothesis l & 31
    if (!half && h < hyp) {
        pot0[hi] = n0 - xv;
        head[hi] = make_int2(kVsHeadUncertified, 0);
    }
}

#ifdef VSLAM_EXPERIMENTS
// (experiments build only, VSLAM_RANSAC_PRUNE_ROWS) The form this one replaced, kept for the identity test and for A/B timing
// inside one library: a hypothesis per tile ROW (F is the A operand, phi the B operand), so a lane's sixteen registers belong
// to sixteen hypotheses, the misses leave the vector pipe as compare masks and are counted with s_bcnt1 on each 32-lane half
// into 32 scalar X.  n and a0 are the same fma chains element for element (the products commute, k runs in the same order).
__device__ __forceinline__ void prune_tile_rows(const PruneA &A, bool half, float x1, float y1, float x2, float y2, v16f &n, v16f &a0) {
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

__device__ __forceinline__ void head_on_certificate_rows(const float *__restrict__ rk, int kp_pad, int b, int m, int n0, int hbase, int hyp,
                                                         float threshold, float splus, const float *__restrict__ hypF,
                                                         const float *__restrict__ cmax, int32_t *__restrict__ pot0, int2 *__restrict__ head) {
    const int lane = threadIdx.x & 63, col = lane & 31;
    const bool half = lane >= 32;
    const int h = hbase + col;
    const size_t hi = (size_t)b * hyp + min(h, hyp - 1);
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = hypF[hi * 9 + k];
    const float c = pc_margin(f, cmax[2 * b], cmax[2 * b + 1], threshold, splus);
    const PruneA A = prune_operands(f, half);
    float cr[16];   // c of the hypothesis each accumulator register holds in this lane
#pragma unroll
    for (int r = 0; r < 16; r++) cr[r] = __shfl(c, half ? prune_row(r, 1) : prune_row(r, 0), 64);

    const float *r1 = rk + (size_t)b * 4 * kp_pad, *r2 = r1 + kp_pad, *r3 = r2 + kp_pad, *r4 = r3 + kp_pad;
    float x1[kHeadTiles], y1[kHeadTiles], x2[kHeadTiles], y2[kHeadTiles];
#pragma unroll
    for (int t = 0; t < kHeadTiles; t++) {
        const int j = min(t * kPruneTile + col, m - 1);
        x1[t] = r1[j];
        y1[t] = r2[j];
        x2[t] = r3[j];
        y2[t] = r4[j];
    }
    int X[kPruneHyps];
#pragma unroll
    for (int i = 0; i < kPruneHyps; i++) X[i] = 0;
#pragma unroll
    for (int t = 0; t < kHeadTiles; t++) {
        if (t * kPruneTile >= n0) break;   // wave-uniform
        v16f n, a0;
        prune_tile_rows(A, half, x1[t], y1[t], x2[t], y2[t], n, a0);
        const unsigned long long valid = __ballot(t * kPruneTile + col < n0);
#pragma unroll
        for (int r = 0; r < 16; r++) {
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
#endif

}  // namespace vs_prune

// VSLAM_RANSAC_PRUNE_ROWS=1 (experiments build; the product reads no environment variable): the prune kernel and the screen's
// head path in the row-per-hypothesis form.  Read at every call: a test switches it within a process.
inline bool vs_prune_rows_form() {
    const char *e = VS_EXPERIMENT_ENV("VSLAM_RANSAC_PRUNE_ROWS");
    return e != nullptr && atoi(e) != 0;
}
