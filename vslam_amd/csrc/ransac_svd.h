// OpenCV's one-sided Jacobi SVD (JacobiSVDImpl_<float>) replayed on per-lane matrices held in LDS.  Device helpers of
// ransac_solve.hip; no kernel lives here.
//
// Stands in for the two cv::SVDecomp calls of RansacFilter::compute_fundamental (the reference's src/RansacFilter.cpp:94
// on the 8 x 9 design matrix, :98 on the 3 x 3 F0).
//
// Numerics: OpenCV's Jacobi keeps double accumulators and float rotations; the code here executes the same operations in
// the same order (no FMA contraction: the library is built with -ffp-contract=off; explicit fma() is used only where the
// product of two floats is exact in double, which makes fma == mul+add bit for bit).  std::hypot is pinned to
// sqrt(p*p + beta*beta) on both sides.  The shortened sqrt / division sequences and the square-root-free
// convergence test are taken only where they give the same bits; each states its range argument.
#pragma once

#include "ctx.h"

#include <cfloat>

namespace vs_ransac {

constexpr int kSolveThreads = 64;

__device__ __forceinline__ uint32_t cvrng_next(uint64_t &state) {   // cv::RNG (MWC)
    state = (uint64_t)(uint32_t)state * 4164903690ull + (uint32_t)(state >> 32);
    return (uint32_t)state;
}

// Element (r,k) of this lane's matrix; lanes are interleaved so every ds access is conflict-free.
#define VS_A(r, k) sA[((r) * M + (k)) * kSolveThreads + tid]
#define VS_V(r, k) sV[((r) * N + (k)) * kSolveThreads + tid]

// JacobiSVDImpl_(At, astep, W, Vt, vstep, m = M, n = N, n1 = N1, FLT_MIN, FLT_EPSILON*2).
// Rows 0..N-1 of A are orthogonalised; rows up to N1-1 are normalised / generated.
// wout receives (float)W[i].
// OpenCV keeps the squared row norms W[] between rotations; every W[i] it reads is the k-ordered double
// sum of squares of the CURRENT row i (set so at start-up and after each rotation of that row), so the
// norms are recomputed from the rows where needed instead of being stored: same bits, and the LDS
// footprint per lane drops by 64 B, which is what bounds this kernel's occupancy.
// fabs(p) <= eps * sqrt(a * b) with eps = 2 * FLT_EPSILON = 2^-22, decided without the square root where that is
// safe.  With y = |p| * 2^22 (exact) and x = fl(a * b) the test is y <= RN(sqrt(x)); rounding is monotone, so it
// equals y * y <= x except when x lies within an ulp or so of y * y.  h = fl(y * y) decides every case in which h
// and x differ by more than 2^-50 relative; if any lane of the wave is closer than that (or x is 0) the wave
// evaluates the original expression.
__device__ __forceinline__ bool jacobi_converged(double p, double a, double b) {
    const double y = fabs(p) * 4194304.0;
    const double x = a * b;
    const double h = y * y;
    const bool near = !(fabs(h - x) > x * 0x1p-50);   // also true for NaN / zero
    if (__any(near)) return fabs(p) <= (double)(FLT_EPSILON * 2) * sqrt(x);
    return h < x;
}

// sqrt(x) and x / y for operands in a comfortable exponent range: the instruction sequences hipcc emits for the
// IEEE-correct f64 sqrt and division (v_rsq_f64 / v_rcp_f64 + the Goldschmidt / Newton corrections) without
// the parts that only act on extreme exponents, zeros, infinities and NaNs (v_ldexp rescaling and the class
// select for sqrt; v_div_scale, the scale fix-up of v_div_fmas and v_div_fixup for division) — outside those
// cases these leave the value untouched, so the results are the same bits for 37 resp. 16 fewer issue cycles.
__device__ __forceinline__ double sqrt_inrange(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
__device__ __forceinline__ double div_inrange(double x, double y) {
    double r = __builtin_amdgcn_rcp(y);
    double f = __builtin_fma(-y, r, 1.0);
    r = __builtin_fma(r, f, r);
    f = __builtin_fma(-y, r, 1.0);
    r = __builtin_fma(r, f, r);
    const double q = x * r;
    const double e = __builtin_fma(-y, q, x);
    return __builtin_fma(e, r, q);
}

// Everything after the sweeps: W, the descending sort (rows travel with W), normalisation / regeneration of the rows,
// the row beyond the rank.  The matrix is reached through pA / pV with element stride SA, so the same code runs on a
// lane's LDS columns (SA = kSolveThreads) and on a private copy (SA = 1).
#define FA(r, k) pA[((r) * M + (k)) * SA]
#define FV(r, k) pV[((r) * N + (k)) * SA]
template <int M, int N, int N1, bool HASV, int SA>
__device__ __forceinline__ void jacobi_finish(float *pA, float *pV, float *wout, float *extra_row) {
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    double W[N];   // singular values: registers, every index below is compile-time
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) {
            const float t = FA(i, k);
            sd = __builtin_fma((double)t, (double)t, sd);
        }
        W[i] = sqrt(sd);
    }

#pragma unroll
    for (int i = 0; i < N - 1; i++) {   // selection sort, descending, rows travel with W
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < N; k++)
            if (wj < W[k]) {
                j = k;
                wj = W[k];
            }
        if (i != j) {
#pragma unroll
            for (int jj = i + 1; jj < N; jj++)
                if (jj == j) W[jj] = W[i];
            W[i] = wj;
#pragma unroll
            for (int k = 0; k < M; k++) {
                const float x = FA(i, k), y = FA(j, k);
                FA(i, k) = y;
                FA(j, k) = x;
            }
            if (HASV) {
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const float x = FV(i, k), y = FV(j, k);
                    FV(i, k) = y;
                    FV(j, k) = x;
                }
            }
        }
    }

#pragma unroll
    for (int i = 0; i < N; i++) wout[i] = (float)W[i];

    uint64_t rng = 0x12345678ull;
    for (int i = 0; i < N; i++) {
        double sd = 0;   // W[i] again: the sorted row's norm
#pragma unroll
        for (int k = 0; k < M; k++) {
            const float t = FA(i, k);
            sd = __builtin_fma((double)t, (double)t, sd);
        }
        sd = sqrt(sd);
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / M);
#pragma unroll
            for (int k = 0; k < M; k++) FA(i, k) = (cvrng_next(rng) & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; iter++) {
                for (int j = 0; j < i; j++) {
                    float vi[M], vj[M];
                    sd = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) {
                        vi[k] = FA(i, k);
                        vj[k] = FA(j, k);
                        sd += (double)(vi[k] * vj[k]);   // float product, double running sum
                    }
                    float asum = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) {
                        const float t = (float)((double)vi[k] - sd * (double)vj[k]);
                        vi[k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
#pragma unroll
                    for (int k = 0; k < M; k++) FA(i, k) = vi[k] * asum;
                }
            }
            sd = 0;
#pragma unroll
            for (int k = 0; k < M; k++) {
                const float t = FA(i, k);
                sd = __builtin_fma((double)t, (double)t, sd);
            }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
#pragma unroll
        for (int k = 0; k < M; k++) FA(i, k) = FA(i, k) * s;
    }
    if (N1 > N) {
        // the row beyond the rank (FULL_UV): same procedure with i = N, W = 0; it lives in registers,
        // which keeps the per-lane LDS footprint at N rows
        float v[M];
        double sd = 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / M);
#pragma unroll
            for (int k = 0; k < M; k++) v[k] = (cvrng_next(rng) & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; iter++) {
                for (int j = 0; j < N; j++) {
                    float vj[M];
                    sd = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) {
                        vj[k] = FA(j, k);
                        sd += (double)(v[k] * vj[k]);
                    }
                    float asum = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) {
                        const float t = (float)((double)v[k] - sd * (double)vj[k]);
                        v[k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
#pragma unroll
                    for (int k = 0; k < M; k++) v[k] = v[k] * asum;
                }
            }
            sd = 0;
#pragma unroll
            for (int k = 0; k < M; k++) sd = __builtin_fma((double)v[k], (double)v[k], sd);
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
#pragma unroll
        for (int k = 0; k < M; k++) extra_row[k] = v[k] * s;
    }
}
#undef FA
#undef FV

template <int M, int N, int N1, bool HASV>
__device__ void jacobi_svd_lanes(float *sA, float *sV, int tid, float *wout, float *extra_row) {
    static_assert(N1 == N || N1 == N + 1, "FULL_UV asks for at most one row beyond the rank here");
    constexpr int max_iter = M > 30 ? M : 30;

    if (HASV) {
        for (int i = 0; i < N; i++) {
#pragma unroll
            for (int k = 0; k < N; k++) VS_V(i, k) = (i == k) ? 1.f : 0.f;
        }
    }

    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < N - 1; i++)
            for (int j = i + 1; j < N; j++) {
                float ai[M], aj[M];
                double a = 0, p = 0, b = 0;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    ai[k] = VS_A(i, k);
                    aj[k] = VS_A(j, k);
                    const double di = (double)ai[k], dj = (double)aj[k];
                    p = __builtin_fma(di, dj, p);
                    a = __builtin_fma(di, di, a);   // W[i]
                    b = __builtin_fma(dj, dj, b);   // W[j]
                }
                if (jacobi_converged(p, a, b)) continue;

                p *= 2;
                const double beta = a - b;
                const double g2 = p * p + beta * beta;
                float c, s;
                // With g2 and p in this range every operand and quotient below stays within 2^+-500 (gamma <= 2^200,
                // the two ratios under the square roots lie in [1/2, 1], |p / (gamma * s * 2)| >= 2^-500), where the
                // short sequences equal the full ones; otherwise the whole wave takes sqrt() and '/'.
                const bool safe = g2 > 0x1p-400 && g2 < 0x1p400 && fabs(p) > 0x1p-300;
                if (!__any(!safe)) {
                    const double gamma = sqrt_inrange(g2);   // pinned hypot
                    if (beta < 0) {
                        const double delta = (gamma - beta) * 0.5;
                        s = (float)sqrt_inrange(div_inrange(delta, gamma));
                        c = (float)div_inrange(p, gamma * (double)s * 2);
                    } else {
                        c = (float)sqrt_inrange(div_inrange(gamma + beta, gamma * 2));
                        s = (float)div_inrange(p, gamma * (double)c * 2);
                    }
                } else {
                    const double gamma = sqrt(g2);   // pinned hypot
                    if (beta < 0) {
                        const double delta = (gamma - beta) * 0.5;
                        s = (float)sqrt(delta / gamma);
                        c = (float)(p / (gamma * (double)s * 2));
                    } else {
                        c = (float)sqrt((gamma + beta) / (gamma * 2));
                        s = (float)(p / (gamma * (double)c * 2));
                    }
                }
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float t0 = c * ai[k] + s * aj[k];
                    const float t1 = (-s) * ai[k] + c * aj[k];
                    VS_A(i, k) = t0;
                    VS_A(j, k) = t1;
                }
                changed = true;
                if (HASV) {
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        const float vi = VS_V(i, k), vj = VS_V(j, k);
                        const float t0 = c * vi + s * vj;
                        const float t1 = (-s) * vi + c * vj;
                        VS_V(i, k) = t0;
                        VS_V(j, k) = t1;
                    }
                }
            }
        if (!changed) break;
    }

    jacobi_finish<M, N, N1, HASV, kSolveThreads>(sA + tid, HASV ? sV + tid : nullptr, wout, extra_row);
}

}  // namespace vs_ransac
