// The residual of one correspondence under F as the reference evaluates it: what ransac_count.hip and ransac_select.hip
// share.  Device helpers only; no kernel lives here.
//
// Replaces the per-correspondence arithmetic of RansacFilter::compute_fundamental_residual (the reference's
// src/RansacFilter.cpp:119-126).
//
// Numerics: bit-exact.  Same IEEE operations in the same order as the reference's OpenCV expressions (no FMA contraction:
// -ffp-contract=off; explicit fma() only where the product of two floats is exact in double).  Every inlier decision
// (e <= threshold) and every residual sum the accept rule sees is made from these values.
#pragma once

#include "ctx.h"

namespace vs_ransac {

// e for one correspondence under F, exactly as RansacFilter.cpp:119-126 evaluates it through
// OpenCV: F*x1 in float (left to right), F.t()*x2 in double with one rounding, the row reduce
// as (r0 + r1) + r2, and n*n / a*a + b*b + c*c + d*d with C++ precedence.
struct ResidualF {
    float f[9];
    double ft[6];   // F[0],F[3],F[6], F[1],F[4],F[7] as doubles
};
__device__ __forceinline__ void residual_prepare(ResidualF &R) {
    R.ft[0] = (double)R.f[0];
    R.ft[1] = (double)R.f[3];
    R.ft[2] = (double)R.f[6];
    R.ft[3] = (double)R.f[1];
    R.ft[4] = (double)R.f[4];
    R.ft[5] = (double)R.f[7];
}
__device__ __forceinline__ float residual_e(const ResidualF &R, const float4 c, const double dx2, const double dy2) {
    const float x1 = c.x, y1 = c.y, x2 = c.z, y2 = c.w;
    const float a0 = R.f[0] * x1 + R.f[1] * y1 + R.f[2];
    const float a1 = R.f[3] * x1 + R.f[4] * y1 + R.f[5];
    const float a2 = R.f[6] * x1 + R.f[7] * y1 + R.f[8];
    // products of two floats are exact in double: fma(a,b,c) == a*b + c rounded once
    const float t0 = (float)(__builtin_fma(R.ft[1], dy2, R.ft[0] * dx2) + R.ft[2]);
    const float t1 = (float)(__builtin_fma(R.ft[4], dy2, R.ft[3] * dx2) + R.ft[5]);
    const float n = (x2 * a0 + y2 * a1) + a2;
    const float q = (n * n) / (a0 * a0);
    return ((q + a1 * a1) + t0 * t0) + t1 * t1;
}

// Two correspondences at once: the float multiplies and adds become v_pk_mul_f32 / v_pk_add_f32 (IEEE, same
// roundings as the scalar forms), which halves the float instruction count of the hot loop; the double
// part (F.t()*x2) and the division stay per element.  Lane .x is the lower correspondence index.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f residual_e2(const ResidualF &R, const v2f x1, const v2f y1, const v2f x2, const v2f y2,
                                           const double2 da, const double2 db) {
    const v2f a0 = (R.f[0] * x1 + R.f[1] * y1) + R.f[2];
    const v2f a1 = (R.f[3] * x1 + R.f[4] * y1) + R.f[5];
    const v2f a2 = (R.f[6] * x1 + R.f[7] * y1) + R.f[8];
    v2f t0, t1;
    t0.x = (float)(__builtin_fma(R.ft[1], da.y, R.ft[0] * da.x) + R.ft[2]);
    t0.y = (float)(__builtin_fma(R.ft[1], db.y, R.ft[0] * db.x) + R.ft[2]);
    t1.x = (float)(__builtin_fma(R.ft[4], da.y, R.ft[3] * da.x) + R.ft[5]);
    t1.y = (float)(__builtin_fma(R.ft[4], db.y, R.ft[3] * db.x) + R.ft[5]);
    const v2f n = (x2 * a0 + y2 * a1) + a2;
    const v2f nn = n * n, dd = a0 * a0;
    v2f q;
    q.x = nn.x / dd.x;
    q.y = nn.y / dd.y;
    return ((q + a1 * a1) + t0 * t0) + t1 * t1;
}

}  // namespace vs_ransac

// The counts-first scoring up to and including ransac_count_kernel (ransac_count.hip), called by vs_launch_ransac_evaluate
// (ransac_select.hip) and by nobody else.  approx: 2 floats per hypothesis, the cheap sum and its error bound.
int vs_launch_ransac_count(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs, const int32_t *m,
                           const float *hypF, int batch, int kp_stride, int hyp, float threshold, int32_t *hyp_count,
                           float *hyp_sum, float *approx);

// Between ransac_cand_kernel and ransac_count_kernel (ransac_prune.hip): hypotheses whose certified misses behind the head keep
// them below cbound get pot0 = -(m - n0) - 1, which ransac_count_kernel reads as "ruled out".  n_head: the screen's matches.
int vs_launch_ransac_prune(vslam_ctx *ctx, const float *rk, int kp_pad, const int32_t *m, int min_m, int kp_stride, int hyp,
                           float threshold, const float *hypF, const float *cmax, const int32_t *cbound, int32_t *pot0, int batch,
                           int n_head);

// The word the head's kernel hands on per hypothesis beside pot0 where nothing of the head is certified (ransac_count.hip).
constexpr int kVsHeadUncertified = -1;

// Which kernel forms pot0 on a pair's head (its n0 most-missed matches).  A pair whose hypotheses have to miss more matches
// than the head holds -- the prune gate's form, with the pilots' bound that ransac_rank_kernel has stored by then, never
// above the bound the gate sees: every pair the prune kernel walks is among them -- takes the certificate
// (head_on_certificate, ransac_prune_tile.h: certified misses only, nothing exact handed on); every other pair takes the cheap
// evaluation, whose exact head counts and sums its survivors live on.  route: -1 = by this rule, 0 / 1 = every pair to the
// cheap evaluation / to the certificate (experiments build, VSLAM_RANSAC_HEAD_ROUTE).  ransac_screen_kernel branches on it per
// workgroup.  (A pair without a match stays with the cheap evaluation: the certificate's lanes read ranked match m - 1 where
// they have none of their own.)
__host__ __device__ constexpr bool vs_head_on_certificate(int m, int bound, int n0, int route) {
    return m > 0 && (route < 0 ? m - bound + 1 > n0 : route != 0);
}
