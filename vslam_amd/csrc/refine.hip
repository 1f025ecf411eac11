// Two-view bundle adjustment of each pair's pose and points (vslam_refine_pairs, include/vslam_amd.h): the step the reference
// left as an empty `struct optimizer` (src/optimzer.cpp).  One workgroup of 256 lanes per pair, everything in f64 and never fused;
// lane l owns the points i = l (mod 256).  A point's accepted and candidate coordinates stay in f64 from the first iteration to
// the last: in LDS when the pair's n fits the launch's dynamic LDS, in an arena workspace otherwise -- the arithmetic is the same,
// only the address differs.  Sums follow refit.hip's rule (strided partial sums, a butterfly inside the wave, the four wave sums
// in order), so a pair's bits depend on the pair alone.
#include "ctx.h"
#include "refine_math.h"

#pragma clang fp contract(off)

using namespace vs_refine;

namespace {
constexpr int kBT = 256;        // lanes per pair
constexpr int kBW = kBT / 64;   // waves per pair
constexpr int kStateBytes = 6 * 8 + 1;                   // per point: accepted and candidate (x, y, z) f64, one flag byte
constexpr int kLdsPoints = 3200;                         // most points whose state fits beside the 896 B of static LDS

template <int N>
__device__ __forceinline__ void ba_block_sum(double (&v)[N], double *lds /* [kBW][N] */) {
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

struct BaK {
    float v[9];
};

__global__ __launch_bounds__(kBT) void refine_pairs_kernel(const float *__restrict__ xy1, const float *__restrict__ xy2,
                                                           const int32_t *__restrict__ matches, const int32_t *__restrict__ best,
                                                           int kp_stride, BaK Kc, double gate_sq, int max_iterations, float *R_io,
                                                           float *t_io, float *__restrict__ c2_out, float *points4d,
                                                           double *__restrict__ stats, int lds_points, double *arena_state,
                                                           uint8_t *arena_flags) {
    extern __shared__ __align__(16) unsigned char ba_dyn[];
    __shared__ double red[kBW * 20];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *p1 = xy1 + (size_t)b * kp_stride * 2, *p2 = xy2 + (size_t)b * kp_stride * 2;
    const int32_t *mt = matches + (size_t)b * kp_stride * 2;
    float *P = points4d + (size_t)b * kp_stride * 4;
    const int winner = best[b * 4 + 0];
    int n = best[b * 4 + 3];
    n = n < 0 ? 0 : (n > kp_stride ? kp_stride : n);
    // R and t are read by every lane before the first barrier and written behind the last one
    float Rin32[9], tin32[3];
    double K[9];
    BaCam in;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        Rin32[k] = R_io[(size_t)b * 9 + k];
        in.R[k] = (double)Rin32[k];
        K[k] = (double)Kc.v[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tin32[k] = t_io[(size_t)b * 3 + k];
        in.t[k] = (double)tin32[k];
    }
    // the point state: [2][3][cap] doubles (accepted / candidate) and [cap] flags, in LDS when n fits and in the arena otherwise
    const bool in_lds = n <= lds_points;
    const int cap = in_lds ? lds_points : kp_stride;
    double *st = in_lds ? reinterpret_cast<double *>(ba_dyn) : arena_state + (size_t)b * 6 * kp_stride;
    uint8_t *fl = in_lds ? ba_dyn + (size_t)48 * lds_points : arena_flags + (size_t)b * kp_stride;

    auto observed = [&](int i, double (&o)[4]) -> bool {
        const int a = mt[2 * i], c = mt[2 * i + 1];
        if (a < 0 || a >= kp_stride || c < 0 || c >= kp_stride) return false;
        o[0] = (double)p1[2 * a]; o[1] = (double)p1[2 * a + 1];
        o[2] = (double)p2[2 * c]; o[3] = (double)p2[2 * c + 1];
        return true;
    };

    // 1. the participating correspondences, fixed here; their count and objective under the inputs
    double s2[2] = {0, 0};
    for (int i = tid; i < n; i += kBT) {
        double o[4], X[3], e1, e2, dz;
        bool part = observed(i, o);
        if (part) {
#pragma unroll
            for (int k = 0; k < 3; k++) X[k] = (double)P[4 * i + k];
            ba_errors(K, in, X, o, e1, e2, dz);
            part = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && X[2] > 0.0 && dz > 0.0 && e1 <= gate_sq && e2 <= gate_sq;
        }
        fl[i] = part ? 1 : 0;
        if (part) {
#pragma unroll
            for (int k = 0; k < 3; k++) st[(size_t)k * cap + i] = X[k];
            s2[0] += 1.0;
            s2[1] += e1 + e2;
        }
    }
    ba_block_sum(s2, red);
    const double cnt = s2[0];
    const double qnan = __builtin_nan("");
    const double tn = sqrt((in.t[0] * in.t[0] + in.t[1] * in.t[1]) + in.t[2] * in.t[2]);
    const bool t_ok = isfinite(in.t[0]) && isfinite(in.t[1]) && isfinite(in.t[2]) && tn > 0.0;

    // c2 = K [R | t] in f64, products summed left to right, one rounding
    auto camera = [&](const BaCam &c, float (&c2)[12]) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int k = 0; k < 3; k++) c2[4 * r + k] = (float)((K[3 * r] * c.R[k] + K[3 * r + 1] * c.R[3 + k]) + K[3 * r + 2] * c.R[6 + k]);
            c2[4 * r + 3] = (float)((K[3 * r] * c.t[0] + K[3 * r + 1] * c.t[1]) + K[3 * r + 2] * c.t[2]);
        }
    };
    auto leave_alone = [&]() {
        if (tid == 0) {
            float c2[12];
            camera(in, c2);
#pragma unroll
            for (int k = 0; k < 9; k++) R_io[(size_t)b * 9 + k] = Rin32[k];
#pragma unroll
            for (int k = 0; k < 3; k++) t_io[(size_t)b * 3 + k] = tin32[k];
#pragma unroll
            for (int k = 0; k < 12; k++) c2_out[(size_t)b * 12 + k] = c2[k];
            if (stats) {
                stats[(size_t)b * 4 + 0] = cnt;
                stats[(size_t)b * 4 + 1] = stats[(size_t)b * 4 + 2] = stats[(size_t)b * 4 + 3] = qnan;
            }
        }
    };
    if (winner < 0 || cnt < 8.0 || !t_ok) {   // the same in every lane
        leave_alone();
        return;
    }
    const double mean_in = s2[1] / (2.0 * cnt);

    // 2. the start: R one Newton step of the polar iteration closer to a rotation, R (3 I - R^t R) / 2; t / |t|
    BaCam cur;
    ba_start(in, tn, cur);
    int acc_buf = 0;   // which half of the state holds the accepted points
    auto state = [&](int buf, int k, int i) -> double & { return st[((size_t)buf * 3 + k) * cap + i]; };

    double s1[1] = {0};
    for (int i = tid; i < n; i += kBT) {
        if (!fl[i]) continue;
        double o[4], e1, e2, dz;
        observed(i, o);
        const double X[3] = {state(0, 0, i), state(0, 1, i), state(0, 2, i)};
        ba_errors(K, cur, X, o, e1, e2, dz);
        s1[0] += e1 + e2;
    }
    ba_block_sum(s1, red);
    double obj = s1[0], lambda = kLambda0;
    int accepted = 0;

    // 3. Levenberg-Marquardt
    for (int it = 0; it < max_iterations; it++) {
        double b1[3], b2[3];
        ba_tangent(cur.t, b1, b2);
        double acc[20];
#pragma unroll
        for (int k = 0; k < 20; k++) acc[k] = 0.0;
        int bad = 0;
        for (int i = tid; i < n; i += kBT) {
            if (!fl[i]) continue;
            double o[4], Yv[3][5], z[3], a[20];
            observed(i, o);
            const double X[3] = {state(acc_buf, 0, i), state(acc_buf, 1, i), state(acc_buf, 2, i)};
            if (!ba_point_blocks(K, cur, b1, b2, lambda, X, o, Yv, z, a)) bad = 1;
#pragma unroll
            for (int k = 0; k < 20; k++) acc[k] += a[k];
        }
        ba_block_sum(acc, red);
        bad = __syncthreads_or(bad);
        // the reduced system by Cholesky, in every lane
        double dc[5];
        const bool ok = !bad && ba_reduced_solve(acc, dc);
        bool accept = false;
        double obj_new = 0.0;
        BaCam cand;
        if (ok) {   // the same in every lane
            ba_candidate(cur, b1, b2, dc, cand);
            double so[1] = {0};
            int behind = 0;
            for (int i = tid; i < n; i += kBT) {
                if (!fl[i]) continue;
                double o[4], Yv[3][5], z[3], a[20], Xn[3], e1, e2, dz;
                observed(i, o);
                const double X[3] = {state(acc_buf, 0, i), state(acc_buf, 1, i), state(acc_buf, 2, i)};
                ba_point_blocks(K, cur, b1, b2, lambda, X, o, Yv, z, a);
                ba_point_step(X, Yv, z, dc, Xn);
#pragma unroll
                for (int k = 0; k < 3; k++) state(acc_buf ^ 1, k, i) = Xn[k];
                ba_errors(K, cand, Xn, o, e1, e2, dz);
                so[0] += e1 + e2;
                if (!(Xn[2] > 0.0) || !(dz > 0.0)) behind = 1;
            }
            ba_block_sum(so, red);
            behind = __syncthreads_or(behind);
            obj_new = so[0];
            accept = !behind && obj_new < obj;   // false for a NaN objective
        }
        if (accept) {
            const double rel = (obj - obj_new) / obj;
            cur = cand;
            obj = obj_new;
            acc_buf ^= 1;
            accepted++;
            lambda = fmax(lambda / 10.0, kLambdaMin);
            if (rel < kRelStop) break;
        } else {
            lambda = lambda * 10.0;
            if (lambda > kLambdaMax) break;
        }
    }
    if (accepted == 0) {
        leave_alone();
        return;
    }

    // 4. one rounding to f32; anything not finite leaves the item alone
    float R32[9], t32[3], c2[12];
    BaCam outc;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        R32[k] = (float)cur.R[k];
        outc.R[k] = (double)R32[k];
        finite = finite && isfinite(R32[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        t32[k] = (float)cur.t[k];
        outc.t[k] = (double)t32[k];
        finite = finite && isfinite(t32[k]);
    }
    camera(cur, c2);
#pragma unroll
    for (int k = 0; k < 12; k++) finite = finite && isfinite(c2[k]);
    int nonfinite = finite ? 0 : 1;
    double sf[1] = {0};
    for (int i = tid; i < n; i += kBT) {
        if (!fl[i]) continue;
        double o[4], Xf[3], e1, e2, dz;
        observed(i, o);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float x32 = (float)state(acc_buf, k, i);
            if (!isfinite(x32)) nonfinite = 1;
            Xf[k] = (double)x32;
        }
        ba_errors(K, outc, Xf, o, e1, e2, dz);
        sf[0] += e1 + e2;
    }
    ba_block_sum(sf, red);
    nonfinite = __syncthreads_or(nonfinite);
    if (nonfinite) {
        leave_alone();
        return;
    }
    for (int i = tid; i < n; i += kBT) {
        if (!fl[i]) continue;
        reinterpret_cast<float4 *>(P)[i] =
            make_float4((float)state(acc_buf, 0, i), (float)state(acc_buf, 1, i), (float)state(acc_buf, 2, i), 1.f);
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) R_io[(size_t)b * 9 + k] = R32[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t_io[(size_t)b * 3 + k] = t32[k];
#pragma unroll
        for (int k = 0; k < 12; k++) c2_out[(size_t)b * 12 + k] = c2[k];
        if (stats) {
            stats[(size_t)b * 4 + 0] = cnt;
            stats[(size_t)b * 4 + 1] = mean_in;
            stats[(size_t)b * 4 + 2] = sf[0] / (2.0 * cnt);
            stats[(size_t)b * 4 + 3] = (double)accepted;
        }
    }
}
}  // namespace

int vs_launch_refine_pairs(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *matches, const int32_t *best, int batch,
                           int kp_stride, const float *h_K, float gate_sq, int max_iterations, float *R, float *t, float *c2,
                           float *points4d, double *stats) {
    VS_REQUIRE(ctx, xy1 && xy2 && matches && best && h_K && R && t && c2 && points4d, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && kp_stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, max_iterations >= 1 && max_iterations <= 64, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, gate_sq > 0.f && gate_sq <= 3.402823466e38f, VSLAM_ERR_INVALID);   // false for NaN and infinity
    BaK K;
    for (int i = 0; i < 9; i++) K.v[i] = h_K[i];
    const int lds_points = kp_stride < kLdsPoints ? ((kp_stride + 7) & ~7) : kLdsPoints;
    const size_t lds_bytes = (size_t)kStateBytes * lds_points;
    double *arena_state = nullptr;
    uint8_t *arena_flags = nullptr;
    int rc;
    if (kp_stride > lds_points) {   // a pair may hold more points than the LDS takes
        if ((rc = vs_arena_get(ctx, "refine.state", sizeof(double) * 6 * (size_t)batch * kp_stride, (void **)&arena_state))) return rc;
        if ((rc = vs_arena_get(ctx, "refine.flags", (size_t)batch * kp_stride, (void **)&arena_flags))) return rc;
    }
    if (lds_bytes > 48 * 1024 && (rc = vs_allow_dynamic_lds(ctx, refine_pairs_kernel, "refine_pairs", (size_t)kStateBytes * kLdsPoints)))
        return rc;
    VsProfScope ps(ctx, "refine_pairs_kernel");
    refine_pairs_kernel<<<batch, kBT, lds_bytes, ctx->stream>>>(xy1, xy2, matches, best, kp_stride, K, (double)gate_sq, max_iterations, R,
                                                               t, c2, points4d, stats, lds_points, arena_state, arena_flags);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

extern "C" int vslam_refine_pairs(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const int32_t *d_matches,
                                  const int32_t *d_best, int batch, int kp_stride, const float *h_K, float gate_sq, int max_iterations,
                                  float *d_R, float *d_t, float *d_c2, float *d_points4d, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_ALIGNED(ctx, d_xy1, 8);
    VS_ALIGNED(ctx, d_xy2, 8);
    VS_ALIGNED(ctx, d_matches, 8);
    VS_ALIGNED(ctx, d_points4d, 16);
    VS_ALIGNED(ctx, d_stats, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_best, d_R, d_t, d_c2) % 4 == 0, VSLAM_ERR_INVALID);
    return vs_launch_refine_pairs(ctx, d_xy1, d_xy2, d_matches, d_best, batch, kp_stride, h_K, gate_sq, max_iterations, d_R, d_t, d_c2,
                                  d_points4d, d_stats);
}
