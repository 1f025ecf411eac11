// Two-view bundle adjustment of each pair's pose and points (vslam_refine_pairs, include/vslam_amd.h): the step the reference
// left as an empty `struct optimizer` (src/optimzer.cpp).  One workgroup of 256 lanes per pair, everything in f64 and never fused;
// lane l owns the points i = l (mod 256).  The kernel runs ba_run of refine_math.h, which decides everything; what is here is
// about the device: the loads in front of the first barrier, where a point's state lives, and the writes behind the last barrier.
// A point's accepted and candidate coordinates stay in f64 from the first iteration to the last: in LDS when the pair's n fits
// the launch's dynamic LDS, in an arena workspace otherwise -- the arithmetic is the same, only the address differs.  Sums are
// block_reduce.h's, so a pair's bits depend on the pair alone.
#include "ctx.h"
#include "block_reduce.h"
#include "refine_math.h"

#pragma clang fp contract(off)

using namespace vs_refine;

namespace {
constexpr int kBT = 256;        // lanes per pair
constexpr int kBW = kBT / 64;   // waves per pair
constexpr int kStateBytes = 6 * 8 + 1;                   // per point: accepted and candidate (x, y, z) f64, one flag byte
constexpr int kLdsPoints = 3200;                         // most points whose state fits beside the 896 B of static LDS

// ba_run's policy: lane l walks correspondences l, l + 256, ...; correspondence i is match i's two keypoints and points4d[i]
struct PairEx : VsBlockReduce {
    const float *__restrict__ p1, *__restrict__ p2;
    const int32_t *__restrict__ mt;
    const float *P;
    int kp_stride, cap;
    double *st;    // [2][3][cap] (accepted / candidate)
    uint8_t *fl;   // [cap]
    template <class F>
    __device__ __forceinline__ void each(int n, F f) const {
        for (int i = threadIdx.x; i < n; i += kBT) f(i);
    }
    // false for an index outside the keypoint slots
    __device__ __forceinline__ bool observed(int i, double (&o)[4]) const {
        const int a = mt[2 * i], c = mt[2 * i + 1];
        if (a < 0 || a >= kp_stride || c < 0 || c >= kp_stride) return false;
        const float x1 = p1[2 * a], y1 = p1[2 * a + 1], x2 = p2[2 * c], y2 = p2[2 * c + 1];
        // both loads are in flight before either is used: at this register pressure the scheduler otherwise converts the first
        // keypoint before it asks for the second, one more round trip to memory per correspondence and pass
        __builtin_amdgcn_sched_barrier(0);
        o[0] = (double)x1; o[1] = (double)y1;
        o[2] = (double)x2; o[3] = (double)y2;
        return true;
    }
    __device__ __forceinline__ void input(int i, double (&X)[3]) const {
#pragma unroll
        for (int k = 0; k < 3; k++) X[k] = (double)P[4 * i + k];
    }
    __device__ __forceinline__ double &state(int buf, int k, int i) const { return st[((size_t)buf * 3 + k) * cap + i]; }
    __device__ __forceinline__ uint8_t &flag(int i) const { return fl[i]; }
};

__global__ __launch_bounds__(kBT) void refine_pairs_kernel(const float *__restrict__ xy1, const float *__restrict__ xy2,
                                                           const int32_t *__restrict__ matches, const int32_t *__restrict__ best,
                                                           int kp_stride, VsK Kc, double gate_sq, int max_iterations, float *R_io,
                                                           float *t_io, float *__restrict__ c2_out, float *points4d,
                                                           double *__restrict__ stats, int lds_points, double *arena_state,
                                                           uint8_t *arena_flags) {
    extern __shared__ __align__(16) unsigned char ba_dyn[];
    __shared__ double red[kBW * 20];
    const int b = blockIdx.x, tid = threadIdx.x;
    float *P = points4d + (size_t)b * kp_stride * 4;
    const int winner = best[b * 4 + 0];
    int n = best[b * 4 + 3];
    n = n < 0 ? 0 : (n > kp_stride ? kp_stride : n);
    // R and t are read by every lane before the first barrier and written behind the last one
    float Rin32[9], tin32[3];
    double K[9];
    LmCam in;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        Rin32[k] = R_io[(size_t)b * 9 + k];
        in.R[k] = (double)Rin32[k];
        K[k] = (double)Kc.v[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tin32[k] = t_io[(size_t)b * 3 + k];
        in.T[k] = (double)tin32[k];
    }
    PairEx ex;
    ex.lds = red;
    ex.p1 = xy1 + (size_t)b * kp_stride * 2;
    ex.p2 = xy2 + (size_t)b * kp_stride * 2;
    ex.mt = matches + (size_t)b * kp_stride * 2;
    ex.P = P;
    ex.kp_stride = kp_stride;
    // the point state in LDS when n fits and in the arena otherwise, chosen once per pair: ba_run is inlined behind each choice, so
    // its state accesses are LDS instructions in one copy and global ones in the other, not flat ones behind a selected pointer
    BaResult res;
    double st4[4];
    bool moved;   // the same in every lane
    if (n <= lds_points) {
        ex.cap = lds_points;
        ex.st = reinterpret_cast<double *>(ba_dyn);
        ex.fl = ba_dyn + (size_t)48 * lds_points;
        moved = ba_run(K, in, winner, n, gate_sq, max_iterations, ex, res, st4);
    } else {
        ex.cap = kp_stride;
        ex.st = arena_state + (size_t)b * 6 * kp_stride;
        ex.fl = arena_flags + (size_t)b * kp_stride;
        moved = ba_run(K, in, winner, n, gate_sq, max_iterations, ex, res, st4);
    }
    if (moved) {
        for (int i = tid; i < n; i += kBT) {
            if (!ex.fl[i]) continue;
            reinterpret_cast<float4 *>(P)[i] =
                make_float4((float)ex.state(res.buf, 0, i), (float)ex.state(res.buf, 1, i), (float)ex.state(res.buf, 2, i), 1.f);
        }
    }
    if (tid != 0) return;
    if (!moved) {   // left alone: the inputs' bits, and the camera they make
        ba_camera(K, in, res.c2);
#pragma unroll
        for (int k = 0; k < 9; k++) res.R32[k] = Rin32[k];
#pragma unroll
        for (int k = 0; k < 3; k++) res.t32[k] = tin32[k];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) R_io[(size_t)b * 9 + k] = res.R32[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t_io[(size_t)b * 3 + k] = res.t32[k];
#pragma unroll
    for (int k = 0; k < 12; k++) c2_out[(size_t)b * 12 + k] = res.c2[k];
    if (stats) {
#pragma unroll
        for (int k = 0; k < 4; k++) stats[(size_t)b * 4 + k] = st4[k];
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
    const VsK K = vs_pack_K(h_K);
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
