// Tracking against the map (include/vslam_resect.h): a pose-only adjustment from 3-D / 2-D correspondences, for a batch of
// independent items (vslam_resect_poses) and behind the world step (world.hip) for every track of a resecting world.  One
// workgroup of 256 lanes per item, one launch for all items, everything in f64 and never fused.  Both kernels run one body, the
// rounds of resect_math.h, and differ in where lane l finds its correspondences l, l + 256, ...: in the caller's arrays, or among
// the step's matches (the links whose current keypoint is finite, with the OLD carry as the 3-D half).  Nothing is kept per
// correspondence between two passes -- points and keypoints are read again, from L2 after the first pass -- so the LDS holds the
// reduction's scratch and nothing else.  Sums are block_reduce.h's, so an item's bits depend on the item alone.
#include <cmath>

#include "ctx.h"
#include "block_reduce.h"
#include "resect_math.h"
#include "world_match.h"
#include "world_select.h"

#pragma clang fp contract(off)

using namespace vs_resect;

namespace {
constexpr int kRT = 256;        // lanes per item
constexpr int kRW = kRT / 64;   // waves per item
constexpr int kRSums = 27;      // the widest sum: H (21) and g (6)

// the caller's arrays: correspondence i is (points[i], xy[i])
struct ArraySrc {
    const double *__restrict__ P;
    const float2 *__restrict__ xy;
    int n;
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        for (int i = threadIdx.x; i < n; i += kRT) {
            const double p[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
            const float2 o = xy[i];
            const double x[2] = {(double)o.x, (double)o.y};
            f(p, x);
        }
    }
};

// the step's matches: match k is a correspondence when it is a link of the step (usable under the pair's R, t, its `first` with
// a valid carry and a finite ratio) and the current frame's keypoint `second` is finite: (carry[first], xy_cur[second])
struct LinkSrc {
    const int2 *__restrict__ M;
    const float4 *__restrict__ P4;
    const double *__restrict__ carry;
    const int32_t *__restrict__ cidx;
    const float2 *__restrict__ xy;
    int n, nl, nc;
    double R[9], t[3];
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        for (int k = threadIdx.x; k < n; k += kRT) {
            const VsWorldMatch m = vs_world_load_match(M, P4, k, nl, nc, R, t);
            if (!m.usable || cidx[m.first] < 0) continue;
            const double c[3] = {carry[3 * (size_t)m.first], carry[3 * (size_t)m.first + 1], carry[3 * (size_t)m.first + 2]};
            if (ws_link_key(c, m.X) == kWsNoKey) continue;
            const float2 o = xy[m.second];
            if (!(isfinite(o.x) && isfinite(o.y))) continue;
            const double x[2] = {(double)o.x, (double)o.y};
            f(c, x);
        }
    }
};

__global__ __launch_bounds__(kRT) void resect_poses_kernel(const double *__restrict__ points, const float *__restrict__ xy,
                                                           const int32_t *__restrict__ n_in, int stride, VsK Kc, RsParams prm, double *R_io,
                                                           double *T_io, double *__restrict__ stats_out) {
    __shared__ double red[kRW * kRSums];
    const int b = blockIdx.x;
    double K[9];
    LmCam in, out;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        K[k] = (double)Kc.v[k];
        in.R[k] = R_io[(size_t)b * 9 + k];   // read by every lane before the first barrier, written behind the last one
    }
#pragma unroll
    for (int k = 0; k < 3; k++) in.T[k] = T_io[(size_t)b * 3 + k];
    ArraySrc src;
    src.P = points + (size_t)b * stride * 3;
    src.xy = reinterpret_cast<const float2 *>(xy) + (size_t)b * stride;
    src.n = min(max(n_in[b], 0), stride);
    VsBlockReduce rd{red};
    double stats[4];
    const bool moved = rs_run(K, in, prm, src, rd, out, stats);
    if (threadIdx.x != 0) return;
    if (moved) {
#pragma unroll
        for (int k = 0; k < 9; k++) R_io[(size_t)b * 9 + k] = out.R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) T_io[(size_t)b * 3 + k] = out.T[k];
    }
    if (stats_out) {
#pragma unroll
        for (int k = 0; k < 4; k++) stats_out[(size_t)b * 4 + k] = stats[k];
    }
}

struct ResectWorld {
    int max_frames, kp_stride;
    double *Twc;
    float *pose;
    double *scale;
    const double *carry_old;
    const int32_t *cidx_old;
    double *carry_new;
    const int32_t *cidx_new;
    double *stats;
};

// behind world_step_kernel for frame fid: that kernel has written Twc, pose, scale (s0), links and the new carry of the plain step
__global__ __launch_bounds__(kRT) void world_resect_kernel(ResectWorld w, int fid, const int32_t *__restrict__ matches,
                                                           const int32_t *__restrict__ best, const float *__restrict__ points4d,
                                                           const float *__restrict__ Rf, const float *__restrict__ tf,
                                                           const int32_t *__restrict__ n_last, const int32_t *__restrict__ n_cur,
                                                           const float *__restrict__ xy_cur, VsK Kc, RsParams prm) {
    __shared__ double red[kRW * kRSums];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K_ = w.kp_stride;
    const size_t fr = (size_t)b * w.max_frames + fid;
    double *st = w.stats + fr * 4;
    const double qnan = __builtin_nan("");
    if (best[(size_t)b * 4] < 0) {   // no winner: the plain step's
        if (tid == 0) {
            st[0] = 0.0;
            st[1] = st[2] = st[3] = qnan;
        }
        return;
    }
    LinkSrc src;
    src.n = min(max(best[(size_t)b * 4 + 3], 0), K_);
    src.nl = min(n_last[b], K_);
    src.nc = min(n_cur[b], K_);
    src.M = reinterpret_cast<const int2 *>(matches) + (size_t)b * K_;
    src.P4 = reinterpret_cast<const float4 *>(points4d) + (size_t)b * K_;
    src.carry = w.carry_old + (size_t)b * K_ * 3;
    src.cidx = w.cidx_old + (size_t)b * K_;
    src.xy = reinterpret_cast<const float2 *>(xy_cur) + (size_t)b * K_;
    const double s0 = w.scale[fr];   // read by every lane before the first barrier, written behind the last one
    double K[9];
    LmCam in, out;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        K[i] = (double)Kc.v[i];
        src.R[i] = (double)Rf[(size_t)b * 9 + i];
        in.R[i] = src.R[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        src.t[i] = (double)tf[(size_t)b * 3 + i];
        in.T[i] = s0 * src.t[i];
    }
    VsBlockReduce rd{red};
    double stats[4];
    const bool moved = rs_run(K, in, prm, src, rd, out, stats);   // the same in every lane
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) st[k] = stats[k];
    }
    if (!moved) return;   // left alone: the plain step's

    // Twc_f = Twc_(f-1) * [R'^t | -(R'^t T')]: one entry per lane
    const double *Tp = w.Twc + (fr - 1) * 16;
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        double B[4];   // column c of [R'^t | -(R'^t T')]; selected, not indexed, so that R' stays in registers
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double last = -((out.R[i] * out.T[0] + out.R[3 + i] * out.T[1]) + out.R[6 + i] * out.T[2]);
            B[i] = c == 0 ? out.R[i] : c == 1 ? out.R[3 + i] : c == 2 ? out.R[6 + i] : last;
        }
        B[3] = c == 3 ? 1.0 : 0.0;
        const double v = ((Tp[4 * r] * B[0] + Tp[4 * r + 1] * B[1]) + Tp[4 * r + 2] * B[2]) + Tp[4 * r + 3] * B[3];
        w.Twc[fr * 16 + tid] = v;
        w.pose[fr * 16 + tid] = (float)v;
    }
    const double s = sqrt((out.T[0] * out.T[0] + out.T[1] * out.T[1]) + out.T[2] * out.T[2]);
    if (tid == 0) w.scale[fr] = s;
    // the new carry's values: the plain step chose the winners (under the pair's own R, t); their values are R' (s X) + T'
    double *cn = w.carry_new + (size_t)b * K_ * 3;
    const int32_t *in_ = w.cidx_new + (size_t)b * K_;
    for (int k = tid; k < src.n; k += kRT) {
        const VsWorldMatch m = vs_world_load_match(src.M, src.P4, k, src.nl, src.nc, src.R, src.t);
        if (!(m.usable && in_[m.second] == k)) continue;
        const double x = s * m.X[0], y = s * m.X[1], z = s * m.X[2];
#pragma unroll
        for (int r = 0; r < 3; r++)
            cn[3 * (size_t)m.second + r] = ((out.R[3 * r] * x + out.R[3 * r + 1] * y) + out.R[3 * r + 2] * z) + out.T[r];
    }
}

// frame 0 of every track and every slot no step has written: 0, NaN, NaN, NaN
__global__ __launch_bounds__(kRT) void world_resect_reset_kernel(double *stats, size_t count) {
    const size_t i = (size_t)blockIdx.x * kRT + threadIdx.x;
    if (i < count) stats[i] = (i & 3) == 0 ? 0.0 : __builtin_nan("");
}

RsParams pack(const vslam_resect_params &p) {
    RsParams q;
    q.max_iterations = p.max_iterations; q.rounds = p.rounds; q.min_links = p.min_links;
    q.huber = p.huber_px; q.gate = p.gate_px;
    return q;
}
}  // namespace

bool vs_resect_params_ok(const vslam_resect_params &p) {
    return p.max_iterations >= 1 && p.max_iterations <= 64 && p.rounds >= 1 && p.rounds <= 4 && p.min_links >= 6 &&
           p.huber_px > 0.0 && std::isfinite(p.huber_px) && p.gate_px > 0.0 && std::isfinite(p.gate_px);
}

int vs_world_resect_reset(vslam_ctx *ctx, vslam_world *w) {
    const size_t count = (size_t)w->tracks * w->max_frames * 4;
    // the second carry table as world_reset_kernel leaves the first: values 0, every entry invalid, so that after any number of
    // steps both tables are a function of the steps alone
    const size_t slots = (size_t)w->tracks * w->kp_stride;
    VS_HIP(ctx, hipMemsetAsync(w->carry_next, 0, sizeof(double) * 3 * slots, ctx->stream));
    VS_HIP(ctx, hipMemsetAsync(w->carry_idx_next, 0xFF, sizeof(int32_t) * slots, ctx->stream));
    world_resect_reset_kernel<<<(unsigned)((count + kRT - 1) / kRT), kRT, 0, ctx->stream>>>(w->resect_stats, count);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vs_launch_world_resect(vslam_ctx *ctx, vslam_world *w, int fid, const int32_t *matches, const int32_t *best, const float *points4d,
                           const float *R, const float *t, const int32_t *n_last, const int32_t *n_cur, const float *xy_cur,
                           const float *h_K) {
    VS_REQUIRE(ctx, xy_cur && h_K, VSLAM_ERR_INVALID);
    const VsK K = vs_pack_K(h_K);
    ResectWorld d;
    d.max_frames = w->max_frames; d.kp_stride = w->kp_stride;
    d.Twc = w->Twc; d.pose = w->pose; d.scale = w->scale;
    d.carry_old = w->carry; d.cidx_old = w->carry_idx; d.carry_new = w->carry_next; d.cidx_new = w->carry_idx_next;
    d.stats = w->resect_stats;
    VsProfScope ps(ctx, "world_resect_kernel");
    world_resect_kernel<<<w->tracks, kRT, 0, ctx->stream>>>(d, fid, matches, best, points4d, R, t, n_last, n_cur, xy_cur, K,
                                                           pack(w->resect_params));
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

extern "C" {

int vslam_resect_params_default(vslam_resect_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->max_iterations = 20; out->rounds = 3; out->min_links = 8;
    out->huber_px = 2.0; out->gate_px = 6.0;
    return VSLAM_OK;
}

int vslam_resect_poses(vslam_ctx *ctx, const double *d_points, const float *d_xy, const int32_t *d_n, int batch, int stride,
                       const float *h_K, const vslam_resect_params *params, double *d_R, double *d_T, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_points && d_xy && d_n && h_K && d_R && d_T, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    VS_ALIGNED(ctx, d_xy, 8);   // float2 rows
    VS_REQUIRE(ctx, vs_ptr_bits(d_points, d_R, d_T, d_stats) % 8 == 0, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_n, 4);
    vslam_resect_params p;
    vslam_resect_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, vs_resect_params_ok(p), VSLAM_ERR_INVALID);
    const VsK K = vs_pack_K(h_K);
    VsProfScope ps(ctx, "resect_poses_kernel");
    resect_poses_kernel<<<batch, kRT, 0, ctx->stream>>>(d_points, d_xy, d_n, stride, K, pack(p), d_R, d_T, d_stats);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

}  // extern "C"
