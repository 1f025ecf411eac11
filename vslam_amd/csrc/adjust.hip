// The window adjustment (include/vslam_adjust.h): cameras and the points they share moved together, for a batch of independent
// items.  One workgroup of 256 lanes per item, one launch for all items, everything in f64 and never fused.  The kernel runs the
// rounds of adjust_math.h: lane l owns points l, l + 256, ... (their observations' blocks, the damped 3 x 3 solve, the point's
// step), then the entries of the reduced system are dealt out over the lanes and each is summed over the points in ascending
// order from what the points left in the arena -- a second pass by camera pair, no atomics --, the reduced system (at most
// 42 x 42) is factored in the LDS with row i on lane i, and sums over the observations are block_reduce.h's.  An item's bits
// depend on the item alone.
#include <cmath>

#include "ctx.h"
#include "../../include/vslam_adjust.h"
#include "block_reduce.h"
#include "adjust_math.h"

#pragma clang fp contract(off)

using namespace vs_adjust;

namespace {
constexpr int kAT = 256;        // lanes per item
constexpr int kAW = kAT / 64;   // waves per item
constexpr int kASums = kAdMaxCams + 1;   // the widest sum: the counts per camera and their total

struct BlockEx : VsBlockReduce {   // lds: [kAW][kASums]
    template <class F>
    __device__ __forceinline__ void points(int n, F f) const {
        for (int i = threadIdx.x; i < n; i += kAT) f(i);
    }
    template <class F>
    __device__ __forceinline__ void entries(int n, F f) const {
        for (int e = threadIdx.x; e < n; e += kAT) f(e);
    }
    template <class F>
    __device__ __forceinline__ void rows(int n, F f) const {
        if ((int)threadIdx.x < n) f((int)threadIdx.x);
    }
    template <class F>
    __device__ __forceinline__ void one(F f) const {
        if (threadIdx.x == 0) f();
    }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

struct AdArgs {
    double *R, *T, *X;
    const int32_t *n_cams, *n_points, *off, *cam;
    const float *xy;
    int cam_stride, pt_stride, obs_stride;
    double *f64;      // [batch][pt_stride][kPerPoint]
    int32_t *mask;    // [batch][pt_stride]
    uint8_t *flags;   // [batch][2][obs_stride]
    double *stats;
    int32_t *out_free;   // [batch] or null: bit c = camera c was written
    uint8_t *out_took;   // [batch][pt_stride] or null: the point was written
};
constexpr int kPerPoint = 9 + kAdMaxSlots * kAdStage;   // Xa, Xb, z, the staged blocks

__global__ __launch_bounds__(kAT) void adjust_windows_kernel(AdArgs a, VsK Kc, AdParams prm) {
    __shared__ AdShared sh;
    __shared__ double red[kAW * kASums];
    const int b = blockIdx.x;
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = (double)Kc.v[k];
    AdItem it;
    it.C = a.n_cams[b];
    it.N = a.n_points[b];
    it.cam_stride = a.cam_stride; it.pt_stride = a.pt_stride; it.obs_stride = a.obs_stride;
    double *R = a.R + (size_t)b * a.cam_stride * 9, *T = a.T + (size_t)b * a.cam_stride * 3, *X = a.X + (size_t)b * a.pt_stride * 3;
    it.R = R; it.T = T; it.X = X;
    it.off = a.off + (size_t)b * (a.pt_stride + 1);
    it.cam = a.cam + (size_t)b * a.obs_stride;
    it.xy = a.xy + (size_t)b * a.obs_stride * 2;
    AdWork w;
    double *base = a.f64 + (size_t)b * a.pt_stride * kPerPoint;
    w.Xa = base;
    w.Xb = base + (size_t)a.pt_stride * 3;
    w.z = base + (size_t)a.pt_stride * 6;
    w.stage = base + (size_t)a.pt_stride * 9;
    w.mask = a.mask + (size_t)b * a.pt_stride;
    w.fa = a.flags + (size_t)b * 2 * a.obs_stride;
    w.fb = w.fa + a.obs_stride;
    BlockEx ex;
    ex.lds = red;
    AdResult res;
    double stats[4];
    const bool moved = ad_run(K, it, prm, w, sh, ex, res, stats);   // the same in every lane
    if (a.stats && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) a.stats[(size_t)b * 4 + k] = stats[k];
    }
    if (a.out_free && threadIdx.x == 0) a.out_free[b] = moved ? res.ever_free : 0;
    if (a.out_took) {
        const int n = min(max(it.N, 0), a.pt_stride);
        for (int i = threadIdx.x; i < n; i += kAT) a.out_took[(size_t)b * a.pt_stride + i] = moved && ad_took_part(it.off, res.flags, i) ? 1 : 0;
    }
    if (!moved) return;
    __syncthreads();   // the inputs have been read by everyone (the statistics under the start)
    if ((int)threadIdx.x < it.C && ((res.ever_free >> threadIdx.x) & 1)) {
        const int c = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 9; k++) R[9 * c + k] = sh.cur[c].R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) T[3 * c + k] = sh.cur[c].T[k];
    }
    for (int i = threadIdx.x; i < it.N; i += kAT) {
        if (!ad_took_part(it.off, res.flags, i)) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) X[3 * (size_t)i + k] = res.X[3 * (size_t)i + k];
    }
}

bool params_ok(const vslam_adjust_params &p) {
    return p.max_iterations >= 1 && p.max_iterations <= 64 && p.rounds >= 1 && p.rounds <= 4 && p.min_obs >= 6 && p.n_fixed >= 1 &&
           p.huber_px > 0.0 && std::isfinite(p.huber_px) && p.gate_px > 0.0 && std::isfinite(p.gate_px);
}

int launch_adjust(vslam_ctx *ctx, AdArgs a, int batch, const float *h_K, const vslam_adjust_params &p) {
    void *ptr = nullptr;
    int rc = vs_arena_get(ctx, "adjust_f64", sizeof(double) * (size_t)batch * a.pt_stride * kPerPoint, &ptr);
    if (rc != VSLAM_OK) return rc;
    a.f64 = static_cast<double *>(ptr);
    rc = vs_arena_get(ctx, "adjust_mask", sizeof(int32_t) * (size_t)batch * a.pt_stride, &ptr);
    if (rc != VSLAM_OK) return rc;
    a.mask = static_cast<int32_t *>(ptr);
    rc = vs_arena_get(ctx, "adjust_flags", (size_t)batch * 2 * a.obs_stride, &ptr);
    if (rc != VSLAM_OK) return rc;
    a.flags = static_cast<uint8_t *>(ptr);
    const VsK K = vs_pack_K(h_K);
    AdParams q;
    q.max_iterations = p.max_iterations; q.rounds = p.rounds; q.min_obs = p.min_obs; q.n_fixed = p.n_fixed;
    q.huber = p.huber_px; q.gate = p.gate_px;
    VsProfScope ps(ctx, "adjust_windows_kernel");
    adjust_windows_kernel<<<batch, kAT, 0, ctx->stream>>>(a, K, q);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

// ---- on the world (vslam_world_adjust): the window's problem gathered from the world and the map's log, and written back
struct WorldAdjust {
    int32_t *log_off, *log_frame, *log_kp;   // the map's CSR as vslam_map_observations writes it
    int32_t *off, *cam, *n_cams, *n_points, *free_mask;
    double *R, *T, *X, *stats;
    float *xy;
    uint8_t *took;
    int max_frames, kp_stride, P, O, xy_frames, f0, f1;
    const int32_t *sizes;
    double *Twc;
    float *pose, *world_points;
    double *carry;
    const int32_t *carry_idx;
    const float *d_xy;
};

// one workgroup per track: cameras f0 .. f1 from d_Twc, the track's map points widened, and of each point's observations those
// whose frame lies in the window and whose keypoint index is in range, in the log's push order
__global__ __launch_bounds__(kAT) void world_adjust_gather_kernel(WorldAdjust g) {
    __shared__ int scan[kAT];
    __shared__ int carry_over;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = g.f1 - g.f0 + 1;
    const int N = min(max(g.sizes[b], 0), g.P);
    if (tid == 0) {
        g.n_cams[b] = C;
        g.n_points[b] = N;
        carry_over = 0;
    }
    if (tid < C) {
        const double *M = g.Twc + ((size_t)b * g.max_frames + g.f0 + tid) * 16;
        double *R = g.R + ((size_t)b * 8 + tid) * 9, *T = g.T + ((size_t)b * 8 + tid) * 3;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) R[3 * r + c] = M[4 * c + r];
            T[r] = -((M[r] * M[3] + M[4 + r] * M[7]) + M[8 + r] * M[11]);
        }
    }
    const int32_t *lo = g.log_off + (size_t)b * (g.P + 1), *lf = g.log_frame + (size_t)b * g.O, *lk = g.log_kp + (size_t)b * g.O;
    int32_t *off = g.off + (size_t)b * (g.P + 1);
    auto in_window = [&](int o) { return lf[o] >= g.f0 && lf[o] <= g.f1 && lk[o] >= 0 && lk[o] < g.kp_stride; };
    for (int base = 0; base < N; base += kAT) {   // exclusive prefix of the points' counts, 256 points at a time
        const int i = base + tid;
        int cnt = 0;
        if (i < N) {
#pragma unroll
            for (int k = 0; k < 3; k++) g.X[((size_t)b * g.P + i) * 3 + k] = (double)g.world_points[((size_t)b * g.P + i) * 4 + k];
            const int e = min(max(lo[i + 1], 0), g.O);
            for (int o = min(max(lo[i], 0), g.O); o < e; o++) cnt += in_window(o) ? 1 : 0;
        }
        __syncthreads();   // carry_over and scan[] of the chunk before have been read
        scan[tid] = cnt;
        __syncthreads();
        for (int d = 1; d < kAT; d <<= 1) {
            const int v = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int start = carry_over + scan[tid] - cnt;
        if (i < N) {
            off[i] = start;
            int pos = start;
            const int e = min(max(lo[i + 1], 0), g.O);
            for (int o = min(max(lo[i], 0), g.O); o < e; o++) {
                if (!in_window(o)) continue;
                g.cam[(size_t)b * g.O + pos] = lf[o] - g.f0;
                const float *src = g.d_xy + (((size_t)b * g.xy_frames + lf[o]) * g.kp_stride + lk[o]) * 2;
                g.xy[((size_t)b * g.O + pos) * 2] = src[0];
                g.xy[((size_t)b * g.O + pos) * 2 + 1] = src[1];
                pos++;
            }
        }
        __syncthreads();
        if (tid == kAT - 1) carry_over += scan[tid];
    }
    __syncthreads();
    if (tid == 0) off[N] = carry_over;
}

// one workgroup per track, behind the adjustment: where the item moved, d_Twc / d_pose of the cameras written, d_world_points of
// the points written, and the latest carry re-expressed in the last camera when that camera moved
__global__ __launch_bounds__(kAT) void world_adjust_scatter_kernel(WorldAdjust g, double *__restrict__ stats_out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (stats_out && tid < 4) stats_out[(size_t)b * 4 + tid] = g.stats[(size_t)b * 4 + tid];
    const int free_mask = g.free_mask[b];
    if (free_mask == 0) return;
    const int C = g.f1 - g.f0 + 1, N = g.n_points[b];
    double old[12];   // the last camera's pose before it is written: read by every lane, written behind the barrier
#pragma unroll
    for (int k = 0; k < 12; k++) old[k] = g.Twc[((size_t)b * g.max_frames + g.f1) * 16 + k];
    __syncthreads();
    if (tid < C && ((free_mask >> tid) & 1)) {
        const double *R = g.R + ((size_t)b * 8 + tid) * 9, *T = g.T + ((size_t)b * 8 + tid) * 3;
        double *M = g.Twc + ((size_t)b * g.max_frames + g.f0 + tid) * 16;
        float *Mf = g.pose + ((size_t)b * g.max_frames + g.f0 + tid) * 16;
        double v[16];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) v[4 * r + c] = R[3 * c + r];
            v[4 * r + 3] = -((R[r] * T[0] + R[3 + r] * T[1]) + R[6 + r] * T[2]);
        }
        v[12] = v[13] = v[14] = 0.0;
        v[15] = 1.0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            M[k] = v[k];
            Mf[k] = (float)v[k];
        }
    }
    for (int i = tid; i < N; i += kAT) {
        if (!g.took[(size_t)b * g.P + i]) continue;
        float *w = g.world_points + ((size_t)b * g.P + i) * 4;
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = (float)g.X[((size_t)b * g.P + i) * 3 + k];
        w[3] = 1.0f;
    }
    if (!((free_mask >> (C - 1)) & 1)) return;
    const double *R = g.R + ((size_t)b * 8 + C - 1) * 9, *T = g.T + ((size_t)b * 8 + C - 1) * 3;
    for (int k = tid; k < g.kp_stride; k += kAT) {
        if (g.carry_idx[(size_t)b * g.kp_stride + k] < 0) continue;
        double *c = g.carry + ((size_t)b * g.kp_stride + k) * 3;
        double wv[3], out[3];
#pragma unroll
        for (int r = 0; r < 3; r++) wv[r] = ((old[4 * r] * c[0] + old[4 * r + 1] * c[1]) + old[4 * r + 2] * c[2]) + old[4 * r + 3];
#pragma unroll
        for (int r = 0; r < 3; r++) out[r] = ((R[3 * r] * wv[0] + R[3 * r + 1] * wv[1]) + R[3 * r + 2] * wv[2]) + T[r];
#pragma unroll
        for (int r = 0; r < 3; r++) c[r] = out[r];
    }
}
}  // namespace

extern "C" {

int vslam_adjust_params_default(vslam_adjust_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->max_iterations = 20; out->rounds = 3; out->min_obs = 8; out->n_fixed = 2;
    out->huber_px = 2.0; out->gate_px = 6.0;
    return VSLAM_OK;
}

int vslam_adjust_windows(vslam_ctx *ctx, double *d_R, double *d_T, const int32_t *d_n_cams, int cam_stride, double *d_points,
                         const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets, const int32_t *d_obs_cam,
                         const float *d_obs_xy, int obs_stride, int batch, const float *h_K, const vslam_adjust_params *params,
                         double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_R && d_T && d_n_cams && d_points && d_n_points && d_obs_offsets && d_obs_cam && d_obs_xy && h_K, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && cam_stride > 0 && pt_stride > 0 && obs_stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, cam_stride <= VSLAM_ADJUST_MAX_CAMS, VSLAM_ERR_CAPACITY);
    VS_ALIGNED(ctx, d_R, 8);
    VS_ALIGNED(ctx, d_T, 8);
    VS_ALIGNED(ctx, d_points, 8);
    VS_ALIGNED(ctx, d_stats, 8);
    VS_ALIGNED(ctx, d_obs_xy, 8);   // float2 rows
    VS_ALIGNED(ctx, d_n_cams, 4);
    VS_ALIGNED(ctx, d_n_points, 4);
    VS_ALIGNED(ctx, d_obs_offsets, 4);
    VS_ALIGNED(ctx, d_obs_cam, 4);
    vslam_adjust_params p;
    vslam_adjust_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    AdArgs a;
    a.R = d_R; a.T = d_T; a.X = d_points;
    a.n_cams = d_n_cams; a.n_points = d_n_points; a.off = d_obs_offsets; a.cam = d_obs_cam; a.xy = d_obs_xy;
    a.cam_stride = cam_stride; a.pt_stride = pt_stride; a.obs_stride = obs_stride;
    a.stats = d_stats;
    a.out_free = nullptr; a.out_took = nullptr;
    return launch_adjust(ctx, a, batch, h_K, p);
}

int vslam_world_adjust(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy, int xy_frames, const float *h_K,
                       int window, const vslam_adjust_params *params, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy && h_K, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc = vs_world_map_view(ctx, world, map, &m);
    if (rc != VSLAM_OK) return rc;
    VS_REQUIRE(ctx, window >= 2 && window <= VSLAM_ADJUST_MAX_CAMS && xy_frames >= m.frames, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xy, 8);
    VS_ALIGNED(ctx, d_stats, 8);
    vslam_adjust_params p;
    vslam_adjust_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    const int T = m.tracks, P = m.map_capacity, O = m.obs_capacity;
    // workspace: the map's CSR, the gathered problem, what the kernel wrote
    const size_t i32s = (size_t)T * (2 * (size_t)(P + 1) + 3 * (size_t)O + 3), f64s = (size_t)T * (8 * 12 + 3 * (size_t)P + 4);
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_adjust_i32", sizeof(int32_t) * i32s, &ptr))) return rc;
    int32_t *ip = static_cast<int32_t *>(ptr);
    if ((rc = vs_arena_get(ctx, "world_adjust_f64", sizeof(double) * f64s, &ptr))) return rc;
    double *dp = static_cast<double *>(ptr);
    if ((rc = vs_arena_get(ctx, "world_adjust_xy", sizeof(float) * 2 * (size_t)T * O, &ptr))) return rc;
    float *xy = static_cast<float *>(ptr);
    if ((rc = vs_arena_get(ctx, "world_adjust_took", (size_t)T * P, &ptr))) return rc;
    uint8_t *took = static_cast<uint8_t *>(ptr);
    WorldAdjust g;
    g.log_off = ip; g.log_frame = g.log_off + (size_t)T * (P + 1); g.log_kp = g.log_frame + (size_t)T * O;
    g.off = g.log_kp + (size_t)T * O; g.cam = g.off + (size_t)T * (P + 1);
    g.n_cams = g.cam + (size_t)T * O; g.n_points = g.n_cams + T; g.free_mask = g.n_points + T;
    g.R = dp; g.T = g.R + (size_t)T * 8 * 9; g.X = g.T + (size_t)T * 8 * 3; g.stats = g.X + (size_t)T * P * 3;
    g.xy = xy; g.took = took;
    g.max_frames = m.max_frames; g.kp_stride = m.kp_stride; g.P = P; g.O = O; g.xy_frames = xy_frames;
    g.f1 = m.frames - 1;
    g.f0 = g.f1 - window + 1 > 0 ? g.f1 - window + 1 : 0;
    g.sizes = static_cast<const int32_t *>(m.d_sizes);
    g.Twc = world->Twc; g.pose = world->pose; g.world_points = world->world_points; g.carry = world->carry; g.carry_idx = world->carry_idx;
    g.d_xy = d_xy;
    if ((rc = vs_world_csr(ctx, world, map, g.log_off, g.log_frame, g.log_kp, nullptr))) return rc;
    world_adjust_gather_kernel<<<T, kAT, 0, ctx->stream>>>(g);
    VS_HIP(ctx, hipGetLastError());
    AdArgs a;
    a.R = g.R; a.T = g.T; a.X = g.X;
    a.n_cams = g.n_cams; a.n_points = g.n_points; a.off = g.off; a.cam = g.cam; a.xy = g.xy;
    a.cam_stride = VSLAM_ADJUST_MAX_CAMS; a.pt_stride = P; a.obs_stride = O;
    a.stats = g.stats;
    a.out_free = g.free_mask; a.out_took = g.took;
    if ((rc = launch_adjust(ctx, a, T, h_K, p))) return rc;
    world_adjust_scatter_kernel<<<T, kAT, 0, ctx->stream>>>(g, d_stats);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

}  // extern "C"
