// Each track triangulated from all its observations (include/vslam_tracks.h), for a batch of independent items.
//   triangulate_tracks_kernel   grid (ceil(pt_stride / 256), batch): one lane per point (tracks_math.h's tr_point): sums have to run
//                               in observation order and rows are short, so a row is one lane's.  A lane walks its row once per
//                               pass -- two for the parallax test and the linear start, one per Levenberg-Marquardt iteration, one
//                               for the verdict -- and forms cameras, rays and centres afresh each time: nothing per observation
//                               is kept, the state is X, two sets of 3 x 3 blocks and the damping, all in registers.  Rows of
//                               different lengths and runs that stop early diverge inside a wave; nothing is staged in LDS but the
//                               four counts, which reach d_stats by integer atomics behind a fill.
//   vslam_world_retriangulate   the world's CSR (vs_world_csr), its cameras (vs_world_cameras, fuse.hip) and the kernel above on
//                               d_world_points in place.
// No floating-point atomics and no scratch.
#include <cmath>

#include "ctx.h"
#include "../../include/vslam_adjust.h"
#include "../../include/vslam_tracks.h"
#include "tracks_math.h"

#pragma clang fp contract(off)

using namespace vs_tracks;

namespace {
constexpr int kTT = 256;   // lanes per workgroup
constexpr int kMaxCams = 1024;

struct TrackArgs {
    const float4 *points;
    const int32_t *n_points;
    int pt_stride;
    const int32_t *off, *cam, *kp;
    int obs_stride;
    const double *R, *T;
    const int32_t *n_cams;
    int cam_stride;
    const float *xy;
    size_t xy_item;   // floats from one item's keypoints to the next: >= cam_stride x kp_stride x 2
    int kp_stride;
    TrParams prm;
    double Ki[9];
    float4 *out_points;
    int32_t *status, *counts, *stats;   // status and counts may be null
    double *info;
};

__global__ __launch_bounds__(kTT) void triangulate_tracks_kernel(TrackArgs a, VsK Kc) {
    __shared__ int sums[4];
    const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * kTT + tid;
    if (tid < 4) sums[tid] = 0;
    __syncthreads();
    const int S = a.pt_stride;
    const int n = min(max(a.n_points[b], 0), S);
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = (double)Kc.v[k];
    TrResult res;
    res.status = kTrNoPart;
    res.m = res.n_good = 0;
    res.cos_parallax = res.cost_in = res.cost_out = tr_qnan();
    float4 P = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < S) P = a.points[(size_t)b * S + i];   // the row is read before it is written: d_out_points may be d_points
    if (i < n) {
        const int32_t *OFF = a.off + (size_t)b * (S + 1);
        TrItem it;
        it.cam = a.cam + (size_t)b * a.obs_stride;
        it.kp = a.kp + (size_t)b * a.obs_stride;
        it.R = a.R + (size_t)b * a.cam_stride * 9;
        it.T = a.T + (size_t)b * a.cam_stride * 3;
        it.xy = a.xy + (size_t)b * a.xy_item;
        it.C = min(max(a.n_cams[b], 0), a.cam_stride);
        it.kp_stride = a.kp_stride;
        tr_point(K, a.Ki, it, OFF[i], OFF[i + 1], a.obs_stride, P.x, P.y, P.z, a.prm, res);
    }
    if (i < S) {
        const size_t at = (size_t)b * S + i;
        if (res.status == kTrOk) P = make_float4((float)res.X[0], (float)res.X[1], (float)res.X[2], 1.0f);
        if (res.status == kTrOk || a.out_points != a.points) a.out_points[at] = P;
        if (a.status) a.status[at] = res.status;
        if (a.counts) {
            a.counts[at * 2] = res.m;
            a.counts[at * 2 + 1] = res.n_good;
        }
        if (a.info) {
            a.info[at * 3] = res.cos_parallax;
            a.info[at * 3 + 1] = res.cost_in;
            a.info[at * 3 + 2] = res.cost_out;
        }
    }
    if (res.status >= 0) {
        atomicAdd(&sums[0], 1);
        atomicAdd(&sums[res.status == kTrOk ? 1 : res.status == kTrLowParallax ? 2 : 3], 1);
    }
    __syncthreads();
    if (tid < 4 && sums[tid]) atomicAdd(&a.stats[(size_t)b * 4 + tid], sums[tid]);
}

bool K_finite(const float *h_K) {
    bool ok = true;
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(h_K[k]);
    return ok;
}

// params (or the defaults) checked and packed; Kinv from the widened h_K
int track_setup(vslam_ctx *ctx, const vslam_track_params *params, const float *h_K, TrackArgs &a) {
    vslam_track_params p;
    vslam_track_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, tr_params_ok(p.cos_parallax_max, p.huber_px, p.inlier_px, p.iterations, p.min_good, p.good10), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    double K[9];
    for (int k = 0; k < 9; k++) K[k] = (double)h_K[k];
    VS_REQUIRE(ctx, tr_kinv(K, a.Ki), VSLAM_ERR_INVALID);
    a.prm = tr_params(p.cos_parallax_max, p.huber_px, p.inlier_px, p.iterations, p.min_good, p.good10);
    return VSLAM_OK;
}

int launch_tracks(vslam_ctx *ctx, const TrackArgs &a, int batch, const float *h_K) {
    VS_HIP(ctx, hipMemsetAsync(a.stats, 0, sizeof(int32_t) * 4 * (size_t)batch, ctx->stream));
    {
        VsProfScope ps(ctx, "triangulate_tracks_kernel");
        triangulate_tracks_kernel<<<dim3(vs_div_up(a.pt_stride, kTT), batch), kTT, 0, ctx->stream>>>(a, vs_pack_K(h_K));
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}
}  // namespace

extern "C" {

int vslam_track_params_default(vslam_track_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    vslam_adjust_params ap;
    vslam_adjust_params_default(&ap);
    out->cos_parallax_max = 0.9998; out->huber_px = ap.huber_px; out->inlier_px = ap.gate_px; out->iterations = 10; out->min_good = 2; out->good10 = 5;
    return VSLAM_OK;
}

int vslam_triangulate_tracks(vslam_ctx *ctx, const float *d_points, const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets,
                             const int32_t *d_obs_cam, const int32_t *d_obs_kp, int obs_stride, const double *d_R, const double *d_T,
                             const int32_t *d_n_cams, int cam_stride, const float *d_xy, int kp_stride, const float *h_K, int batch,
                             const vslam_track_params *params, float *d_out_points, int32_t *d_status, int32_t *d_counts, double *d_info,
                             int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_points && d_n_points && d_obs_offsets && d_obs_cam && d_obs_kp && d_R && d_T && d_n_cams && d_xy && h_K && d_out_points &&
                        d_status && d_stats, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && pt_stride > 0 && obs_stride > 0 && cam_stride > 0 && kp_stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP && cam_stride <= kMaxCams, VSLAM_ERR_CAPACITY);
    TrackArgs a;
    int rc;
    if ((rc = track_setup(ctx, params, h_K, a))) return rc;
    VS_ALIGNED(ctx, d_points, 16);   // float4 rows
    VS_ALIGNED(ctx, d_out_points, 16);
    VS_ALIGNED(ctx, d_xy, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_R, d_T, d_info) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_points, d_obs_offsets, d_obs_cam, d_obs_kp, d_n_cams, d_status, d_counts, d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    a.points = reinterpret_cast<const float4 *>(d_points); a.n_points = d_n_points; a.pt_stride = pt_stride;
    a.off = d_obs_offsets; a.cam = d_obs_cam; a.kp = d_obs_kp; a.obs_stride = obs_stride;
    a.R = d_R; a.T = d_T; a.n_cams = d_n_cams; a.cam_stride = cam_stride; a.xy = d_xy; a.xy_item = (size_t)cam_stride * kp_stride * 2; a.kp_stride = kp_stride;
    a.out_points = reinterpret_cast<float4 *>(d_out_points); a.status = d_status; a.counts = d_counts; a.info = d_info; a.stats = d_stats;
    return launch_tracks(ctx, a, batch, h_K);
}

int vslam_world_retriangulate(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy, int xy_frames, const float *h_K,
                              const vslam_track_params *params, int32_t *d_status, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy && h_K, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &m))) return rc;
    VS_REQUIRE(ctx, xy_frames >= m.frames, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, m.max_frames <= kMaxCams, VSLAM_ERR_CAPACITY);
    TrackArgs a;
    if ((rc = track_setup(ctx, params, h_K, a))) return rc;
    VS_ALIGNED(ctx, d_xy, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_status, d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    const size_t T = m.tracks, P = m.map_capacity, O = m.obs_capacity, Fr = m.max_frames;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_tracks_i32", sizeof(int32_t) * T * ((P + 1) + 2 * O + 5), &ptr))) return rc;
    int32_t *off = static_cast<int32_t *>(ptr), *frame = off + T * (P + 1), *kp = frame + T * O, *n_cams = kp + T * O, *stats = n_cams + T;
    if ((rc = vs_arena_get(ctx, "world_tracks_f64", sizeof(double) * T * Fr * 12, &ptr))) return rc;
    double *R = static_cast<double *>(ptr), *Tv = R + T * Fr * 9;
    if ((rc = vs_world_csr(ctx, world, map, off, frame, kp, nullptr))) return rc;
    if ((rc = vs_world_cameras(ctx, world, m.max_frames, m.frames, R, Tv, n_cams))) return rc;
    a.points = reinterpret_cast<const float4 *>(world->world_points); a.n_points = static_cast<const int32_t *>(m.d_sizes); a.pt_stride = m.map_capacity;
    a.off = off; a.cam = frame; a.kp = kp; a.obs_stride = m.obs_capacity;
    a.R = R; a.T = Tv; a.n_cams = n_cams; a.cam_stride = m.max_frames; a.xy = d_xy; a.xy_item = (size_t)xy_frames * m.kp_stride * 2;
    a.kp_stride = m.kp_stride;
    a.out_points = reinterpret_cast<float4 *>(world->world_points); a.status = d_status; a.counts = nullptr; a.info = nullptr;
    a.stats = d_stats ? d_stats : stats;
    return launch_tracks(ctx, a, m.tracks, h_K);
}

}  // extern "C"
