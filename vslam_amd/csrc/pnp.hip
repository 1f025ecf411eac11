// A pose without a prior (include/vslam_pnp.h): P3P RANSAC over 3-D / 2-D correspondences for a batch of independent items, all in
// f64 and never fused; every decision is pnp_math.h's, which tests/native/pnp_serial.cpp walks on the host.  Three kernels:
//   solve   one workgroup per item: the finiteness of the item, then one lane per hypothesis -- its set, its P3P -- writing up to
//           four poses and their flags into the arena.  It is a few thousand operations per hypothesis against the count's
//           ~45 per pose and correspondence, and it is kept out of the count so that kernel's registers hold a pose and nothing
//           else.
//   count   the hot path.  One lane owns one pose (12 f64 in registers) and its count; a workgroup of 256 poses stages the item's
//           correspondences through LDS in tiles of 256, widened once, and every lane reads the same tile entry (a broadcast,
//           no bank conflict).  No atomics, no per-correspondence global traffic.
//   select  one workgroup per item: the maximum of the integer keys, then the winner's mask again (the same function on the same
//           operands: the same bits), compacted in ascending order with a ballot scan.
// The polish is vslam_resect_poses' own launch on the compacted rows.  Further down: vslam_world_relocalise, which joins
// vslam_match_points (search.hip: world points to keypoints by descriptor alone) and this on a world attached to a map.
#include <cmath>

#include "block_scan.h"
#include "ctx.h"
#include "pnp_math.h"
#include "../../include/vslam_pnp.h"

#pragma clang fp contract(off)

using namespace vs_pnp;

namespace {
constexpr int kPT = 256;         // lanes per workgroup, every kernel of this file
constexpr int kPTile = 256;      // correspondences per LDS tile of the count

struct PnpArgs {
    const double *__restrict__ points;
    const float2 *__restrict__ xy;
    const int32_t *__restrict__ n;
    const uint32_t *__restrict__ seeds;
    int stride, hypotheses, min_inliers;
    double thr2;
    // the arena: [batch][4 hypotheses] poses of 12 f64, their flags and counts
    double *poses;
    int32_t *ok, *counts;
    double *R, *T;
    int32_t *inlier;
    double *corr_points;
    float2 *corr_xy;
    int32_t *corr_index, *n_inliers, *winner, *counts_out;
    double *stats;
};

__device__ __forceinline__ int item_n(const PnpArgs &a, int b) { return min(max(a.n[b], 0), a.stride); }

__global__ __launch_bounds__(kPT) void pnp_solve_kernel(PnpArgs a, VsK Kc) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = item_n(a, b);
    const double *P = a.points + (size_t)b * a.stride * 3;
    const float2 *X = a.xy + (size_t)b * a.stride;
    double K[9], Kinv[9];
    bool bad = n < 4;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        K[k] = (double)Kc.v[k];
        bad = bad || !std::isfinite(K[k]);
    }
    auto at = [&](int i, double(&p)[3], double(&x)[2]) {
        p[0] = P[3 * (size_t)i];
        p[1] = P[3 * (size_t)i + 1];
        p[2] = P[3 * (size_t)i + 2];
        const float2 o = X[i];
        x[0] = (double)o.x;
        x[1] = (double)o.y;
    };
    for (int i = tid; i < n; i += kPT) {
        double p[3], x[2];
        at(i, p, x);
        bad = bad || !pn_finite_row(p, x);
    }
    bad = __syncthreads_or(bad) != 0;
    pn_kinv(K, Kinv);
    const uint32_t seed = a.seeds[b];
    for (int h = tid; h < a.hypotheses; h += kPT) {
        LmCam cam[4];
        bool ok[4] = {false, false, false, false};
        if (!bad) pn_hypothesis(Kinv, seed, h, n, at, cam, ok);
        const size_t base = ((size_t)b * a.hypotheses + h) * 4;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            a.ok[base + s] = ok[s] ? 1 : 0;
            if (!ok[s]) continue;
            double *o = a.poses + (base + s) * 12;
#pragma unroll
            for (int k = 0; k < 9; k++) o[k] = cam[s].R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) o[9 + k] = cam[s].T[k];
        }
    }
}

struct alignas(16) PnpEntry {   // one correspondence, widened: three 16-byte reads
    double P[3], x[2], pad;
};

__device__ __forceinline__ void load_pose(const PnpArgs &a, size_t pose, LmCam &c) {
    const double *o = a.poses + pose * 12;
#pragma unroll
    for (int k = 0; k < 9; k++) c.R[k] = o[k];
#pragma unroll
    for (int k = 0; k < 3; k++) c.T[k] = o[9 + k];
}

// grid (4 hypotheses / 256, batch)
__global__ __launch_bounds__(kPT) void pnp_count_kernel(PnpArgs a, VsK Kc) {
    __shared__ PnpEntry tile[kPTile];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = item_n(a, b);
    const size_t pose = (size_t)b * a.hypotheses * 4 + (size_t)blockIdx.x * kPT + tid;
    const bool ok = a.ok[pose] != 0;
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = (double)Kc.v[k];
    LmCam c;
#pragma unroll
    for (int k = 0; k < 9; k++) c.R[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) c.T[k] = 0.0;
    if (ok) load_pose(a, pose, c);
    const double *P = a.points + (size_t)b * a.stride * 3;
    const float2 *X = a.xy + (size_t)b * a.stride;
    int count = 0;
    for (int base = 0; base < n; base += kPTile) {
        const int m = min(kPTile, n - base);
        if (tid < m) {
            const size_t i = (size_t)base + tid;
            const float2 o = X[i];
            PnpEntry e;
            e.P[0] = P[3 * i];
            e.P[1] = P[3 * i + 1];
            e.P[2] = P[3 * i + 2];
            e.x[0] = (double)o.x;
            e.x[1] = (double)o.y;
            e.pad = 0.0;
            tile[tid] = e;
        }
        __syncthreads();
        for (int j = 0; j < m; j++) {
            const PnpEntry e = tile[j];
            count += pn_inlier(K, c, e.P, e.x, a.thr2) ? 1 : 0;
        }
        __syncthreads();
    }
    const int32_t v = ok ? count : -1;
    a.counts[pose] = v;
    if (a.counts_out) a.counts_out[pose] = v;
}

__global__ __launch_bounds__(kPT) void pnp_select_kernel(PnpArgs a, VsK Kc) {
    __shared__ uint32_t best;
    __shared__ int wave_n[kPT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = item_n(a, b);
    if (tid == 0) best = 0u;
    __syncthreads();
    const size_t pose0 = (size_t)b * a.hypotheses * 4;
    uint32_t mine = 0u;
    for (int p = tid; p < a.hypotheses * 4; p += kPT) mine = max(mine, pn_key(a.counts[pose0 + p], p));
    if (mine) atomicMax(&best, mine);   // integers: the maximum is the same in any order
    __syncthreads();
    const uint32_t key = best;
    const bool found = key != 0u && pn_key_count(key) >= a.min_inliers;
    const int win = pn_key_pose(key);
    const double qnan = __builtin_nan("");
    if (tid == 0) {
        a.winner[b] = found ? win : -1;
        a.n_inliers[b] = found ? pn_key_count(key) : 0;
    }
    if (a.stats && tid < 4) a.stats[(size_t)b * 4 + tid] = qnan;
    int32_t *inl = a.inlier + (size_t)b * a.stride;
    if (!found) {
        for (int i = tid; i < a.stride; i += kPT) inl[i] = 0;
        return;
    }
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = (double)Kc.v[k];
    LmCam c;
    load_pose(a, pose0 + win, c);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) a.R[(size_t)b * 9 + k] = c.R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) a.T[(size_t)b * 3 + k] = c.T[k];
    }
    const double *P = a.points + (size_t)b * a.stride * 3;
    const float2 *X = a.xy + (size_t)b * a.stride;
    double *cp = a.corr_points + (size_t)b * a.stride * 3;
    float2 *cx = a.corr_xy + (size_t)b * a.stride;
    int32_t *ci = a.corr_index ? a.corr_index + (size_t)b * a.stride : nullptr;
    int running = 0;   // the same in every lane
    for (int base = 0; base < a.stride; base += kPT) {
        const int i = base + tid;
        bool in = false;
        double p[3] = {0.0, 0.0, 0.0};
        float2 o = make_float2(0.f, 0.f);
        if (i < n) {
            p[0] = P[3 * (size_t)i];
            p[1] = P[3 * (size_t)i + 1];
            p[2] = P[3 * (size_t)i + 2];
            o = X[i];
            const double x[2] = {(double)o.x, (double)o.y};
            in = pn_inlier(K, c, p, x, a.thr2);
        }
        if (i < a.stride) inl[i] = in ? 1 : 0;
        int total;
        const int slot = running + vs_block_flag_scan<kPT>(in, wave_n, total);
        if (in) {
            cp[3 * (size_t)slot] = p[0];
            cp[3 * (size_t)slot + 1] = p[1];
            cp[3 * (size_t)slot + 2] = p[2];
            cx[slot] = o;
            if (ci) ci[slot] = i;
        }
        running += total;
    }
}

// ---- vslam_world_relocalise: the tracks that were found, as the mark vs_world_search_writeback reads (a number in [3]), and d_found
__global__ __launch_bounds__(kPT) void relocalise_mark_kernel(const int32_t *__restrict__ winner, int tracks, double *__restrict__ mark,
                                                              int32_t *__restrict__ found) {
    const int b = blockIdx.x * kPT + threadIdx.x;
    if (b >= tracks) return;
    const bool f = winner[b] >= 0;
    found[b] = f ? 1 : 0;
    mark[(size_t)b * 4 + 3] = f ? 1.0 : __builtin_nan("");
}

bool params_ok(const vslam_pnp_params &p) {
    return p.hypotheses >= 64 && p.hypotheses <= 1024 && p.hypotheses % 64 == 0 && p.min_inliers >= 4 && std::isfinite(p.inlier_px) &&
           p.inlier_px > 0.0;
}
}  // namespace

extern "C" {

int vslam_pnp_params_default(vslam_pnp_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->hypotheses = 128; out->min_inliers = 8; out->inlier_px = 2.0;
    return VSLAM_OK;
}

int vslam_pnp_ransac(vslam_ctx *ctx, const double *d_points, const float *d_xy, const int32_t *d_n, int batch, int stride, const float *h_K,
                     const uint32_t *d_seeds, const vslam_pnp_params *params, const vslam_resect_params *polish, double *d_R, double *d_T,
                     int32_t *d_inlier, double *d_corr_points, float *d_corr_xy, int32_t *d_corr_index, int32_t *d_n_inliers,
                     int32_t *d_winner, int32_t *d_counts, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_points && d_xy && d_n && h_K && d_seeds && d_R && d_T && d_inlier && d_corr_points && d_corr_xy && d_n_inliers && d_winner,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    vslam_pnp_params p;
    vslam_pnp_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, !polish || vs_resect_params_ok(*polish), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xy, 8);        // float2 rows
    VS_ALIGNED(ctx, d_corr_xy, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_points, d_R, d_T, d_corr_points, d_stats) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n, d_seeds, d_inlier, d_corr_index, d_n_inliers, d_winner, d_counts) % 4 == 0, VSLAM_ERR_INVALID);
    const size_t poses = (size_t)batch * p.hypotheses * 4;
    int rc;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "pnp_poses", sizeof(double) * 12 * poses, &ptr))) return rc;
    PnpArgs a;
    a.poses = static_cast<double *>(ptr);
    if ((rc = vs_arena_get(ctx, "pnp_counts", sizeof(int32_t) * 2 * poses, &ptr))) return rc;
    a.ok = static_cast<int32_t *>(ptr);
    a.counts = a.ok + poses;
    a.points = d_points; a.xy = reinterpret_cast<const float2 *>(d_xy); a.n = d_n; a.seeds = d_seeds;
    a.stride = stride; a.hypotheses = p.hypotheses; a.min_inliers = p.min_inliers;
    a.thr2 = p.inlier_px * p.inlier_px;
    a.R = d_R; a.T = d_T; a.inlier = d_inlier; a.corr_points = d_corr_points; a.corr_xy = reinterpret_cast<float2 *>(d_corr_xy);
    a.corr_index = d_corr_index; a.n_inliers = d_n_inliers; a.winner = d_winner; a.counts_out = d_counts; a.stats = d_stats;
    const VsK K = vs_pack_K(h_K);
    {
        VsProfScope ps(ctx, "pnp_solve_kernel");
        pnp_solve_kernel<<<batch, kPT, 0, ctx->stream>>>(a, K);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "pnp_count_kernel");
        pnp_count_kernel<<<dim3(p.hypotheses * 4 / kPT, batch), kPT, 0, ctx->stream>>>(a, K);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "pnp_select_kernel");
        pnp_select_kernel<<<batch, kPT, 0, ctx->stream>>>(a, K);
    }
    VS_HIP(ctx, hipGetLastError());
    if (!polish) return VSLAM_OK;
    return vslam_resect_poses(ctx, d_corr_points, d_corr_xy, d_n_inliers, batch, stride, h_K, polish, d_R, d_T, d_stats);
}

int vslam_world_relocalise(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                           const int32_t *d_n_cur, const float *h_K, const uint32_t *d_seeds, const vslam_match_params *match,
                           const vslam_pnp_params *pnp, const vslam_resect_params *polish, int32_t *d_found, int32_t *d_winner,
                           int32_t *d_n_inliers, int32_t *d_corr_point, int32_t *d_corr_kp, int32_t *d_n_corr, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy_cur && d_desc_cur && d_n_cur && h_K && d_seeds, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_found && d_winner && d_n_inliers && d_corr_point && d_corr_kp && d_n_corr, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_cur, d_seeds, d_found, d_winner, d_n_inliers, d_corr_point, d_corr_kp, d_n_corr) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_match_params mp;
    vslam_match_params_default(&mp);
    if (match) mp = *match;
    vslam_pnp_params pp;
    vslam_pnp_params_default(&pp);
    if (pnp) pp = *pnp;
    VS_REQUIRE(ctx, vs_match_params_ok(mp) && params_ok(pp) && (!polish || vs_resect_params_ok(*polish)), VSLAM_ERR_INVALID);
    VsWorldCorr c;   // R, T: the winner's pose; mark: a number in [3] where the track was found
    int rc;
    if ((rc = vs_world_corr_begin(ctx, world, map, d_xy_cur, d_desc_cur, d_stats, &c))) return rc;
    const int T = c.m.tracks, Kp = c.m.kp_stride;
    // beside the shared workspace: the winner's inliers (points, xy) and its mask
    void *ptr = nullptr;
    const size_t rows = (size_t)T * Kp;
    if ((rc = vs_arena_get(ctx, "relocalise_inliers", rows * (3 * sizeof(double) + 2 * sizeof(float) + sizeof(int32_t)), &ptr))) return rc;
    double *in_points = static_cast<double *>(ptr);
    float *in_xy = reinterpret_cast<float *>(in_points + (size_t)T * Kp * 3);
    int32_t *inlier = reinterpret_cast<int32_t *>(in_xy + (size_t)T * Kp * 2);
    if ((rc = vslam_match_points(ctx, world->world_points, static_cast<const int32_t *>(c.m.d_sizes), c.m.map_capacity, c.off, c.obs_desc,
                                 c.m.obs_capacity, d_xy_cur, d_desc_cur, d_n_cur, Kp, nullptr, T, &mp, c.kp_of_point, c.dist, c.corr_points,
                                 c.corr_xy, d_corr_point, d_corr_kp, d_n_corr, nullptr)))
        return rc;
    if ((rc = vslam_pnp_ransac(ctx, c.corr_points, c.corr_xy, d_n_corr, T, Kp, h_K, d_seeds, &pp, polish, c.R, c.T, inlier, in_points, in_xy,
                               nullptr, d_n_inliers, d_winner, nullptr, d_stats)))
        return rc;
    relocalise_mark_kernel<<<vs_div_up(T, kPT), kPT, 0, ctx->stream>>>(d_winner, T, c.mark, d_found);
    VS_HIP(ctx, hipGetLastError());
    return vs_world_search_writeback(ctx, world, c.m.frames - 1, c.R, c.T, c.mark);
}

}  // extern "C"
