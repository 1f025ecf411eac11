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
// The polish is vslam_resect_poses' own launch on the compacted rows.  Further down: vslam_match_points (world points to keypoints
// by descriptor alone) and vslam_world_relocalise, which joins the two on a world attached to a map.
#include <cmath>

#include "ctx.h"
#include "pnp_math.h"
#include "search_math.h"
#include "../../include/vslam_pnp.h"
#include "../../include/vslam_search.h"

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

// exclusive prefix of a flag over the workgroup by ballots; every lane calls it.  lds: kPT / 64 words.
__device__ __forceinline__ int block_flag_scan(bool f, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) lds[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kPT / 64; w++) {
        const int c = lds[w];
        before += w < wave ? c : 0;
        total += c;
    }
    __syncthreads();
    return before + __popcll(bal & ((1ull << lane) - 1ull));
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
        const int slot = running + block_flag_scan(in, wave_n, total);
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

// ---- vslam_match_points: every point against every keypoint.  Grid (ceil(pt_stride / 256), batch), one lane per point with up to
// four of its observation descriptors in registers (further ones are read again per keypoint); the item's keypoint descriptors
// pass through LDS in tiles of 1024 (32 KB: VSLAM_MAX_KP x 32 B would not fit), and every lane reads the same row of the tile, a
// broadcast.  The choice, the proposal rule and the keys are search_math.h's; the resolution is search.hip's, over these
// proposals.
constexpr int kMTile = 1024;     // keypoints per LDS tile
constexpr int kMObs = 4;         // observation descriptors a lane keeps in registers
constexpr int kPropPart = 1 << 16, kPropCandidate = 1 << 17;   // beside d0 (<= 256) in a proposal's second word

struct MatchArgs {
    const float4 *points;
    const int32_t *n_points;
    int pt_stride;
    const int32_t *obs_offsets;
    const uint8_t *obs_desc;
    int obs_stride;
    const float2 *xy;
    const uint8_t *desc;
    const int32_t *n_kp;
    int kp_stride;
    const int32_t *taken;
    vs_search::SsParams prm;
    unsigned long long *keys;   // [batch][kp_stride], all ones ahead of the proposals
    int2 *prop;                 // [batch][pt_stride]: (k0 or -1, d0 | flags)
    int32_t *kp_of_point, *dist;
    double *corr_points;
    float2 *corr_xy;
    int32_t *corr_point, *corr_kp, *n_corr, *stats;
};

__device__ __forceinline__ void load_desc(const uint8_t *row, uint32_t (&w)[8]) {   // a 32-byte row, 16-byte aligned
    const uint4 a = reinterpret_cast<const uint4 *>(row)[0], b = reinterpret_cast<const uint4 *>(row)[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

__global__ __launch_bounds__(kPT) void match_propose_kernel(MatchArgs a) {
    using namespace vs_search;
    __shared__ uint4 tile[2 * kMTile];
    __shared__ uint8_t cand[kMTile];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    if (blockIdx.x * kPT >= n) return;   // the whole workgroup: the resolution writes the rows from n on
    const int n_kp = min(max(a.n_kp[b], 0), a.kp_stride);
    const int32_t *taken = a.taken ? a.taken + (size_t)b * a.kp_stride : nullptr;
    const int32_t *OO = a.obs_offsets + (size_t)b * (a.pt_stride + 1);
    const uint8_t *OD = a.obs_desc + (size_t)b * a.obs_stride * VSLAM_DESC_BYTES;
    const uint4 *D = reinterpret_cast<const uint4 *>(a.desc + (size_t)b * a.kp_stride * VSLAM_DESC_BYTES);
    const int i = blockIdx.x * kPT + tid;
    bool part = false;
    int o0 = 0, o1 = 0;
    if (i < n) {
        const float4 P = a.points[(size_t)b * a.pt_stride + i];
        o0 = OO[i];
        o1 = OO[i + 1];
        part = o0 >= 0 && o0 < o1 && o1 <= a.obs_stride && isfinite(P.x) && isfinite(P.y) && isfinite(P.z);
    }
    const int cnt = part ? o1 - o0 : 0;
    uint32_t obs[kMObs][8];
#pragma unroll
    for (int q = 0; q < kMObs; q++) {
        if (q < cnt) {
            load_desc(OD + (size_t)(o0 + q) * VSLAM_DESC_BYTES, obs[q]);
        } else {
#pragma unroll
            for (int w = 0; w < 8; w++) obs[q][w] = 0u;
        }
    }
    SsBest best;
    bool any = false;
    for (int base = 0; base < n_kp; base += kMTile) {
        const int m = min(kMTile, n_kp - base);
        for (int j = tid; j < 2 * m; j += kPT) tile[j] = D[2 * (size_t)base + j];
        for (int j = tid; j < m; j += kPT) cand[j] = (taken && taken[base + j] >= 0) ? 0 : 1;
        __syncthreads();
        if (part) {
            for (int j = 0; j < m; j++) {
                if (!cand[j]) continue;   // the same in every lane
                any = true;
                const uint4 lo = tile[2 * j], hi = tile[2 * j + 1];
                const uint32_t dk[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                uint32_t d = kSsNone;
#pragma unroll
                for (int q = 0; q < kMObs; q++) {
                    if (q < cnt) {
                        const uint32_t cur = ss_ham256(dk, obs[q]);
                        d = cur < d ? cur : d;
                    }
                }
                for (int o = o0 + kMObs; o < o1; o++) {
                    uint32_t dobs[8];
                    load_desc(OD + (size_t)o * VSLAM_DESC_BYTES, dobs);
                    const uint32_t cur = ss_ham256(dk, dobs);
                    d = cur < d ? cur : d;
                }
                ss_offer(best, d, (uint32_t)(base + j));
            }
        }
        __syncthreads();
    }
    if (i >= n) return;
    const bool proposes = part && ss_proposes(best, a.prm);
    int2 pr;
    pr.x = proposes ? (int)best.k0 : -1;
    pr.y = (proposes ? (int)best.d0 : 0) | (part ? kPropPart : 0) | (any ? kPropCandidate : 0);
    a.prop[(size_t)b * a.pt_stride + i] = pr;
    if (proposes) atomicMin(&a.keys[(size_t)b * a.kp_stride + best.k0], ss_key(best.d0, (uint32_t)i));
}

// one workgroup per item: a point has found its keypoint iff the key there is its own; ordered compaction in chunks of 256 points
__global__ __launch_bounds__(kPT) void match_resolve_kernel(MatchArgs a) {
    using namespace vs_search;
    __shared__ int scan_lds[kPT / 64];
    __shared__ int counts[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    if (tid < 3) counts[tid] = 0;
    __syncthreads();
    const unsigned long long *keys = a.keys + (size_t)b * a.kp_stride;
    const float2 *XY = a.xy + (size_t)b * a.kp_stride;
    int run = 0, part = 0, with_candidate = 0, proposing = 0;
    for (int base = 0; base < a.pt_stride; base += kPT) {   // ascending chunks: the compacted order is the points' order
        const int i = base + tid;
        int k0 = -1, d0 = -1;
        bool found = false;
        if (i < n) {
            const int2 pr = a.prop[(size_t)b * a.pt_stride + i];
            part += (pr.y & kPropPart) ? 1 : 0;
            with_candidate += (pr.y & kPropCandidate) ? 1 : 0;
            if (pr.x >= 0) {
                proposing++;
                k0 = pr.x;
                d0 = pr.y & 0xFFFF;
                found = keys[k0] == ss_key((uint32_t)d0, (uint32_t)i);
            }
        }
        int chunk;
        const int pos = run + block_flag_scan(found, scan_lds, chunk);
        if (i < a.pt_stride) {
            a.kp_of_point[(size_t)b * a.pt_stride + i] = found ? k0 : -1;
            a.dist[(size_t)b * a.pt_stride + i] = found ? d0 : -1;
        }
        if (found) {   // one point per keypoint at the most, so pos < n_kp <= kp_stride
            const size_t slot = (size_t)b * a.kp_stride + pos;
            const float4 P = a.points[(size_t)b * a.pt_stride + i];
            a.corr_points[3 * slot] = (double)P.x;
            a.corr_points[3 * slot + 1] = (double)P.y;
            a.corr_points[3 * slot + 2] = (double)P.z;
            a.corr_xy[slot] = XY[k0];
            if (a.corr_point) a.corr_point[slot] = i;
            if (a.corr_kp) a.corr_kp[slot] = k0;
        }
        run += chunk;
    }
    if (tid == 0) a.n_corr[b] = run;
    if (!a.stats) return;
    atomicAdd(&counts[0], part);
    atomicAdd(&counts[1], with_candidate);
    atomicAdd(&counts[2], proposing);
    __syncthreads();
    if (tid < 3) a.stats[(size_t)b * 4 + tid] = counts[tid];
    if (tid == 3) a.stats[(size_t)b * 4 + 3] = run;
}

// the fill of the keys and the two launches; everything has been checked
int launch_match(vslam_ctx *ctx, MatchArgs a, int batch) {
    int rc;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "match_keys", sizeof(unsigned long long) * (size_t)batch * a.kp_stride, &ptr))) return rc;
    a.keys = static_cast<unsigned long long *>(ptr);
    if ((rc = vs_arena_get(ctx, "match_prop", sizeof(int2) * (size_t)batch * a.pt_stride, &ptr))) return rc;
    a.prop = static_cast<int2 *>(ptr);
    VS_HIP(ctx, hipMemsetAsync(a.keys, 0xFF, sizeof(unsigned long long) * (size_t)batch * a.kp_stride, ctx->stream));
    {
        VsProfScope ps(ctx, "match_propose_kernel");
        match_propose_kernel<<<dim3(vs_div_up(a.pt_stride, kPT), batch), kPT, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "match_resolve_kernel");
        match_resolve_kernel<<<batch, kPT, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

bool match_params_ok(const vslam_match_params &p) {
    return p.dist_threshold >= 1 && p.dist_threshold <= 257 && p.ratio10 >= 0 && p.ratio10 <= 10;
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

vslam_world *vs_map_world(vslam_map *map);                                                                                   // map.hip
int vs_world_search_writeback(vslam_ctx *ctx, vslam_world *world, int f1, double *R, double *T, double *mark);   // search.hip

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

int vslam_match_params_default(vslam_match_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->dist_threshold = 64; out->ratio10 = 8;
    return VSLAM_OK;
}

int vslam_match_points(vslam_ctx *ctx, const float *d_points, const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets,
                       const uint8_t *d_obs_desc, int obs_stride, const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp,
                       int kp_stride, const int32_t *d_kp_taken, int batch, const vslam_match_params *params, int32_t *d_kp_of_point,
                       int32_t *d_dist, double *d_corr_points, float *d_corr_xy, int32_t *d_corr_point, int32_t *d_corr_kp,
                       int32_t *d_n_corr, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_points && d_n_points && d_obs_offsets && d_obs_desc && d_xy && d_desc && d_n_kp, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_kp_of_point && d_dist && d_corr_points && d_corr_xy && d_n_corr, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && pt_stride > 0 && obs_stride > 0 && kp_stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    vslam_match_params p;
    vslam_match_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, match_params_ok(p), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_points, 16);   // float4 rows
    VS_ALIGNED(ctx, d_desc, 16);     // descriptor rows move as uint4 pairs
    VS_ALIGNED(ctx, d_obs_desc, 16);
    VS_ALIGNED(ctx, d_xy, 8);        // float2 rows
    VS_ALIGNED(ctx, d_corr_xy, 8);
    VS_ALIGNED(ctx, d_corr_points, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_points, d_obs_offsets, d_n_kp, d_kp_taken, d_kp_of_point, d_dist, d_corr_point, d_corr_kp, d_n_corr,
                                d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    MatchArgs a;
    a.points = reinterpret_cast<const float4 *>(d_points); a.n_points = d_n_points; a.pt_stride = pt_stride;
    a.obs_offsets = d_obs_offsets; a.obs_desc = d_obs_desc; a.obs_stride = obs_stride;
    a.xy = reinterpret_cast<const float2 *>(d_xy); a.desc = d_desc; a.n_kp = d_n_kp; a.kp_stride = kp_stride; a.taken = d_kp_taken;
    a.prm = vs_search::ss_params(1.0, p.dist_threshold, p.ratio10);   // no disc: the radius is not read
    a.keys = nullptr; a.prop = nullptr;
    a.kp_of_point = d_kp_of_point; a.dist = d_dist; a.corr_points = d_corr_points; a.corr_xy = reinterpret_cast<float2 *>(d_corr_xy);
    a.corr_point = d_corr_point; a.corr_kp = d_corr_kp; a.n_corr = d_n_corr; a.stats = d_stats;
    return launch_match(ctx, a, batch);
}

int vslam_world_relocalise(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                           const int32_t *d_n_cur, const float *h_K, const uint32_t *d_seeds, const vslam_match_params *match,
                           const vslam_pnp_params *pnp, const vslam_resect_params *polish, int32_t *d_found, int32_t *d_winner,
                           int32_t *d_n_inliers, int32_t *d_corr_point, int32_t *d_corr_kp, int32_t *d_n_corr, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy_cur && d_desc_cur && d_n_cur && h_K && d_seeds, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_found && d_winner && d_n_inliers && d_corr_point && d_corr_kp && d_n_corr, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, world->ctx == ctx && vs_map_world(map) == world && world->world_points, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc = vslam_map_view(map, &m);
    if (rc != VSLAM_OK) return rc;
    VS_REQUIRE(ctx, m.frames == world->frames && m.frames >= 1, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xy_cur, 8);
    VS_ALIGNED(ctx, d_desc_cur, 16);
    VS_ALIGNED(ctx, d_stats, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_cur, d_seeds, d_found, d_winner, d_n_inliers, d_corr_point, d_corr_kp, d_n_corr) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_match_params mp;
    vslam_match_params_default(&mp);
    if (match) mp = *match;
    vslam_pnp_params pp;
    vslam_pnp_params_default(&pp);
    if (pnp) pp = *pnp;
    VS_REQUIRE(ctx, match_params_ok(mp) && params_ok(pp) && (!polish || vs_resect_params_ok(*polish)), VSLAM_ERR_INVALID);
    const int T = m.tracks, P = m.map_capacity, O = m.obs_capacity, Kp = m.kp_stride;
    // workspace: the map's CSR and its descriptors, the per-point outputs of the match, what was matched, the mask and the inliers
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "relocalise_i32", sizeof(int32_t) * (size_t)T * ((size_t)(P + 1) + 2 * (size_t)P + (size_t)Kp), &ptr))) return rc;
    int32_t *off = static_cast<int32_t *>(ptr), *kp_of_point = off + (size_t)T * (P + 1), *dist = kp_of_point + (size_t)T * P,
            *inlier = dist + (size_t)T * P;
    if ((rc = vs_arena_get(ctx, "relocalise_desc", (size_t)T * O * VSLAM_DESC_BYTES, &ptr))) return rc;
    uint8_t *obs_desc = static_cast<uint8_t *>(ptr);
    if ((rc = vs_arena_get(ctx, "relocalise_f64", sizeof(double) * (size_t)T * (16 + 6 * (size_t)Kp), &ptr))) return rc;
    double *R = static_cast<double *>(ptr), *Tr = R + (size_t)T * 9, *mark = Tr + (size_t)T * 3, *corr_points = mark + (size_t)T * 4,
           *in_points = corr_points + (size_t)T * Kp * 3;
    if ((rc = vs_arena_get(ctx, "relocalise_xy", sizeof(float) * 4 * (size_t)T * Kp, &ptr))) return rc;
    float *corr_xy = static_cast<float *>(ptr), *in_xy = corr_xy + (size_t)T * Kp * 2;
    if ((rc = vslam_map_observation_descriptors(ctx, map, off, obs_desc))) return rc;
    if ((rc = vslam_match_points(ctx, world->world_points, static_cast<const int32_t *>(m.d_sizes), P, off, obs_desc, O, d_xy_cur, d_desc_cur,
                                 d_n_cur, Kp, nullptr, T, &mp, kp_of_point, dist, corr_points, corr_xy, d_corr_point, d_corr_kp, d_n_corr,
                                 nullptr)))
        return rc;
    if ((rc = vslam_pnp_ransac(ctx, corr_points, corr_xy, d_n_corr, T, Kp, h_K, d_seeds, &pp, polish, R, Tr, inlier, in_points, in_xy, nullptr,
                               d_n_inliers, d_winner, nullptr, d_stats)))
        return rc;
    relocalise_mark_kernel<<<vs_div_up(T, kPT), kPT, 0, ctx->stream>>>(d_winner, T, mark, d_found);
    VS_HIP(ctx, hipGetLastError());
    return vs_world_search_writeback(ctx, world, m.frames - 1, R, Tr, mark);
}

}  // extern "C"
