// The similarity between two views (include/vslam_sim3.h): 3-point RANSAC over 3-D / 3-D correspondences for a batch of independent
// items and its 7-parameter polish, all in f64 and never fused; every decision is sim3_math.h's, which
// tests/native/sim3_serial.cpp walks on the host.  Four kernels:
//   solve   one workgroup per item: the finiteness of the item, then one lane per hypothesis -- its set, its model, M_a and M_b.
//           The models that are kept are COMPACTED in ascending h (a ballot scan), so the count walks no empty slot.
//   count   the hot path.  A workgroup is 64 models x 4 ranges of correspondences: wave w of the workgroup counts entries
//           64 w .. 64 w + 63 of every LDS tile of 256 (ten f64 per entry, the pixels widened once at the fill) for the same 64
//           models, a lane per model with its two matrices (24 f64) and its count in registers; every lane of a wave reads the
//           same entry (a broadcast).  The four partial counts are added in LDS: integers, so the split changes no bit.  No
//           division, no scratch, no atomics on global memory, no per-correspondence global traffic.  A workgroup whose 64 slots
//           lie past the item's kept models leaves at once.
//   select  one workgroup per item: the maximum of the integer keys, then the winner's mask again (the same function on the same
//           operands: the same bits), compacted in ascending order with a ballot scan.
//   refine  one workgroup per item: the rounds of sim3_math.h's s3_run, sums closed by block_reduce.h.
// Further down, on a world attached to a map: the gather that forms the correspondences of two recorded frames (one workgroup per
// item, a ballot scan in match order), the world-to-world similarity of the found items, and vslam_world_apply_sim3's one kernel.
#include <algorithm>
#include <cmath>
#include <vector>

#include "block_reduce.h"
#include "block_scan.h"
#include "ctx.h"
#include "sim3_math.h"
#include "../../include/vslam_sim3.h"

#pragma clang fp contract(off)

using namespace vs_sim3;

namespace {
constexpr int kST = 256;          // lanes per workgroup, every kernel of this file
constexpr int kSTile = 256;       // correspondences per LDS tile of the count
constexpr int kSModels = 64;      // models per workgroup of the count
constexpr int kSRanges = kST / kSModels;
constexpr int kSModelF64 = 37;    // s, R, t, Ma, Mb

struct Sim3Args {
    const double *__restrict__ A;
    const float2 *__restrict__ xa;
    const double *__restrict__ B;
    const float2 *__restrict__ xb;
    const int32_t *__restrict__ n;
    const uint32_t *__restrict__ seeds;
    int stride, hypotheses, min_inliers;
    double px;
    // the arena: [batch][hypotheses] models (compacted per item), the h of each slot, the slot of each h, the counts by h, and
    // [batch] the number of kept models
    double *models;
    int32_t *slot_h, *h_slot, *counts, *n_valid;
    double *scale, *R, *T;
    int32_t *inlier, *corr_index, *n_inliers, *winner, *counts_out;
    double *stats;
};

__device__ __forceinline__ int item_n(const Sim3Args &a, int b) { return min(max(a.n[b], 0), a.stride); }

__device__ __forceinline__ void load_row(const Sim3Args &a, int b, int i, double (&A)[3], double (&xa)[2], double (&B)[3], double (&xb)[2]) {
    const size_t r = (size_t)b * a.stride + i;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        A[k] = a.A[3 * r + k];
        B[k] = a.B[3 * r + k];
    }
    const float2 oa = a.xa[r], ob = a.xb[r];
    xa[0] = (double)oa.x;
    xa[1] = (double)oa.y;
    xb[0] = (double)ob.x;
    xb[1] = (double)ob.y;
}

__global__ __launch_bounds__(kST) void sim3_solve_kernel(Sim3Args a, VsK Kc) {
    __shared__ int wave_n[kST / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = item_n(a, b);
    double K[9];
    bool bad = n < 4;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        K[k] = (double)Kc.v[k];
        bad = bad || !std::isfinite(K[k]);
    }
    for (int i = tid; i < n; i += kST) {
        double A[3], xa[2], B[3], xb[2];
        load_row(a, b, i, A, xa, B, xb);
        bad = bad || !s3_finite_row(A, xa, B, xb);
    }
    bad = __syncthreads_or(bad) != 0;
    const uint32_t seed = a.seeds[b];
    auto at = [&](int i, double(&A)[3], double(&B)[3]) {
        const size_t r = (size_t)b * a.stride + i;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            A[k] = a.A[3 * r + k];
            B[k] = a.B[3 * r + k];
        }
    };
    const size_t item0 = (size_t)b * a.hypotheses;
    int running = 0;   // the same in every lane
    for (int base = 0; base < a.hypotheses; base += kST) {
        const int h = base + tid;   // hypotheses is a multiple of 64: whole waves are in or out
        S3Model m;
        S3Proj p;
        bool ok = false;
        if (h < a.hypotheses && !bad) ok = s3_hypothesis(K, seed, h, n, at, m, p);
        int total;
        const int slot = running + vs_block_flag_scan<kST>(ok, wave_n, total);
        running += total;
        if (h >= a.hypotheses) continue;
        a.h_slot[item0 + h] = ok ? slot : -1;
        a.counts[item0 + h] = -1;
        if (a.counts_out) a.counts_out[item0 + h] = -1;
        if (!ok) continue;
        a.slot_h[item0 + slot] = h;
        double *o = a.models + (item0 + slot) * kSModelF64;
        o[0] = m.s;
#pragma unroll
        for (int k = 0; k < 9; k++) o[1 + k] = m.R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) o[10 + k] = m.t[k];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            o[13 + k] = p.Ma[k];
            o[25 + k] = p.Mb[k];
        }
    }
    if (tid == 0) a.n_valid[b] = running;
}

struct alignas(16) Sim3Entry {   // one correspondence, widened: five 16-byte reads
    double A[3], B[3], xa[2], xb[2];
};

__device__ __forceinline__ void load_proj(const double *__restrict__ o, S3Proj &p) {
#pragma unroll
    for (int k = 0; k < 12; k++) {
        p.Ma[k] = o[13 + k];
        p.Mb[k] = o[25 + k];
    }
}

// grid (hypotheses / 64, batch)
__global__ __launch_bounds__(kST) void sim3_count_kernel(Sim3Args a) {
    __shared__ Sim3Entry tile[kSTile];
    __shared__ int part[kSRanges][kSModels];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nv = a.n_valid[b];
    if ((int)blockIdx.x * kSModels >= nv) return;   // the whole workgroup: no kept model in its slots
    const int n = item_n(a, b);
    const int lane = tid & (kSModels - 1), range = tid / kSModels;
    const int slot = blockIdx.x * kSModels + lane;
    const bool live = slot < nv;
    const size_t item0 = (size_t)b * a.hypotheses;
    S3Proj p;
#pragma unroll
    for (int k = 0; k < 12; k++) p.Ma[k] = p.Mb[k] = 0.0;
    if (live) load_proj(a.models + (item0 + slot) * kSModelF64, p);
    int count = 0;
    for (int base = 0; base < n; base += kSTile) {
        const int m = min(kSTile, n - base);
        if (tid < m) {
            Sim3Entry e;
            load_row(a, b, base + tid, e.A, e.xa, e.B, e.xb);
            tile[tid] = e;
        }
        __syncthreads();
        const int hi = min(m, (range + 1) * kSModels);
        for (int j = range * kSModels; j < hi; j++) {
            const Sim3Entry e = tile[j];
            count += s3_inlier(p, e.A, e.xa, e.B, e.xb, a.px) ? 1 : 0;
        }
        __syncthreads();
    }
    part[range][lane] = count;
    __syncthreads();
    if (range != 0 || !live) return;
    int total = 0;
#pragma unroll
    for (int r = 0; r < kSRanges; r++) total += part[r][lane];
    const int h = a.slot_h[item0 + slot];
    a.counts[item0 + h] = total;
    if (a.counts_out) a.counts_out[item0 + h] = total;
}

__global__ __launch_bounds__(kST) void sim3_select_kernel(Sim3Args a) {
    __shared__ uint32_t best;
    __shared__ int wave_n[kST / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = item_n(a, b);
    if (tid == 0) best = 0u;
    __syncthreads();
    const size_t item0 = (size_t)b * a.hypotheses;
    uint32_t mine = 0u;
    for (int h = tid; h < a.hypotheses; h += kST) mine = max(mine, s3_key(a.counts[item0 + h], h));
    if (mine) atomicMax(&best, mine);   // integers: the maximum is the same in any order
    __syncthreads();
    const uint32_t key = best;
    const bool found = key != 0u && s3_key_count(key) >= a.min_inliers;
    const int win = s3_key_h(key);
    const double qnan = __builtin_nan("");
    if (tid == 0) {
        a.winner[b] = found ? win : -1;
        a.n_inliers[b] = found ? s3_key_count(key) : 0;
    }
    if (a.stats && tid < 4) a.stats[(size_t)b * 4 + tid] = qnan;
    int32_t *inl = a.inlier + (size_t)b * a.stride;
    if (!found) {
        for (int i = tid; i < a.stride; i += kST) inl[i] = 0;
        return;
    }
    const double *o = a.models + (item0 + a.h_slot[item0 + win]) * kSModelF64;
    S3Proj p;
    load_proj(o, p);
    if (tid == 0) a.scale[b] = o[0];
    if (tid < 9) a.R[(size_t)b * 9 + tid] = o[1 + tid];
    if (tid < 3) a.T[(size_t)b * 3 + tid] = o[10 + tid];
    int32_t *ci = a.corr_index ? a.corr_index + (size_t)b * a.stride : nullptr;
    int running = 0;   // the same in every lane
    for (int base = 0; base < a.stride; base += kST) {
        const int i = base + tid;
        bool in = false;
        if (i < n) {
            double A[3], xa[2], B[3], xb[2];
            load_row(a, b, i, A, xa, B, xb);
            in = s3_inlier(p, A, xa, B, xb, a.px);
        }
        if (i < a.stride) inl[i] = in ? 1 : 0;
        int total;
        const int slot = running + vs_block_flag_scan<kST>(in, wave_n, total);
        if (in && ci) ci[slot] = i;
        running += total;
    }
}

// the correspondences i < n of an item with mask[i] != 0 (mask may be null: all of them), lane l taking l, l + 256, ...
struct MaskSrc {
    const double *__restrict__ A;
    const float2 *__restrict__ xa;
    const double *__restrict__ B;
    const float2 *__restrict__ xb;
    const int32_t *__restrict__ mask;
    int n;
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        for (int i = threadIdx.x; i < n; i += kST) {
            if (mask && mask[i] == 0) continue;
            const double p[3] = {A[3 * (size_t)i], A[3 * (size_t)i + 1], A[3 * (size_t)i + 2]};
            const double q[3] = {B[3 * (size_t)i], B[3 * (size_t)i + 1], B[3 * (size_t)i + 2]};
            const float2 oa = xa[i], ob = xb[i];
            const double x[2] = {(double)oa.x, (double)oa.y}, y[2] = {(double)ob.x, (double)ob.y};
            f(p, x, q, y);
        }
    }
};

__global__ __launch_bounds__(kST) void sim3_refine_kernel(const double *__restrict__ A, const float *__restrict__ xa,
                                                          const double *__restrict__ B, const float *__restrict__ xb,
                                                          const int32_t *__restrict__ n_in, int stride, const int32_t *__restrict__ mask,
                                                          VsK Kc, RsParams prm, double *scale_io, double *R_io, double *T_io,
                                                          double *__restrict__ stats_out) {
    __shared__ double red[(kST / 64) * kS3Sums];
    const int b = blockIdx.x;
    double K[9];
    S3Model in, out;
    in.s = scale_io[b];   // read by every lane before the first barrier, written behind the last one
#pragma unroll
    for (int k = 0; k < 9; k++) {
        K[k] = (double)Kc.v[k];
        in.R[k] = R_io[(size_t)b * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) in.t[k] = T_io[(size_t)b * 3 + k];
    MaskSrc src;
    src.A = A + (size_t)b * stride * 3;
    src.B = B + (size_t)b * stride * 3;
    src.xa = reinterpret_cast<const float2 *>(xa) + (size_t)b * stride;
    src.xb = reinterpret_cast<const float2 *>(xb) + (size_t)b * stride;
    src.mask = mask ? mask + (size_t)b * stride : nullptr;
    src.n = min(max(n_in[b], 0), stride);
    VsBlockReduce rd{red};
    double stats[4];
    const bool moved = s3_run(K, in, prm, src, rd, out, stats);
    if (threadIdx.x != 0) return;
    if (moved) {
        scale_io[b] = out.s;
#pragma unroll
        for (int k = 0; k < 9; k++) R_io[(size_t)b * 9 + k] = out.R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) T_io[(size_t)b * 3 + k] = out.t[k];
    }
    if (stats_out) {
#pragma unroll
        for (int k = 0; k < 4; k++) stats_out[(size_t)b * 4 + k] = stats[k];
    }
}

// ---- on the world
struct WorldSim3 {
    int tracks, max_frames, frames, kp_stride, map_capacity;
    const double *__restrict__ Twc;
    const float4 *__restrict__ points;
    const int32_t *__restrict__ ids, *__restrict__ fuse_to;   // fuse_to: null without a fusion
    const int32_t *__restrict__ track_a, *__restrict__ frame_a, *__restrict__ track_b, *__restrict__ frame_b;
    __device__ __forceinline__ bool valid(int item) const {
        const int ta = track_a[item], tb = track_b[item], fa = frame_a[item], fb = frame_b[item];
        return ta >= 0 && ta < tracks && tb >= 0 && tb < tracks && fa >= 0 && fa < frames && fb >= 0 && fb < frames;
    }
    __device__ __forceinline__ const double *pose(int t, int f) const { return Twc + ((size_t)t * max_frames + f) * 16; }
    // the map point behind keypoint k of frame f of track t as the world sees it (-1: none) and its row
    __device__ __forceinline__ int point(int t, int f, int k, double (&p)[3]) const {
        int id = ids[((size_t)t * max_frames + f) * kp_stride + k];
        if (id < 0 || id >= map_capacity) return -1;
        if (fuse_to) id = fuse_to[(size_t)t * map_capacity + id];
        if (id < 0 || id >= map_capacity) return -1;
        const float4 v = points[(size_t)t * map_capacity + id];
        p[0] = (double)v.x;
        p[1] = (double)v.y;
        p[2] = (double)v.z;
        return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) ? id : -1;
    }
};

// one workgroup per item: the taken matches compacted in match order
__global__ __launch_bounds__(kST) void sim3_gather_kernel(WorldSim3 w, const int2 *__restrict__ matches, const int32_t *__restrict__ n_matches,
                                                          const float2 *__restrict__ xy_a, const float2 *__restrict__ xy_b, double *__restrict__ A,
                                                          float2 *__restrict__ xa, double *__restrict__ B, float2 *__restrict__ xb,
                                                          int32_t *__restrict__ n_corr, int32_t *__restrict__ point_a,
                                                          int32_t *__restrict__ point_b) {
    __shared__ int wave_n[kST / 64];
    const int item = blockIdx.x, tid = threadIdx.x, Kp = w.kp_stride;
    const bool valid = w.valid(item);   // the same in every lane
    const int n = valid ? min(max(n_matches[item], 0), Kp) : 0;
    const size_t row0 = (size_t)item * Kp;
    int running = 0;   // the same in every lane
    for (int base = 0; base < n; base += kST) {
        const int k = base + tid;
        bool take = false;
        int ia = -1, ib = -1;
        double a[3], b[3];
        float2 oa = make_float2(0.f, 0.f), ob = oa;
        if (k < n) {
            const int2 m = matches[row0 + k];
            if (m.x >= 0 && m.x < Kp && m.y >= 0 && m.y < Kp) {
                const int ta = w.track_a[item], tb = w.track_b[item], fa = w.frame_a[item], fb = w.frame_b[item];
                double pa[3], pb[3];
                ia = w.point(ta, fa, m.x, pa);
                ib = w.point(tb, fb, m.y, pb);
                oa = xy_a[row0 + m.x];
                ob = xy_b[row0 + m.y];
                take = ia >= 0 && ib >= 0 && isfinite(oa.x) && isfinite(oa.y) && isfinite(ob.x) && isfinite(ob.y);
                if (take) {
                    s3_to_camera(w.pose(ta, fa), pa, a);
                    s3_to_camera(w.pose(tb, fb), pb, b);
                }
            }
        }
        int total;
        const size_t slot = row0 + running + vs_block_flag_scan<kST>(take, wave_n, total);
        running += total;
        if (!take) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            A[3 * slot + c] = a[c];
            B[3 * slot + c] = b[c];
        }
        xa[slot] = oa;
        xb[slot] = ob;
        if (point_a) point_a[slot] = ia;
        if (point_b) point_b[slot] = ib;
    }
    if (tid == 0) n_corr[item] = running;
}

// one lane per item: d_found and the world-to-world similarity of the found items
__global__ __launch_bounds__(kST) void sim3_world_kernel(WorldSim3 w, int items, const int32_t *__restrict__ winner, const double *__restrict__ scale,
                                                         const double *__restrict__ R, const double *__restrict__ T, int32_t *__restrict__ found,
                                                         double *__restrict__ s_w, double *__restrict__ R_w, double *__restrict__ t_w) {
    const int item = blockIdx.x * kST + threadIdx.x;
    if (item >= items) return;
    const bool f = winner[item] >= 0 && w.valid(item);
    found[item] = f ? 1 : 0;
    if (!f) return;
    S3Model m;
    m.s = scale[item];
#pragma unroll
    for (int k = 0; k < 9; k++) m.R[k] = R[(size_t)item * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) m.t[k] = T[(size_t)item * 3 + k];
    double sw, Rw[9], tw[3];
    s3_world_similarity(w.pose(w.track_a[item], w.frame_a[item]), w.pose(w.track_b[item], w.frame_b[item]), m, sw, Rw, tw);
    s_w[item] = sw;
#pragma unroll
    for (int k = 0; k < 9; k++) R_w[(size_t)item * 9 + k] = Rw[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t_w[(size_t)item * 3 + k] = tw[k];
}

constexpr int kSApplyChunk = 64;   // tracks per launch of the apply kernel, handed over by value
struct ApplyTracks {
    int32_t t[kSApplyChunk];
};

// one workgroup per listed track: every array of the world that holds coordinates, carried through X' = s R X + t
__global__ __launch_bounds__(kST) void sim3_apply_kernel(ApplyTracks track, int first, const double *__restrict__ s_in,
                                                         const double *__restrict__ R_in, const double *__restrict__ t_in,
                                                         const int32_t *__restrict__ apply, int max_frames, int frames, int kp_stride,
                                                         int map_capacity, const int32_t *__restrict__ sizes, double *Twc, float *pose,
                                                         double *scale, double *carry, const int32_t *__restrict__ carry_idx, float4 *points) {
    const int item = first + blockIdx.x, tid = threadIdx.x;
    if (apply[item] == 0) return;
    S3Model m;
    m.s = s_in[item];
#pragma unroll
    for (int k = 0; k < 9; k++) m.R[k] = R_in[(size_t)item * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) m.t[k] = t_in[(size_t)item * 3 + k];
    if (!s3_finite(m) || !(m.s > 0.0)) return;
    const int t = track.t[blockIdx.x];   // checked on the host: in range, listed once
    for (int f = tid; f < frames; f += kST) {
        const size_t fr = (size_t)t * max_frames + f;
        double out[16];
        s3_apply_pose(m, Twc + fr * 16, out);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            Twc[fr * 16 + k] = out[k];
            pose[fr * 16 + k] = (float)out[k];
        }
        scale[fr] = scale[fr] * m.s;
    }
    for (int k = tid; k < kp_stride; k += kST) {
        const size_t r = (size_t)t * kp_stride + k;
        if (carry_idx[r] < 0) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) carry[3 * r + c] = carry[3 * r + c] * m.s;
    }
    const int n = min(max(sizes[t], 0), map_capacity);
    for (int i = tid; i < n; i += kST) {
        float4 v = points[(size_t)t * map_capacity + i];
        const double X[3] = {(double)v.x, (double)v.y, (double)v.z};
        if (!(std::isfinite(X[0]) && std::isfinite(X[1]) && std::isfinite(X[2]))) continue;
        double Y[3];
        s3_apply_point(m, X, Y);
        v.x = (float)Y[0];
        v.y = (float)Y[1];
        v.z = (float)Y[2];
        points[(size_t)t * map_capacity + i] = v;
    }
}

bool params_ok(const vslam_sim3_params &p) {
    return p.hypotheses >= 64 && p.hypotheses <= 1024 && p.hypotheses % 64 == 0 && p.min_inliers >= 4 && std::isfinite(p.inlier_px) &&
           p.inlier_px > 0.0;
}

RsParams pack(const vslam_resect_params &p) {
    RsParams q;
    q.max_iterations = p.max_iterations; q.rounds = p.rounds; q.min_links = p.min_links;
    q.huber = p.huber_px; q.gate = p.gate_px;
    return q;
}
}  // namespace

extern "C" {

int vslam_sim3_params_default(vslam_sim3_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->hypotheses = 128; out->min_inliers = 8; out->inlier_px = 2.0;
    return VSLAM_OK;
}

int vslam_sim3_refine(vslam_ctx *ctx, const double *d_A, const float *d_xa, const double *d_B, const float *d_xb, const int32_t *d_n, int batch,
                      int stride, const int32_t *d_mask, const float *h_K, const vslam_resect_params *params, double *d_scale, double *d_R,
                      double *d_T, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_A && d_xa && d_B && d_xb && d_n && h_K && d_scale && d_R && d_T, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    VS_ALIGNED(ctx, d_xa, 8);   // float2 rows
    VS_ALIGNED(ctx, d_xb, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_A, d_B, d_scale, d_R, d_T, d_stats) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n, d_mask) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_resect_params p;
    vslam_resect_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, vs_resect_params_ok(p), VSLAM_ERR_INVALID);
    const VsK K = vs_pack_K(h_K);
    VsProfScope ps(ctx, "sim3_refine_kernel");
    sim3_refine_kernel<<<batch, kST, 0, ctx->stream>>>(d_A, d_xa, d_B, d_xb, d_n, stride, d_mask, K, pack(p), d_scale, d_R, d_T, d_stats);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_sim3_ransac(vslam_ctx *ctx, const double *d_A, const float *d_xa, const double *d_B, const float *d_xb, const int32_t *d_n, int batch,
                      int stride, const float *h_K, const uint32_t *d_seeds, const vslam_sim3_params *params, const vslam_resect_params *polish,
                      double *d_scale, double *d_R, double *d_T, int32_t *d_inlier, int32_t *d_corr_index, int32_t *d_n_inliers,
                      int32_t *d_winner, int32_t *d_counts, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_A && d_xa && d_B && d_xb && d_n && h_K && d_seeds && d_scale && d_R && d_T && d_inlier && d_n_inliers && d_winner,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    vslam_sim3_params p;
    vslam_sim3_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, !polish || vs_resect_params_ok(*polish), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xa, 8);   // float2 rows
    VS_ALIGNED(ctx, d_xb, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_A, d_B, d_scale, d_R, d_T, d_stats) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n, d_seeds, d_inlier, d_corr_index, d_n_inliers, d_winner, d_counts) % 4 == 0, VSLAM_ERR_INVALID);
    const size_t slots = (size_t)batch * p.hypotheses;
    int rc;
    void *ptr = nullptr;
    Sim3Args a;
    if ((rc = vs_arena_get(ctx, "sim3_models", sizeof(double) * kSModelF64 * slots, &ptr))) return rc;
    a.models = static_cast<double *>(ptr);
    if ((rc = vs_arena_get(ctx, "sim3_index", sizeof(int32_t) * (3 * slots + (size_t)batch), &ptr))) return rc;
    a.slot_h = static_cast<int32_t *>(ptr);
    a.h_slot = a.slot_h + slots;
    a.counts = a.h_slot + slots;
    a.n_valid = a.counts + slots;
    a.A = d_A; a.xa = reinterpret_cast<const float2 *>(d_xa); a.B = d_B; a.xb = reinterpret_cast<const float2 *>(d_xb);
    a.n = d_n; a.seeds = d_seeds;
    a.stride = stride; a.hypotheses = p.hypotheses; a.min_inliers = p.min_inliers;
    a.px = p.inlier_px;
    a.scale = d_scale; a.R = d_R; a.T = d_T; a.inlier = d_inlier; a.corr_index = d_corr_index; a.n_inliers = d_n_inliers;
    a.winner = d_winner; a.counts_out = d_counts; a.stats = d_stats;
    const VsK K = vs_pack_K(h_K);
    {
        VsProfScope ps(ctx, "sim3_solve_kernel");
        sim3_solve_kernel<<<batch, kST, 0, ctx->stream>>>(a, K);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "sim3_count_kernel");
        sim3_count_kernel<<<dim3(p.hypotheses / kSModels, batch), kST, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "sim3_select_kernel");
        sim3_select_kernel<<<batch, kST, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    if (!polish) return VSLAM_OK;
    return vslam_sim3_refine(ctx, d_A, d_xa, d_B, d_xb, d_n, batch, stride, d_inlier, h_K, polish, d_scale, d_R, d_T, d_stats);
}

int vslam_world_sim3(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const int32_t *d_track_a, const int32_t *d_frame_a,
                     const int32_t *d_track_b, const int32_t *d_frame_b, int items, const int32_t *d_matches, const int32_t *d_n_matches,
                     const float *d_xy_a, const float *d_xy_b, const float *h_K, const uint32_t *d_seeds, const vslam_sim3_params *params,
                     const vslam_resect_params *polish, double *d_scale, double *d_R, double *d_T, double *d_s_w, double *d_R_w, double *d_t_w,
                     int32_t *d_found, int32_t *d_n_corr, int32_t *d_n_inliers, int32_t *d_winner, int32_t *d_point_a, int32_t *d_point_b,
                     double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_track_a && d_frame_a && d_track_b && d_frame_b && d_matches && d_n_matches && d_xy_a && d_xy_b && h_K && d_seeds,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_scale && d_R && d_T && d_s_w && d_R_w && d_t_w && d_found && d_n_corr && d_n_inliers && d_winner, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, items > 0, VSLAM_ERR_INVALID);
    vslam_sim3_params p;
    vslam_sim3_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p) && (!polish || vs_resect_params_ok(*polish)), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_matches, 8);   // int2 rows
    VS_ALIGNED(ctx, d_xy_a, 8);      // float2 rows
    VS_ALIGNED(ctx, d_xy_b, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_scale, d_R, d_T, d_s_w, d_R_w, d_t_w, d_stats) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_track_a, d_frame_a, d_track_b, d_frame_b, d_n_matches, d_seeds, d_found, d_n_corr, d_n_inliers, d_winner,
                                d_point_a, d_point_b) % 4 == 0,
               VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &m))) return rc;
    const size_t rows = (size_t)items * m.kp_stride;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "sim3_world_rows", rows * (6 * sizeof(double) + 4 * sizeof(float) + sizeof(int32_t)), &ptr))) return rc;
    double *A = static_cast<double *>(ptr), *B = A + 3 * rows;
    float *xa = reinterpret_cast<float *>(B + 3 * rows), *xb = xa + 2 * rows;
    int32_t *inlier = reinterpret_cast<int32_t *>(xb + 2 * rows);
    WorldSim3 w;
    w.tracks = m.tracks; w.max_frames = m.max_frames; w.frames = m.frames; w.kp_stride = m.kp_stride; w.map_capacity = m.map_capacity;
    w.Twc = world->Twc; w.points = reinterpret_cast<const float4 *>(world->world_points); w.ids = m.d_map_point_ids;
    w.fuse_to = world->fusion ? world->fuse_to : nullptr;
    w.track_a = d_track_a; w.frame_a = d_frame_a; w.track_b = d_track_b; w.frame_b = d_frame_b;
    {
        VsProfScope ps(ctx, "sim3_gather_kernel");
        sim3_gather_kernel<<<items, kST, 0, ctx->stream>>>(w, reinterpret_cast<const int2 *>(d_matches), d_n_matches,
                                                          reinterpret_cast<const float2 *>(d_xy_a), reinterpret_cast<const float2 *>(d_xy_b), A,
                                                          reinterpret_cast<float2 *>(xa), B, reinterpret_cast<float2 *>(xb), d_n_corr, d_point_a,
                                                          d_point_b);
    }
    VS_HIP(ctx, hipGetLastError());
    if ((rc = vslam_sim3_ransac(ctx, A, xa, B, xb, d_n_corr, items, m.kp_stride, h_K, d_seeds, &p, polish, d_scale, d_R, d_T, inlier, nullptr,
                                d_n_inliers, d_winner, nullptr, d_stats)))
        return rc;
    {
        VsProfScope ps(ctx, "sim3_world_kernel");
        sim3_world_kernel<<<vs_div_up(items, kST), kST, 0, ctx->stream>>>(w, items, d_winner, d_scale, d_R, d_T, d_found, d_s_w, d_R_w, d_t_w);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_world_apply_sim3(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const int32_t *h_track, const double *d_s, const double *d_R,
                           const double *d_t, const int32_t *d_apply, int items) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && h_track && d_s && d_R && d_t && d_apply, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_world_of_map(ctx, world, map), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, items > 0 && items <= world->tracks, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_s, d_R, d_t) % 8 == 0, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_apply, 4);
    std::vector<char> seen((size_t)world->tracks, 0);
    for (int i = 0; i < items; i++) {
        const int t = h_track[i];
        VS_REQUIRE(ctx, t >= 0 && t < world->tracks && !seen[(size_t)t], VSLAM_ERR_INVALID);   // in range, listed once
        seen[(size_t)t] = 1;
    }
    vslam_map_arrays m;
    int rc;
    if ((rc = vslam_map_view(map, &m))) return rc;
    // the caller's list travels by value, 64 tracks a launch: no copy from the caller's memory is queued
    for (int first = 0; first < items; first += kSApplyChunk) {
        const int count = std::min(kSApplyChunk, items - first);
        ApplyTracks tr;
        for (int i = 0; i < kSApplyChunk; i++) tr.t[i] = i < count ? h_track[first + i] : 0;
        VsProfScope ps(ctx, "sim3_apply_kernel");
        sim3_apply_kernel<<<count, kST, 0, ctx->stream>>>(tr, first, d_s, d_R, d_t, d_apply, world->max_frames, world->frames, world->kp_stride,
                                                         world->map_capacity, m.d_sizes, world->Twc, world->pose, world->scale, world->carry,
                                                         world->carry_idx, reinterpret_cast<float4 *>(world->world_points));
        VS_HIP(ctx, hipGetLastError());
    }
    return VSLAM_OK;
}

}  // extern "C"
