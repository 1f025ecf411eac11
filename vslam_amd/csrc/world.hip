// The world frame of the resident map for gfx950: one coordinate system per track, beside the reference's map (map.hip), which
// keeps every pair's points in the last frame's camera coordinates and in the pair's own unit.  The contract is the text of
// include/vslam_amd.h ("the world frame") and its numpy restatement tests/ref_world.py; every kernel here is held to it bit for
// bit.
//
// Shape: one workgroup of 256 per track, one launch per stage for all tracks.  The step kernel forms the links' ratios as u64 keys
// in LDS (8 bytes per match slot: 64 KB at 8160 keypoints, 128 KB at VSLAM_MAX_KP, inside gfx950's 160 KB per workgroup, so
// there is no global-memory variant), finds the lower median by a radix select over them (world_select.h: eight passes of a
// 256-bin LDS histogram; integer atomics, so arrival order cannot show), chains the pose and writes the new carry: the match
// index that wins a keypoint is an atomicMax in LDS, in the space the keys no longer need, followed by the owner's write.
// Nothing is re-orthonormalised.
#include <algorithm>
#include <cmath>

#include "ctx.h"
#include "world_match.h"
#include "world_select.h"

// the contract's arithmetic is unfused f64, whatever the build's flags are
#pragma clang fp contract(off)

namespace {

constexpr int kWT = 256;   // threads of every kernel here: one workgroup per track in the step

struct WorldDev {
    int max_frames, kp_stride, min_links;
    double *Twc;
    float *pose;
    double *scale;
    int32_t *links;
    double *carry;
    int32_t *carry_idx;
    // where the step writes the new carry: the same table, or the second one of a resecting world (include/vslam_resect.h)
    double *carry_out;
    int32_t *carry_idx_out;
};

WorldDev dev_of(const vslam_world *w) {
    WorldDev d;
    d.max_frames = w->max_frames; d.kp_stride = w->kp_stride; d.min_links = w->min_links;
    d.Twc = w->Twc; d.pose = w->pose; d.scale = w->scale; d.links = w->links; d.carry = w->carry; d.carry_idx = w->carry_idx;
    d.carry_out = w->resect ? w->carry_next : w->carry;
    d.carry_idx_out = w->resect ? w->carry_idx_next : w->carry_idx;
    return d;
}

__global__ __launch_bounds__(kWT) void world_reset_kernel(WorldDev w) {
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < w.max_frames * 16; i += kWT) {
        const bool one = (i & 15) % 5 == 0;
        w.Twc[(size_t)b * w.max_frames * 16 + i] = one ? 1.0 : 0.0;
        w.pose[(size_t)b * w.max_frames * 16 + i] = one ? 1.f : 0.f;
    }
    for (int i = tid; i < w.max_frames; i += kWT) {
        w.scale[(size_t)b * w.max_frames + i] = 1.0;
        w.links[(size_t)b * w.max_frames + i] = 0;
    }
    for (int i = tid; i < w.kp_stride; i += kWT) w.carry_idx[(size_t)b * w.kp_stride + i] = -1;
    for (int i = tid; i < 3 * w.kp_stride; i += kWT) w.carry[(size_t)b * w.kp_stride * 3 + i] = 0.0;
}

// dynamic LDS: kp_stride u64 keys; after the selection the same bytes hold kp_stride int32 winners
__global__ __launch_bounds__(kWT) void world_step_kernel(WorldDev w, int fid, const int32_t *__restrict__ matches,
                                                         const int32_t *__restrict__ best, const float *__restrict__ points4d,
                                                         const float *__restrict__ Rf, const float *__restrict__ tf,
                                                         const int32_t *__restrict__ n_last, const int32_t *__restrict__ n_cur) {
    extern __shared__ unsigned long long ws_keys[];
    __shared__ uint32_t hist[kWsBins];
    __shared__ uint32_t s_links, s_rank;
    __shared__ uint64_t s_prefix;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = w.kp_stride;
    const size_t fr = (size_t)b * w.max_frames + fid;
    const double *Tp = w.Twc + (fr - 1) * 16;
    double *carry = w.carry + (size_t)b * K * 3;
    int32_t *cidx = w.carry_idx + (size_t)b * K;
    double *carry_out = w.carry_out + (size_t)b * K * 3;
    int32_t *cidx_out = w.carry_idx_out + (size_t)b * K;
    const double s_prev = w.scale[fr - 1];
    if (best[(size_t)b * 4] < 0) {   // no winner: pose and scale carried over, the carry all invalid
        if (tid < 16) {
            const double v = Tp[tid];
            w.Twc[fr * 16 + tid] = v;
            w.pose[fr * 16 + tid] = (float)v;
        }
        if (tid == 0) {
            w.scale[fr] = s_prev;
            w.links[fr] = -1;
        }
        for (int i = tid; i < K; i += kWT) cidx_out[i] = -1;
        return;
    }
    const int n = min(max(best[(size_t)b * 4 + 3], 0), K);
    const int nl = min(n_last[b], K), nc = min(n_cur[b], K);
    const int2 *M = reinterpret_cast<const int2 *>(matches) + (size_t)b * K;
    const float4 *P = reinterpret_cast<const float4 *>(points4d) + (size_t)b * K;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)Rf[(size_t)b * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = (double)tf[(size_t)b * 3 + i];
    if (tid == 0) s_links = 0;
    __syncthreads();

    // links -> keys (slot k of the LDS array belongs to match k; the value of the median does not depend on the slots)
    uint32_t mine = 0;
    for (int k = tid; k < n; k += kWT) {
        const VsWorldMatch m = vs_world_load_match(M, P, k, nl, nc, R, t);
        unsigned long long key = kWsNoKey;
        if (m.usable && cidx[m.first] >= 0) {
            const double c[3] = {carry[3 * m.first], carry[3 * m.first + 1], carry[3 * m.first + 2]};
            key = ws_link_key(c, m.X);
        }
        ws_keys[k] = key;
        mine += key != kWsNoKey ? 1u : 0u;
    }
    atomicAdd(&s_links, mine);   // a sum of integers: the order does not show
    __syncthreads();             // every read of the old carry is behind this
    const uint32_t L = s_links;

    double s = s_prev;
    if (L >= (uint32_t)w.min_links) {
        if (tid == 0) {
            s_rank = ws_rank(L);
            s_prefix = 0;
        }
        for (int pass = 0; pass < kWsPasses; pass++) {
            hist[tid] = 0;   // kWT == kWsBins
            __syncthreads();
            const uint64_t prefix = s_prefix;
            for (int k = tid; k < n; k += kWT) {
                const uint64_t key = ws_keys[k];
                if (ws_in_prefix(key, prefix, pass)) atomicAdd(&hist[ws_digit(key, pass)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t rank = s_rank;
                uint64_t pre = s_prefix;
                ws_pick(hist, pass, &rank, &pre);
                s_rank = rank;
                s_prefix = pre;
            }
            __syncthreads();
        }
        s = sqrt(ws_value(s_prefix));   // every lane reads the same key
    }

    // Twc_f = Twc_(f-1) * [R^t | -(s (R^t t))]: one entry per lane
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        double B[4];
        if (c < 3) {
            B[0] = R[3 * c]; B[1] = R[3 * c + 1]; B[2] = R[3 * c + 2]; B[3] = 0.0;
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) B[i] = -(s * ((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]));
            B[3] = 1.0;
        }
        const double v = ((Tp[4 * r] * B[0] + Tp[4 * r + 1] * B[1]) + Tp[4 * r + 2] * B[2]) + Tp[4 * r + 3] * B[3];
        w.Twc[fr * 16 + tid] = v;
        w.pose[fr * 16 + tid] = (float)v;
    }
    if (tid == 0) {
        w.scale[fr] = s;
        w.links[fr] = (int32_t)L;
    }

    // the new carry, keyed by `second`: the higher match index wins a keypoint, then the owner writes
    __syncthreads();   // the keys are done with
    int *win = reinterpret_cast<int *>(ws_keys);
    for (int i = tid; i < K; i += kWT) win[i] = -1;
    __syncthreads();
    for (int k = tid; k < n; k += kWT) {
        const VsWorldMatch m = vs_world_load_match(M, P, k, nl, nc, R, t);
        if (m.usable) atomicMax(&win[m.second], k);
    }
    __syncthreads();
    for (int k = tid; k < n; k += kWT) {
        const VsWorldMatch m = vs_world_load_match(M, P, k, nl, nc, R, t);
        if (m.usable && win[m.second] == k) {
            carry_out[3 * m.second] = s * m.Y[0];
            carry_out[3 * m.second + 1] = s * m.Y[1];
            carry_out[3 * m.second + 2] = s * m.Y[2];
        }
    }
    for (int i = tid; i < K; i += kWT) cidx_out[i] = win[i];
}

// rows [lo, hi) of a track: xf(Twc_(f-1), s_f X) rounded once, w = 1; every lane of a track reads the same Twc and s
__global__ __launch_bounds__(kWT) void world_lift_kernel(WorldDev w, int fid, const float *points, int stride,
                                                         const int32_t *__restrict__ lo, const int32_t *__restrict__ hi,
                                                         float *out) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * kWT + threadIdx.x;
    const int i0 = min(max(lo[b], 0), stride), i1 = min(max(hi[b], 0), stride);
    if (i < i0 || i >= i1) return;
    const size_t fr = (size_t)b * w.max_frames + fid;
    const double *T = w.Twc + (fr - 1) * 16;
    const double s = w.scale[fr];
    const float4 p = reinterpret_cast<const float4 *>(points)[(size_t)b * stride + i];
    const double x = s * (double)p.x, y = s * (double)p.y, z = s * (double)p.z;
    float4 o;
    o.x = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    o.y = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    o.z = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
    o.w = 1.f;
    reinterpret_cast<float4 *>(out)[(size_t)b * stride + i] = o;
}

__global__ void world_flag_kernel(int32_t *errflag) { atomicOr(errflag, 1); }

template <typename T>
int world_alloc(vslam_ctx *ctx, vslam_world *w, T **out, size_t count) {
    void *p = nullptr;
    VS_HIP(ctx, hipMalloc(&p, sizeof(T) * (count ? count : 1)));
    w->owned.push_back(p);
    *out = static_cast<T *>(p);
    return VSLAM_OK;
}

int world_step(vslam_ctx *ctx, vslam_world *w, const int32_t *matches, const int32_t *best, const float *points4d, const float *R,
               const float *t, const int32_t *n_last, const int32_t *n_cur, const float *xy_cur = nullptr, const float *h_K = nullptr) {
    int rc;
    if (w->frames >= w->max_frames) {   // no slot for this frame: nothing happens to any track
        int32_t *errflag = nullptr;
        if ((rc = vs_device_errflag(ctx, &errflag))) return rc;
        world_flag_kernel<<<1, 1, 0, ctx->stream>>>(errflag);
        VS_HIP(ctx, hipGetLastError());
        return VSLAM_OK;
    }
    const size_t lds = sizeof(unsigned long long) * (size_t)w->kp_stride;
    // static + dynamic LDS above the default limit needs the opt-in; gfx950 has 160 KB per workgroup
    if (lds > 32 * 1024 && (rc = vs_allow_dynamic_lds(ctx, world_step_kernel, "world_step", sizeof(unsigned long long) * VSLAM_MAX_KP)))
        return rc;
    {
        VsProfScope ps(ctx, "world_step_kernel");
        world_step_kernel<<<w->tracks, kWT, lds, ctx->stream>>>(dev_of(w), w->frames, matches, best, points4d, R, t, n_last, n_cur);
    }
    VS_HIP(ctx, hipGetLastError());
    if (w->resect) {   // the resection reads the old carry and the step's s0, then the two carry tables change places
        if ((rc = vs_launch_world_resect(ctx, w, w->frames, matches, best, points4d, R, t, n_last, n_cur, xy_cur, h_K))) return rc;
        std::swap(w->carry, w->carry_next);
        std::swap(w->carry_idx, w->carry_idx_next);
    }
    w->frames += 1;
    return VSLAM_OK;
}

int world_lift(vslam_ctx *ctx, vslam_world *w, int frame, const float *points, int stride, const int32_t *lo, const int32_t *hi,
               float *out) {
    VsProfScope ps(ctx, "world_lift_kernel");
    world_lift_kernel<<<dim3(vs_div_up(stride, kWT), w->tracks), kWT, 0, ctx->stream>>>(dev_of(w), frame, points, stride, lo, hi, out);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

}  // namespace

static_assert(kWT == kWsBins, "one lane per histogram bin");

int vs_world_bind(vslam_ctx *ctx, vslam_world *w, int map_capacity) {
    if (w->world_points && w->map_capacity == map_capacity) return VSLAM_OK;
    VS_REQUIRE(ctx, !w->world_points, VSLAM_ERR_INVALID);   // one map shape per world
    int rc;
    if ((rc = world_alloc(ctx, w, &w->world_points, (size_t)w->tracks * map_capacity * 4))) return rc;
    if ((rc = world_alloc(ctx, w, &w->size_before, (size_t)w->tracks))) return rc;
    w->map_capacity = map_capacity;
    VS_HIP(ctx, hipMemsetAsync(w->world_points, 0, sizeof(float) * 4 * (size_t)w->tracks * map_capacity, ctx->stream));
    VS_HIP(ctx, hipMemsetAsync(w->size_before, 0, sizeof(int32_t) * (size_t)w->tracks, ctx->stream));
    return VSLAM_OK;
}

int vs_world_before_map_step(vslam_ctx *ctx, vslam_world *w, const int32_t *sizes) {
    VS_HIP(ctx, hipMemcpyAsync(w->size_before, sizes, sizeof(int32_t) * (size_t)w->tracks, hipMemcpyDeviceToDevice, ctx->stream));
    return VSLAM_OK;
}

int vs_world_after_map_step(vslam_ctx *ctx, vslam_world *w, const int32_t *matches, const int32_t *best, const float *points4d,
                            const float *R, const float *t, const int32_t *n_last, const int32_t *n_cur, const float *map_points,
                            const int32_t *sizes, const float *xy_cur, const float *h_K) {
    const int fid = w->frames;
    int rc;
    if ((rc = world_step(ctx, w, matches, best, points4d, R, t, n_last, n_cur, xy_cur, h_K))) return rc;
    if (w->frames == fid) return VSLAM_OK;   // beyond max_frames: reported, nothing to lift
    return world_lift(ctx, w, fid, map_points, w->map_capacity, w->size_before, sizes, w->world_points);
}

extern "C" {

int vslam_world_destroy(vslam_world *world) {
    if (!world) return VSLAM_ERR_INVALID;
    if (world->ctx) {
        (void)hipSetDevice(world->ctx->device);
        (void)hipStreamSynchronize(world->ctx->stream);
    }
    for (void *p : world->owned) (void)hipFree(p);
    delete world;
    return VSLAM_OK;
}

int vslam_world_reset(vslam_ctx *ctx, vslam_world *world) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && world->ctx == ctx, VSLAM_ERR_INVALID);
    if (world->world_points)
        VS_HIP(ctx, hipMemsetAsync(world->world_points, 0, sizeof(float) * 4 * (size_t)world->tracks * world->map_capacity, ctx->stream));
    world_reset_kernel<<<world->tracks, kWT, 0, ctx->stream>>>(dev_of(world));
    VS_HIP(ctx, hipGetLastError());
    world->frames = 1;
    if (int rc = vs_world_fusion_reset(ctx, world)) return rc;
    if (world->resect_stats) return vs_world_resect_reset(ctx, world);
    return VSLAM_OK;
}

int vslam_world_create(vslam_ctx *ctx, int tracks, int max_frames, int kp_stride, int min_links, vslam_world **out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, out, VSLAM_ERR_INVALID);
    *out = nullptr;
    VS_REQUIRE(ctx, tracks > 0 && max_frames > 0 && kp_stride > 0 && min_links > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    VS_REQUIRE(ctx, (size_t)tracks * max_frames < ((size_t)1 << 26) && (size_t)tracks * kp_stride < ((size_t)1 << 28), VSLAM_ERR_CAPACITY);
    vslam_world *w = new vslam_world;
    w->ctx = ctx;
    w->tracks = tracks; w->max_frames = max_frames; w->kp_stride = kp_stride; w->min_links = min_links;
    const size_t T = tracks, Fr = max_frames, K = kp_stride;
    int rc = world_alloc(ctx, w, &w->Twc, T * Fr * 16);
    if (rc == VSLAM_OK) rc = world_alloc(ctx, w, &w->pose, T * Fr * 16);
    if (rc == VSLAM_OK) rc = world_alloc(ctx, w, &w->scale, T * Fr);
    if (rc == VSLAM_OK) rc = world_alloc(ctx, w, &w->links, T * Fr);
    if (rc == VSLAM_OK) rc = world_alloc(ctx, w, &w->carry, T * K * 3);
    if (rc == VSLAM_OK) rc = world_alloc(ctx, w, &w->carry_idx, T * K);
    if (rc == VSLAM_OK) rc = vslam_world_reset(ctx, w);
    if (rc != VSLAM_OK) {
        const std::string keep = ctx->err;
        vslam_world_destroy(w);
        ctx->err = keep;
        return rc;
    }
    *out = w;
    return VSLAM_OK;
}

int vslam_world_step(vslam_ctx *ctx, vslam_world *world, const int32_t *d_matches, const int32_t *d_best, const float *d_points4d,
                     const float *d_R, const float *d_t, const int32_t *d_n_last, const int32_t *d_n_cur) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && world->ctx == ctx, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_matches && d_best && d_points4d && d_R && d_t && d_n_last && d_n_cur, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_matches, 8);      // int2 rows
    VS_ALIGNED(ctx, d_points4d, 16);    // float4 rows
    VS_REQUIRE(ctx, vs_ptr_bits(d_best, d_R, d_t, d_n_last, d_n_cur) % 4 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, !world->resect, VSLAM_ERR_INVALID);   // a resecting world is stepped by vslam_world_step_resect
    return world_step(ctx, world, d_matches, d_best, d_points4d, d_R, d_t, d_n_last, d_n_cur);
}

int vslam_world_step_resect(vslam_ctx *ctx, vslam_world *world, const int32_t *d_matches, const int32_t *d_best,
                            const float *d_points4d, const float *d_R, const float *d_t, const int32_t *d_n_last,
                            const int32_t *d_n_cur, const float *d_xy_cur, const float *h_K) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && world->ctx == ctx, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_matches && d_best && d_points4d && d_R && d_t && d_n_last && d_n_cur && d_xy_cur && h_K, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_matches, 8);
    VS_ALIGNED(ctx, d_points4d, 16);
    VS_ALIGNED(ctx, d_xy_cur, 8);       // float2 rows
    VS_REQUIRE(ctx, vs_ptr_bits(d_best, d_R, d_t, d_n_last, d_n_cur) % 4 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, world->resect, VSLAM_ERR_INVALID);
    return world_step(ctx, world, d_matches, d_best, d_points4d, d_R, d_t, d_n_last, d_n_cur, d_xy_cur, h_K);
}

int vslam_world_set_resection(vslam_world *world, const vslam_resect_params *params) {
    if (!world || !world->ctx) return VSLAM_ERR_INVALID;
    vslam_ctx *ctx = world->ctx;
    VS_REQUIRE(ctx, world->frames == 1, VSLAM_ERR_INVALID);   // between two steps the carry of the last one is in use
    if (!params) {
        world->resect = false;
        return VSLAM_OK;
    }
    VS_REQUIRE(ctx, vs_resect_params_ok(*params), VSLAM_ERR_INVALID);
    if (!world->resect_stats) {
        const size_t T = world->tracks, K = world->kp_stride;
        int rc = world_alloc(ctx, world, &world->carry_next, T * K * 3);
        if (rc == VSLAM_OK) rc = world_alloc(ctx, world, &world->carry_idx_next, T * K);
        if (rc == VSLAM_OK) rc = world_alloc(ctx, world, &world->resect_stats, T * world->max_frames * 4);
        if (rc == VSLAM_OK) rc = vs_world_resect_reset(ctx, world);
        if (rc != VSLAM_OK) {
            world->resect_stats = nullptr;   // freed with the world
            return rc;
        }
    }
    world->resect_params = *params;
    world->resect = true;
    return VSLAM_OK;
}

int vslam_world_resection_view(vslam_world *world, double **d_stats) {
    if (!world || !d_stats) return VSLAM_ERR_INVALID;
    *d_stats = world->resect_stats;
    return VSLAM_OK;
}

int vslam_world_lift(vslam_ctx *ctx, vslam_world *world, int frame, const float *d_points, int stride, const int32_t *d_lo,
                     const int32_t *d_hi, float *d_out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && world->ctx == ctx, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_points && d_lo && d_hi && d_out && stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, frame >= 1 && frame < world->frames, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_points, 16);
    VS_ALIGNED(ctx, d_out, 16);
    VS_REQUIRE(ctx, vs_ptr_bits(d_lo, d_hi) % 4 == 0, VSLAM_ERR_INVALID);
    return world_lift(ctx, world, frame, d_points, stride, d_lo, d_hi, d_out);
}

int vslam_world_view(vslam_world *world, vslam_world_arrays *out) {
    if (!world || !out) return VSLAM_ERR_INVALID;
    out->tracks = world->tracks; out->max_frames = world->max_frames; out->kp_stride = world->kp_stride;
    out->min_links = world->min_links; out->map_capacity = world->map_capacity; out->frames = world->frames;
    out->d_Twc = world->Twc; out->d_pose = world->pose; out->d_scale = world->scale; out->d_links = world->links;
    out->d_carry = world->carry; out->d_carry_index = world->carry_idx; out->d_world_points = world->world_points;
    return VSLAM_OK;
}

int vslam_world_render(vslam_ctx *ctx, vslam_world *world, vslam_map *map, int track_lo, int track_count, const vslam_view *h_view,
                       int width, int height, int row_stride, uint8_t *d_bgr_out, float *d_depth_out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && world->ctx == ctx && map, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_depth_out) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_map_arrays a;
    const int rc = vslam_map_view(map, &a);
    if (rc != VSLAM_OK) return rc;
    VS_REQUIRE(ctx, world->world_points && a.tracks == world->tracks && a.map_capacity == world->map_capacity, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, track_lo >= 0 && track_count > 0 && track_lo <= a.tracks - track_count, VSLAM_ERR_INVALID);
    const int frames = std::min(world->frames, world->max_frames);
    return vslam_render_points(ctx, world->world_points + (size_t)track_lo * a.map_capacity * 4,
                               a.d_colors + (size_t)track_lo * a.map_capacity * 3, a.d_sizes + track_lo, track_count, a.map_capacity,
                               world->pose + (size_t)track_lo * world->max_frames * 16, frames, world->max_frames, h_view, width,
                               height, row_stride, d_bgr_out, d_depth_out);
}

}  // extern "C"
