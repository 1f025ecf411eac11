// The view of the resident map for gfx950: what the reference shows in its Pangolin window (include/Display.h,
// src/display.cpp), as images in device memory.  The contract is the text of include/vslam_amd.h ("the view of the map") and
// its numpy restatement tests/ref_render.py; every kernel here is held to it bit for bit.
//
// Shape: a key plane [tracks][height][width] of u64 from the context's arena, set to all-ones; map points (one lane each) and
// frustum segments (one wave per segment, lanes over its samples) project in f64 and take the per-pixel minimum of
// (f32 depth bits) << 32 | order index with 64-bit integer atomics -- a minimum does not depend on arrival order, so the image
// is bitwise reproducible; a resolve pass turns keys into BGR rows and the optional depth plane.
#include <cmath>

#include "ctx.h"

// the contract's arithmetic is unfused f64, whatever the build's flags are
#pragma clang fp contract(off)

namespace {

constexpr int kRT = 256;                            // threads of the point / clear / resolve kernels
constexpr unsigned long long kEmpty = ~0ull;

struct RenderView {   // vslam_view, widened once on the host (float -> double is exact)
    double mv[12];
    double fu, fv, u0, v0, zn, zf;
    double bw, bh, bz;   // draw_box's w, h = w * h_ratio, z = w * z_ratio (the products formed in f32)
    int point_size, flags;
    uint8_t bg[3], fr[3];
};

// draw_box's segments (src/display.cpp:129-148): signs of (w, h, z) for both ends
__device__ const signed char kSegEnds[8][6] = {{0, 0, 0, 1, 1, 1},   {0, 0, 0, 1, -1, 1},  {0, 0, 0, -1, -1, 1}, {0, 0, 0, -1, 1, 1},
                                               {1, 1, 1, 1, -1, 1},  {-1, 1, 1, -1, -1, 1}, {-1, 1, 1, 1, 1, 1},  {-1, -1, 1, 1, -1, 1}};

struct Vec3 {
    double x, y, z;
};

__device__ __forceinline__ Vec3 xf(const double *M, const Vec3 &p) {
    Vec3 r;
    r.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];
    r.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
    r.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
    return r;
}

__device__ __forceinline__ double mixd(double a, double b, double t) { return a * (1.0 - t) + b * t; }

__device__ __forceinline__ bool finite3(const Vec3 &p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// points submitted for a track: its size, or what draw_points_colors' `i < size; i += 4` loop submits
__device__ __forceinline__ int submitted_points(const int32_t *__restrict__ sizes, int t, int map_stride, int flags) {
    const int n = min(max(sizes[t], 0), map_stride);
    return (flags & VSLAM_RENDER_AS_REFERENCE) ? n / 4 + ((n & 3) ? 1 : 0) : n;
}

__device__ __forceinline__ unsigned long long make_key(float depth, unsigned order) {
    return ((unsigned long long)__float_as_uint(depth) << 32) | order;
}

// `pairs` 16-byte pairs of empty keys
__global__ __launch_bounds__(kRT) void render_clear_kernel(ulonglong2 *__restrict__ keys, size_t pairs) {
    for (size_t i = (size_t)blockIdx.x * kRT + threadIdx.x; i < pairs; i += (size_t)gridDim.x * kRT) keys[i] = make_ulonglong2(kEmpty, kEmpty);
}

__global__ __launch_bounds__(kRT) void render_points_kernel(RenderView v, const float *__restrict__ points,
                                                            const int32_t *__restrict__ sizes, int map_stride, int W, int H,
                                                            unsigned long long *__restrict__ keys) {
    const int t = blockIdx.y;
    const int i = blockIdx.x * kRT + threadIdx.x;
    if (i >= submitted_points(sizes, t, map_stride, v.flags)) return;
    const float4 P = reinterpret_cast<const float4 *>(points)[(size_t)t * map_stride + i];   // the stored w is ignored
    Vec3 p;
    p.x = (double)P.x;
    p.y = (double)P.y;
    p.z = (double)P.z;
    const Vec3 e = xf(v.mv, p);
    if (!(finite3(e) && e.z >= v.zn && e.z <= v.zf)) return;
    const double pu = floor(v.fu * e.x / e.z + v.u0), pv = floor(v.fv * e.y / e.z + v.v0);
    if (!(fabs(pu) <= 1073741824.0 && fabs(pv) <= 1073741824.0)) return;   // NaN compares false
    const int px = (int)pu, py = (int)pv;
    const int lo = (v.point_size - 1) / 2, hi = v.point_size / 2;
    const int x0 = max(px - lo, 0), x1 = min(px + hi, W - 1), y0 = max(py - lo, 0), y1 = min(py + hi, H - 1);
    const unsigned long long key = make_key((float)e.z, (unsigned)i);
    unsigned long long *plane = keys + (size_t)t * W * H;
    for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++) atomicMin(&plane[(size_t)y * W + x], key);
}

// one wave per segment: every lane forms the clipped segment (uniform work), then the lanes share its samples
__global__ __launch_bounds__(64) void render_segments_kernel(RenderView v, const float *__restrict__ pose, int pose_stride,
                                                             const int32_t *__restrict__ sizes, int map_stride, int W, int H,
                                                             unsigned long long *__restrict__ keys) {
    const int t = blockIdx.y, f = blockIdx.x >> 3, s = blockIdx.x & 7;
    const unsigned order = (unsigned)submitted_points(sizes, t, map_stride, v.flags) + (unsigned)blockIdx.x;
    const float *Pm = pose + ((size_t)t * pose_stride + f) * 16;
    double M[12];
#pragma unroll
    for (int i = 0; i < 12; i++) M[i] = (double)Pm[i];
    const signed char *sg = kSegEnds[s];
    Vec3 A, B;
    A.x = (double)sg[0] * v.bw; A.y = (double)sg[1] * v.bh; A.z = (double)sg[2] * v.bz;
    B.x = (double)sg[3] * v.bw; B.y = (double)sg[4] * v.bh; B.z = (double)sg[5] * v.bz;
    const Vec3 a = xf(v.mv, xf(M, A)), b = xf(v.mv, xf(M, B));
    if (!(finite3(a) && finite3(b))) return;
    // (i) z clip, both ends from the original segment
    if ((a.z < v.zn && b.z < v.zn) || (a.z > v.zf && b.z > v.zf)) return;
    Vec3 e[2] = {a, b};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const bool nearer = e[k].z < v.zn, farther = e[k].z > v.zf;
        if (nearer || farther) {
            const double plane = nearer ? v.zn : v.zf;
            const double tt = (plane - a.z) / (b.z - a.z);
            e[k].x = mixd(a.x, b.x, tt);
            e[k].y = mixd(a.y, b.y, tt);
            e[k].z = plane;
        }
    }
    // (ii) projection
    const double Ua = v.fu * e[0].x / e[0].z + v.u0, Va = v.fv * e[0].y / e[0].z + v.v0, qa = 1.0 / e[0].z;
    const double Ub = v.fu * e[1].x / e[1].z + v.u0, Vb = v.fv * e[1].y / e[1].z + v.v0, qb = 1.0 / e[1].z;
    if (!(isfinite(Ua) && isfinite(Va) && isfinite(qa) && isfinite(Ub) && isfinite(Vb) && isfinite(qb))) return;
    // (iii) Liang-Barsky against [-0.5, W + 0.5] x [-0.5, H + 0.5]
    double s0 = 0.0, s1 = 1.0;
    const double dU = Ub - Ua, dV = Vb - Va;
    const double lp[4] = {-dU, dU, -dV, dV};
    const double lq[4] = {Ua + 0.5, ((double)W + 0.5) - Ua, Va + 0.5, ((double)H + 0.5) - Va};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (lp[k] == 0.0) {
            if (lq[k] < 0.0) return;
        } else {
            const double r = lq[k] / lp[k];
            if (lp[k] < 0.0) {
                if (r > s1) return;
                if (r > s0) s0 = r;
            } else {
                if (r < s0) return;
                if (r < s1) s1 = r;
            }
        }
    }
    const double cUa = mixd(Ua, Ub, s0), cVa = mixd(Va, Vb, s0), cqa = mixd(qa, qb, s0);
    const double cUb = mixd(Ua, Ub, s1), cVb = mixd(Va, Vb, s1), cqb = mixd(qa, qb, s1);
    // (iv) samples
    const double m = fmax(fabs(cUb - cUa), fabs(cVb - cVa));
    if (!(m <= 65536.0)) return;
    const int n = max(1, (int)ceil(m));
    unsigned long long *plane = keys + (size_t)t * W * H;
    for (int k = threadIdx.x; k <= n; k += 64) {
        const double tt = (double)k / (double)n;
        const double pu = floor(mixd(cUa, cUb, tt)), pv = floor(mixd(cVa, cVb, tt));
        if (!(pu >= 0.0 && pu < (double)W && pv >= 0.0 && pv < (double)H)) continue;
        const float depth = (float)(1.0 / mixd(cqa, cqb, tt));
        atomicMin(&plane[(size_t)(int)pv * W + (int)pu], make_key(depth, order));
    }
}

// keys -> BGR rows (+ depth): four pixels = three dwords per lane where the row's address allows, bytes otherwise (row tails,
// rows whose pitch or base is no multiple of 4); nothing past 3 * W of a row is written
__global__ __launch_bounds__(kRT) void render_resolve_kernel(RenderView v, const unsigned long long *__restrict__ keys,
                                                             const uint8_t *__restrict__ colors, const int32_t *__restrict__ sizes,
                                                             int map_stride, int W, int H, int row_stride, uint8_t *__restrict__ bgr,
                                                             float *__restrict__ depth) {
    const int t = blockIdx.z, y = blockIdx.y;
    const int x = 4 * (blockIdx.x * kRT + threadIdx.x);
    if (x >= W) return;
    const int n = submitted_points(sizes, t, map_stride, v.flags);
    const bool as_ref = (v.flags & VSLAM_RENDER_AS_REFERENCE) != 0;
    const size_t row = (size_t)t * H + y;
    const unsigned long long *krow = keys + row * W + x;
    const int cnt = min(4, W - x);
    unsigned long long k4[4] = {kEmpty, kEmpty, kEmpty, kEmpty};
    if (cnt == 4 && (W & 1) == 0) {   // the plane is 256-byte aligned and x a multiple of 4: 16-byte loads
        const ulonglong2 k01 = reinterpret_cast<const ulonglong2 *>(krow)[0], k23 = reinterpret_cast<const ulonglong2 *>(krow)[1];
        k4[0] = k01.x; k4[1] = k01.y; k4[2] = k23.x; k4[3] = k23.y;
    } else {
        for (int j = 0; j < cnt; j++) k4[j] = krow[j];
    }
    uint8_t c[12];
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned long long key = k4[j];
        uint8_t c0 = v.bg[0], c1 = v.bg[1], c2 = v.bg[2];
        d[j] = __uint_as_float(0x7F800000u);
        if (key != kEmpty) {
            const unsigned order = (unsigned)key;
            d[j] = __uint_as_float((unsigned)(key >> 32));
            if (order < (unsigned)n) {
                const uint8_t *src = colors + ((size_t)t * map_stride + order) * 3;
                c0 = src[0]; c1 = src[1]; c2 = src[2];
                if (as_ref) {   // glColor3b(stored b, g, r) as red, green, blue: 2c + 1 below 128, else 0
                    const uint8_t r = c0 < 128 ? (uint8_t)(2 * c0 + 1) : (uint8_t)0, g = c1 < 128 ? (uint8_t)(2 * c1 + 1) : (uint8_t)0;
                    const uint8_t bl = c2 < 128 ? (uint8_t)(2 * c2 + 1) : (uint8_t)0;
                    c0 = bl; c1 = g; c2 = r;
                }
            } else {
                c0 = v.fr[0]; c1 = v.fr[1]; c2 = v.fr[2];
            }
        }
        c[3 * j] = c0; c[3 * j + 1] = c1; c[3 * j + 2] = c2;
    }
    uint8_t *out = bgr + row * row_stride + (size_t)3 * x;
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
        for (int q = 0; q < 3; q++)
            o[q] = (uint32_t)c[4 * q] | ((uint32_t)c[4 * q + 1] << 8) | ((uint32_t)c[4 * q + 2] << 16) | ((uint32_t)c[4 * q + 3] << 24);
    } else {
        for (int j = 0; j < 3 * cnt; j++) out[j] = c[j];
    }
    if (depth) {
        float *drow = depth + row * W + x;
        for (int j = 0; j < cnt; j++) drow[j] = d[j];
    }
}

int render_launch(vslam_ctx *ctx, const float *points, const uint8_t *colors, const int32_t *sizes, int tracks, int map_stride,
                  const float *pose, int frames, int pose_stride, const vslam_view *hv, int W, int H, int row_stride, uint8_t *bgr,
                  float *depth) {
    VS_REQUIRE(ctx, points && colors && sizes && hv && bgr, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, tracks > 0 && map_stride > 0 && W > 0 && H > 0 && frames >= 0 && pose_stride >= frames, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, (long long)row_stride >= 3ll * W, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, hv->point_size >= 1 && hv->point_size <= 15, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, std::isfinite(hv->z_near) && hv->z_near > 0.f && hv->z_far >= hv->z_near, VSLAM_ERR_INVALID);
    const bool frusta = (hv->flags & VSLAM_RENDER_FRUSTA) && frames > 0;
    VS_REQUIRE(ctx, !frusta || pose, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, W <= 16384 && H <= 16384 && tracks <= 65535 && frames <= (1 << 20), VSLAM_ERR_CAPACITY);
    RenderView v;
    for (int i = 0; i < 12; i++) v.mv[i] = (double)hv->mv[i];
    v.fu = hv->fu; v.fv = hv->fv; v.u0 = hv->u0; v.v0 = hv->v0; v.zn = hv->z_near; v.zf = hv->z_far;
    const float bh = hv->box_w * hv->box_h_ratio, bz = hv->box_w * hv->box_z_ratio;   // float h = w * h_ratio (src/display.cpp:119)
    v.bw = hv->box_w; v.bh = bh; v.bz = bz;
    v.point_size = hv->point_size; v.flags = hv->flags;
    for (int i = 0; i < 3; i++) {
        v.bg[i] = hv->background_bgr[i];
        v.fr[i] = hv->frustum_bgr[i];
    }
    const size_t px = (size_t)tracks * W * H;
    unsigned long long *keys = nullptr;
    int rc;
    if ((rc = vs_arena_get(ctx, "render.keys", sizeof(unsigned long long) * (px + 1), (void **)&keys))) return rc;
    {
        VsProfScope ps(ctx, "render_clear_kernel");
        const size_t pairs = (px + 1) / 2;
        const int blocks = (int)std::min<size_t>((pairs + kRT - 1) / kRT, 16384);
        render_clear_kernel<<<blocks, kRT, 0, ctx->stream>>>(reinterpret_cast<ulonglong2 *>(keys), pairs);
    }
    {
        VsProfScope ps(ctx, "render_points_kernel");
        render_points_kernel<<<dim3(vs_div_up(map_stride, kRT), tracks), kRT, 0, ctx->stream>>>(v, points, sizes, map_stride, W, H, keys);
    }
    if (frusta) {
        VsProfScope ps(ctx, "render_segments_kernel");
        render_segments_kernel<<<dim3(8 * frames, tracks), 64, 0, ctx->stream>>>(v, pose, pose_stride, sizes, map_stride, W, H, keys);
    }
    {
        VsProfScope ps(ctx, "render_resolve_kernel");
        render_resolve_kernel<<<dim3(vs_div_up(vs_div_up(W, 4), kRT), H, tracks), kRT, 0, ctx->stream>>>(v, keys, colors, sizes, map_stride,
                                                                                                     W, H, row_stride, bgr, depth);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

void normalize3(double v[3]) {
    const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int i = 0; i < 3; i++) v[i] = v[i] / len;
}

}  // namespace

extern "C" {

int vslam_view_look_at(const double eye[3], const double target[3], const double up[3], float mv_out[16]) {
    if (!eye || !target || !up || !mv_out) return VSLAM_ERR_INVALID;
    double f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]}, r[3], d[3];
    normalize3(f);
    cross3(f, up, r);
    normalize3(r);
    cross3(f, r, d);
    const double *R[3] = {r, d, f};
    float mv[16] = {0};
    for (int i = 0; i < 3; i++) {
        const double tr = -((R[i][0] * eye[0] + R[i][1] * eye[1]) + R[i][2] * eye[2]);
        if (!(std::isfinite(R[i][0]) && std::isfinite(R[i][1]) && std::isfinite(R[i][2]) && std::isfinite(tr))) return VSLAM_ERR_DEGENERATE;
        for (int j = 0; j < 3; j++) mv[4 * i + j] = (float)R[i][j];
        mv[4 * i + 3] = (float)tr;
    }
    mv[15] = 1.f;
    for (int i = 0; i < 16; i++) mv_out[i] = mv[i];
    return VSLAM_OK;
}

int vslam_view_default(int width, int height, vslam_view *out) {
    if (!out || width <= 0 || height <= 0) return VSLAM_ERR_INVALID;
    vslam_view v = {};
    const double eye[3] = {-2, 2, -2}, target[3] = {0, 0, 0}, up[3] = {0, 1, 0};   // pangolin::ModelViewLookAt, src/display.cpp:26
    const int rc = vslam_view_look_at(eye, target, up, v.mv);
    if (rc != VSLAM_OK) return rc;
    v.fu = v.fv = 420.f;                                                           // pangolin::ProjectionMatrix, src/display.cpp:25
    v.u0 = (float)(width / 2);
    v.v0 = (float)(height / 2);
    v.z_near = 0.2f;
    v.z_far = 10000.f;
    v.point_size = 1;
    v.flags = VSLAM_RENDER_FRUSTA;
    v.box_w = 1.0f; v.box_h_ratio = 0.75f; v.box_z_ratio = 0.6f;                    // include/Display.h:34
    v.frustum_bgr[0] = 255;                                                        // glColor3f(0, 0, 1), src/display.cpp:52
    *out = v;
    return VSLAM_OK;
}

int vslam_render_points(vslam_ctx *ctx, const float *d_points, const uint8_t *d_colors, const int32_t *d_sizes, int tracks,
                        int map_stride, const float *d_pose, int frames, int pose_stride, const vslam_view *h_view, int width,
                        int height, int row_stride, uint8_t *d_bgr_out, float *d_depth_out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    // float4 rows; the colours and the image are read and written by bytes (a lane's 12 bytes as dwords only where they are aligned)
    VS_ALIGNED(ctx, d_points, 16);
    VS_REQUIRE(ctx, vs_ptr_bits(d_sizes, d_pose, d_depth_out) % 4 == 0, VSLAM_ERR_INVALID);
    return render_launch(ctx, d_points, d_colors, d_sizes, tracks, map_stride, d_pose, frames, pose_stride, h_view, width, height,
                         row_stride, d_bgr_out, d_depth_out);
}

int vslam_map_render(vslam_ctx *ctx, vslam_map *map, int track_lo, int track_count, const vslam_view *h_view, int width,
                     int height, int row_stride, uint8_t *d_bgr_out, float *d_depth_out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, map, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_depth_out) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_map_arrays a;
    const int rc = vslam_map_view(map, &a);
    if (rc != VSLAM_OK) return rc;
    VS_REQUIRE(ctx, track_lo >= 0 && track_count > 0 && track_lo <= a.tracks - track_count, VSLAM_ERR_INVALID);
    const int frames = std::min(a.frames, a.max_frames);
    return render_launch(ctx, a.d_points + (size_t)track_lo * a.map_capacity * 4, a.d_colors + (size_t)track_lo * a.map_capacity * 3,
                         a.d_sizes + track_lo, track_count, a.map_capacity, a.d_pose + (size_t)track_lo * a.max_frames * 16, frames,
                         a.max_frames, h_view, width, height, row_stride, d_bgr_out, d_depth_out);
}

}  // extern "C"
