// Search by projection (include/vslam_search.h): a track's points projected into a frame with a given pose, the best keypoint of
// each by descriptor distance inside a pixel window, the ratio test, and an order-free one-to-one resolution, for a batch of
// independent items (vslam_search_projection) and for every track of a world attached to a map (vslam_world_search).
//   search_propose_kernel   grid (ceil(pt_stride / 512), batch).  Every workgroup bins the item's keypoints into a uniform grid in
//                           LDS (a counting sort: integer atomics for the counts, a scan, uint16 indices filled per cell), then
//                           one lane per point projects it, walks the cells under its window and takes the Hamming minima over
//                           the point's observations.  A proposing point writes (k0, d0) and takes atomicMin on the 64-bit key
//                           d0 << 32 | i of its keypoint (render.hip is the precedent for an order-free 64-bit minimum).  The
//                           fill order inside a cell differs from run to run; the choice is a minimum over (d, k), so it does
//                           not matter.
//   search_resolve_kernel   one workgroup per item: a point has found its keypoint iff the key there is its own; ordered
//                           compaction in chunks of 256 points, the per-point outputs and the four counts.
// What decides something is search_math.h's.  No floating-point atomics, no scratch.
#include <cmath>

#include "ctx.h"
#include "../../include/vslam_search.h"
#include "search_math.h"

#pragma clang fp contract(off)

using namespace vs_search;

namespace {
constexpr int kST = 256;                                       // lanes per workgroup
constexpr int kSPts = 512;                                     // points per workgroup of the proposals
constexpr int kSCells = kSsMaxCells * kSsMaxCells;             // 4096
constexpr int kSCellsPerLane = kSCells / kST;                  // the scan's share of a lane: 16 consecutive cells
constexpr int kPropVisible = 1 << 16, kPropCandidate = 1 << 17;   // beside d0 (<= 256) in a proposal's second word

struct SearchArgs {
    const float4 *points;
    const int32_t *n_points;
    int pt_stride;
    const int32_t *obs_offsets;
    const uint8_t *obs_desc;
    int obs_stride;
    const double *R, *T;
    int width, height;
    const float2 *xy;
    const uint8_t *desc;
    const int32_t *n_kp;
    int kp_stride;
    const int32_t *taken;
    SsParams prm;
    unsigned long long *keys;   // [batch][kp_stride], all ones ahead of the proposals
    int2 *prop;                 // [batch][pt_stride]: (k0 or -1, d0 | flags)
    int32_t *kp_of_point, *dist;
    double *corr_points;
    float2 *corr_xy;
    int32_t *corr_point, *corr_kp, *n_corr, *stats;
};

// exclusive prefix of `v` over the workgroup (kST lanes, wave64); every lane calls it.  lds: kST / 64 words.
__device__ __forceinline__ int block_excl_scan(int v, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kST / 64; w++) {
        const int s = lds[w];
        if (w < wv) base += s;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

__device__ __forceinline__ void load_desc(const uint8_t *row, uint32_t (&w)[8]) {   // a 32-byte row, 16-byte aligned
    const uint4 a = reinterpret_cast<const uint4 *>(row)[0], b = reinterpret_cast<const uint4 *>(row)[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

__global__ __launch_bounds__(kST) void search_propose_kernel(SearchArgs a, VsK Kc) {
    __shared__ uint32_t cell_end[kSCells];        // counts, then starts, then (behind the fill) the end of every cell
    __shared__ uint16_t cell_kp[VSLAM_MAX_KP];    // keypoint indices, cell by cell
    __shared__ int scan_lds[kST / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    const int first = blockIdx.x * kSPts;
    if (first >= n) return;   // the whole workgroup: the resolution writes the rows from n on
    const int n_kp = min(max(a.n_kp[b], 0), a.kp_stride);
    const float2 *XY = a.xy + (size_t)b * a.kp_stride;
    const int32_t *taken = a.taken ? a.taken + (size_t)b * a.kp_stride : nullptr;
    const SsGrid g = ss_grid(a.width, a.height, a.prm.radius);
    const int cells = g.nx * g.ny;

    // ---- the grid: count, scan, fill
    for (int c = tid; c < cells; c += kST) cell_end[c] = 0;
    __syncthreads();
    auto cell_of = [&](int k) -> int {   // -1: no candidate of any point
        if (taken && taken[k] >= 0) return -1;
        const float2 p = XY[k];
        if (!(isfinite(p.x) && isfinite(p.y))) return -1;
        return ss_cell((double)p.y, g.inv_c, g.ny) * g.nx + ss_cell((double)p.x, g.inv_c, g.nx);
    };
    for (int k = tid; k < n_kp; k += kST) {
        const int c = cell_of(k);
        if (c >= 0) atomicAdd(&cell_end[c], 1u);
    }
    __syncthreads();
    {
        const int c0 = tid * kSCellsPerLane;
        int mine = 0;
#pragma unroll
        for (int j = 0; j < kSCellsPerLane; j++) mine += c0 + j < cells ? (int)cell_end[c0 + j] : 0;
        int total;
        int run = block_excl_scan(mine, scan_lds, total);
#pragma unroll
        for (int j = 0; j < kSCellsPerLane; j++) {
            if (c0 + j < cells) {
                const int cnt = (int)cell_end[c0 + j];
                cell_end[c0 + j] = (uint32_t)run;
                run += cnt;
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < n_kp; k += kST) {
        const int c = cell_of(k);
        if (c >= 0) cell_kp[atomicAdd(&cell_end[c], 1u)] = (uint16_t)k;   // at most n_kp <= VSLAM_MAX_KP entries in all
    }
    __syncthreads();

    // ---- the points: one lane each
    double K[9];
    LmCam cam;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        K[k] = (double)Kc.v[k];
        cam.R[k] = a.R[(size_t)b * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) cam.T[k] = a.T[(size_t)b * 3 + k];
    const bool cam_ok = vs_lm::lm_finite(cam);
    const int32_t *OO = a.obs_offsets + (size_t)b * (a.pt_stride + 1);
    const uint8_t *OD = a.obs_desc + (size_t)b * a.obs_stride * VSLAM_DESC_BYTES;
    const uint8_t *D = a.desc + (size_t)b * a.kp_stride * VSLAM_DESC_BYTES;
    const double reach = a.prm.radius + kSsMargin;
    for (int p = tid; p < kSPts; p += kST) {
        const int i = first + p;
        if (i >= n) break;
        const float4 P = a.points[(size_t)b * a.pt_stride + i];
        const int o0 = OO[i], o1 = OO[i + 1];
        double u, v;
        const bool visible = ss_visible(K, cam, cam_ok, P.x, P.y, P.z, o0, o1, a.obs_stride, a.width, a.height, u, v);
        SsBest best;
        bool any = false;
        if (visible) {
            const int cx0 = ss_cell(u - reach, g.inv_c, g.nx), cx1 = ss_cell(u + reach, g.inv_c, g.nx);
            const int cy0 = ss_cell(v - reach, g.inv_c, g.ny), cy1 = ss_cell(v + reach, g.inv_c, g.ny);
            for (int cy = cy0; cy <= cy1; cy++) {   // the cells cx0 .. cx1 of a row lie side by side in cell_kp
                const int lo = cy * g.nx + cx0, hi = cy * g.nx + cx1;
                const int e = (int)cell_end[hi];
                for (int j = lo > 0 ? (int)cell_end[lo - 1] : 0; j < e; j++) {
                    const int k = cell_kp[j];
                    const float2 q = XY[k];
                    if (!ss_in_disc(q.x, q.y, u, v, a.prm.r2)) continue;
                    any = true;
                    uint32_t dk[8], dobs[8];
                    load_desc(D + (size_t)k * VSLAM_DESC_BYTES, dk);
                    uint32_t d = kSsNone;
                    for (int o = o0; o < o1; o++) {
                        load_desc(OD + (size_t)o * VSLAM_DESC_BYTES, dobs);
                        const uint32_t cur = ss_ham256(dk, dobs);
                        d = cur < d ? cur : d;
                    }
                    ss_offer(best, d, (uint32_t)k);
                }
            }
        }
        const bool proposes = visible && ss_proposes(best, a.prm);
        int2 pr;
        pr.x = proposes ? (int)best.k0 : -1;
        pr.y = (proposes ? (int)best.d0 : 0) | (visible ? kPropVisible : 0) | (any ? kPropCandidate : 0);
        a.prop[(size_t)b * a.pt_stride + i] = pr;
        if (proposes) atomicMin(&a.keys[(size_t)b * a.kp_stride + best.k0], ss_key(best.d0, (uint32_t)i));
    }
}

__global__ __launch_bounds__(kST) void search_resolve_kernel(SearchArgs a) {
    __shared__ int scan_lds[kST / 64];
    __shared__ int counts[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    if (tid < 3) counts[tid] = 0;
    __syncthreads();
    const unsigned long long *keys = a.keys + (size_t)b * a.kp_stride;
    const float2 *XY = a.xy + (size_t)b * a.kp_stride;
    int run = 0, visible = 0, with_candidate = 0, proposing = 0;
    for (int base = 0; base < a.pt_stride; base += kST) {   // ascending chunks: the compacted order is the points' order
        const int i = base + tid;
        int k0 = -1, d0 = -1;
        bool found = false;
        if (i < n) {
            const int2 pr = a.prop[(size_t)b * a.pt_stride + i];
            visible += (pr.y & kPropVisible) ? 1 : 0;
            with_candidate += (pr.y & kPropCandidate) ? 1 : 0;
            if (pr.x >= 0) {
                proposing++;
                k0 = pr.x;
                d0 = pr.y & 0xFFFF;
                found = keys[k0] == ss_key((uint32_t)d0, (uint32_t)i);
            }
        }
        int chunk;
        const int pos = run + block_excl_scan(found ? 1 : 0, scan_lds, chunk);
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
    atomicAdd(&counts[0], visible);
    atomicAdd(&counts[1], with_candidate);
    atomicAdd(&counts[2], proposing);
    __syncthreads();
    if (tid < 3) a.stats[(size_t)b * 4 + tid] = counts[tid];
    if (tid == 3) a.stats[(size_t)b * 4 + 3] = run;
}

// ---- on the world (vslam_world_search)
struct WorldSearch {
    int max_frames, kp_stride, f1;
    double *Twc;
    float *pose;
    double *carry;
    const int32_t *carry_idx;
    double *R, *T, *stats;   // [tracks][9], [tracks][3], [tracks][4]: the pose searched from, resected in place
};

// the last frame's world -> camera pose of every track, from its camera -> world matrix
__global__ __launch_bounds__(kST) void world_search_pose_kernel(WorldSearch w, int tracks) {
    const int b = blockIdx.x * kST + threadIdx.x;
    if (b >= tracks) return;
    const double *M = w.Twc + ((size_t)b * w.max_frames + w.f1) * 16;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) w.R[(size_t)b * 9 + 3 * r + c] = M[4 * c + r];
        w.T[(size_t)b * 3 + r] = -((M[r] * M[3] + M[4 + r] * M[7]) + M[8 + r] * M[11]);
    }
}

// one workgroup per track, behind the resection: where it moved the item (its statistics are numbers), d_Twc / d_pose of the last
// frame and the latest carry re-expressed in the moved camera
__global__ __launch_bounds__(kST) void world_search_writeback_kernel(WorldSearch w, double *__restrict__ stats_out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (stats_out && tid < 4) stats_out[(size_t)b * 4 + tid] = w.stats[(size_t)b * 4 + tid];
    const double accepted = w.stats[(size_t)b * 4 + 3];
    if (!(accepted == accepted)) return;   // NaN: left alone
    double *M = w.Twc + ((size_t)b * w.max_frames + w.f1) * 16;
    double old[12];   // the frame's pose before it is written: read by every lane, written behind the barrier
#pragma unroll
    for (int k = 0; k < 12; k++) old[k] = M[k];
    __syncthreads();
    const double *R = w.R + (size_t)b * 9, *T = w.T + (size_t)b * 3;
    if (tid == 0) {
        float *Mf = w.pose + ((size_t)b * w.max_frames + w.f1) * 16;
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
    for (int k = tid; k < w.kp_stride; k += kST) {
        if (w.carry_idx[(size_t)b * w.kp_stride + k] < 0) continue;
        double *c = w.carry + ((size_t)b * w.kp_stride + k) * 3;
        double wv[3], out[3];
#pragma unroll
        for (int r = 0; r < 3; r++) wv[r] = ((old[4 * r] * c[0] + old[4 * r + 1] * c[1]) + old[4 * r + 2] * c[2]) + old[4 * r + 3];
#pragma unroll
        for (int r = 0; r < 3; r++) out[r] = ((R[3 * r] * wv[0] + R[3 * r + 1] * wv[1]) + R[3 * r + 2] * wv[2]) + T[r];
#pragma unroll
        for (int r = 0; r < 3; r++) c[r] = out[r];
    }
}

bool params_ok(const vslam_search_params &p) {
    return std::isfinite(p.radius_px) && p.radius_px > 0.0 && p.radius_px <= 64.0 && p.dist_threshold >= 1 && p.dist_threshold <= 257 &&
           p.ratio10 >= 0 && p.ratio10 <= 10;
}

bool K_finite(const float *h_K) {
    bool ok = true;
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(h_K[k]);
    return ok;
}

// the fill of the keys and the two launches; everything has been checked
int launch_search(vslam_ctx *ctx, SearchArgs a, int batch, const float *h_K) {
    int rc;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "search_keys", sizeof(unsigned long long) * (size_t)batch * a.kp_stride, &ptr))) return rc;
    a.keys = static_cast<unsigned long long *>(ptr);
    if ((rc = vs_arena_get(ctx, "search_prop", sizeof(int2) * (size_t)batch * a.pt_stride, &ptr))) return rc;
    a.prop = static_cast<int2 *>(ptr);
    VS_HIP(ctx, hipMemsetAsync(a.keys, 0xFF, sizeof(unsigned long long) * (size_t)batch * a.kp_stride, ctx->stream));
    {
        VsProfScope ps(ctx, "search_propose_kernel");
        search_propose_kernel<<<dim3(vs_div_up(a.pt_stride, kSPts), batch), kST, 0, ctx->stream>>>(a, vs_pack_K(h_K));
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "search_resolve_kernel");
        search_resolve_kernel<<<batch, kST, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}
}  // namespace

vslam_world *vs_map_world(vslam_map *map);   // map.hip

// vslam_world_search's write-back for another caller (pnp.hip, vslam_world_relocalise): frame f1 of every track whose mark[4 b + 3]
// is a number gets (R, T) [tracks][9] / [tracks][3] written as d_Twc / d_pose and the latest carry re-expressed
int vs_world_search_writeback(vslam_ctx *ctx, vslam_world *world, int f1, double *R, double *T, double *mark) {
    WorldSearch w;
    w.max_frames = world->max_frames; w.kp_stride = world->kp_stride; w.f1 = f1;
    w.Twc = world->Twc; w.pose = world->pose; w.carry = world->carry; w.carry_idx = world->carry_idx;
    w.R = R; w.T = T; w.stats = mark;
    world_search_writeback_kernel<<<world->tracks, kST, 0, ctx->stream>>>(w, nullptr);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

extern "C" {

int vslam_search_params_default(vslam_search_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->radius_px = 8.0; out->dist_threshold = 64; out->ratio10 = 8;
    return VSLAM_OK;
}

int vslam_search_projection(vslam_ctx *ctx, const float *d_points, const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets,
                            const uint8_t *d_obs_desc, int obs_stride, const double *d_R, const double *d_T, const float *h_K, int width,
                            int height, const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp, int kp_stride,
                            const int32_t *d_kp_taken, int batch, const vslam_search_params *params, int32_t *d_kp_of_point,
                            int32_t *d_dist, double *d_corr_points, float *d_corr_xy, int32_t *d_corr_point, int32_t *d_corr_kp,
                            int32_t *d_n_corr, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_points && d_n_points && d_obs_offsets && d_obs_desc && d_R && d_T && h_K && d_xy && d_desc && d_n_kp, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_kp_of_point && d_dist && d_corr_points && d_corr_xy && d_n_corr, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && pt_stride > 0 && obs_stride > 0 && kp_stride > 0 && width > 0 && height > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP && width <= 16384 && height <= 16384, VSLAM_ERR_CAPACITY);
    vslam_search_params p;
    vslam_search_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_points, 16);   // float4 rows
    VS_ALIGNED(ctx, d_desc, 16);     // descriptor rows move as uint4 pairs
    VS_ALIGNED(ctx, d_obs_desc, 16);
    VS_ALIGNED(ctx, d_xy, 8);        // float2 rows
    VS_ALIGNED(ctx, d_corr_xy, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_R, d_T, d_corr_points) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_points, d_obs_offsets, d_n_kp, d_kp_taken, d_kp_of_point, d_dist, d_corr_point, d_corr_kp, d_n_corr,
                                d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    SearchArgs a;
    a.points = reinterpret_cast<const float4 *>(d_points); a.n_points = d_n_points; a.pt_stride = pt_stride;
    a.obs_offsets = d_obs_offsets; a.obs_desc = d_obs_desc; a.obs_stride = obs_stride;
    a.R = d_R; a.T = d_T; a.width = width; a.height = height;
    a.xy = reinterpret_cast<const float2 *>(d_xy); a.desc = d_desc; a.n_kp = d_n_kp; a.kp_stride = kp_stride; a.taken = d_kp_taken;
    a.prm = ss_params(p.radius_px, p.dist_threshold, p.ratio10);
    a.keys = nullptr; a.prop = nullptr;
    a.kp_of_point = d_kp_of_point; a.dist = d_dist; a.corr_points = d_corr_points; a.corr_xy = reinterpret_cast<float2 *>(d_corr_xy);
    a.corr_point = d_corr_point; a.corr_kp = d_corr_kp; a.n_corr = d_n_corr; a.stats = d_stats;
    return launch_search(ctx, a, batch, h_K);
}

int vslam_world_search(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                       const int32_t *d_n_cur, const float *h_K, int width, int height, const vslam_search_params *search,
                       const vslam_resect_params *resect, int32_t *d_corr_point, int32_t *d_corr_kp, int32_t *d_n_corr,
                       double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy_cur && d_desc_cur && d_n_cur && h_K && d_corr_point && d_corr_kp && d_n_corr, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, world->ctx == ctx && vs_map_world(map) == world && world->world_points, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, width > 0 && height > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, width <= 16384 && height <= 16384, VSLAM_ERR_CAPACITY);
    vslam_map_arrays m;
    int rc = vslam_map_view(map, &m);
    if (rc != VSLAM_OK) return rc;
    VS_REQUIRE(ctx, m.frames == world->frames && m.frames >= 1, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xy_cur, 8);
    VS_ALIGNED(ctx, d_desc_cur, 16);
    VS_ALIGNED(ctx, d_stats, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_cur, d_corr_point, d_corr_kp, d_n_corr) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_search_params p;
    vslam_search_params_default(&p);
    if (search) p = *search;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, !resect || vs_resect_params_ok(*resect), VSLAM_ERR_INVALID);
    const int T = m.tracks, P = m.map_capacity, O = m.obs_capacity, Kp = m.kp_stride;
    // workspace: the map's CSR and its descriptors, the pose, the per-point outputs and the correspondences' values
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_search_i32", sizeof(int32_t) * (size_t)T * ((size_t)(P + 1) + 2 * (size_t)P), &ptr))) return rc;
    int32_t *off = static_cast<int32_t *>(ptr), *kp_of_point = off + (size_t)T * (P + 1), *dist = kp_of_point + (size_t)T * P;
    if ((rc = vs_arena_get(ctx, "world_search_desc", (size_t)T * O * VSLAM_DESC_BYTES, &ptr))) return rc;
    uint8_t *obs_desc = static_cast<uint8_t *>(ptr);
    if ((rc = vs_arena_get(ctx, "world_search_f64", sizeof(double) * (size_t)T * (16 + 3 * (size_t)Kp), &ptr))) return rc;
    double *dp = static_cast<double *>(ptr);
    if ((rc = vs_arena_get(ctx, "world_search_xy", sizeof(float) * 2 * (size_t)T * Kp, &ptr))) return rc;
    float *corr_xy = static_cast<float *>(ptr);
    WorldSearch w;
    w.max_frames = m.max_frames; w.kp_stride = Kp; w.f1 = m.frames - 1;
    w.Twc = world->Twc; w.pose = world->pose; w.carry = world->carry; w.carry_idx = world->carry_idx;
    w.R = dp; w.T = w.R + (size_t)T * 9; w.stats = w.T + (size_t)T * 3;
    double *corr_points = w.stats + (size_t)T * 4;
    if ((rc = vslam_map_observation_descriptors(ctx, map, off, obs_desc))) return rc;
    world_search_pose_kernel<<<vs_div_up(T, kST), kST, 0, ctx->stream>>>(w, T);
    VS_HIP(ctx, hipGetLastError());
    SearchArgs a;
    a.points = reinterpret_cast<const float4 *>(world->world_points); a.n_points = static_cast<const int32_t *>(m.d_sizes); a.pt_stride = P;
    a.obs_offsets = off; a.obs_desc = obs_desc; a.obs_stride = O;
    a.R = w.R; a.T = w.T; a.width = width; a.height = height;
    a.xy = reinterpret_cast<const float2 *>(d_xy_cur); a.desc = d_desc_cur; a.n_kp = d_n_cur; a.kp_stride = Kp; a.taken = nullptr;
    a.prm = ss_params(p.radius_px, p.dist_threshold, p.ratio10);
    a.keys = nullptr; a.prop = nullptr;
    a.kp_of_point = kp_of_point; a.dist = dist; a.corr_points = corr_points; a.corr_xy = reinterpret_cast<float2 *>(corr_xy);
    a.corr_point = d_corr_point; a.corr_kp = d_corr_kp; a.n_corr = d_n_corr; a.stats = nullptr;
    if ((rc = launch_search(ctx, a, T, h_K))) return rc;
    if (!resect) return VSLAM_OK;
    if ((rc = vslam_resect_poses(ctx, corr_points, corr_xy, d_n_corr, T, Kp, h_K, resect, w.R, w.T, w.stats))) return rc;
    world_search_writeback_kernel<<<T, kST, 0, ctx->stream>>>(w, d_stats);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

}  // extern "C"
