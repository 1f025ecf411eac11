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
//   match_propose_kernel    vslam_match_points (include/vslam_pnp.h): the same proposals with visibility and the disc taken out,
//                           every point against every keypoint.
//   corr_resolve_kernel     behind either: one workgroup per item: a point has found its keypoint iff the key there is its own;
//                           ordered compaction in chunks of 256 points, the per-point outputs and the four counts.
// What decides something is search_math.h's.  No floating-point atomics, no scratch.
#include <cmath>

#include "block_scan.h"
#include "ctx.h"
#include "../../include/vslam_pnp.h"
#include "../../include/vslam_search.h"
#include "search_math.h"

#pragma clang fp contract(off)

using namespace vs_search;

namespace {
constexpr int kST = 256;                                       // lanes per workgroup
constexpr int kSPts = 512;                                     // points per workgroup of the proposals
constexpr int kSCells = kSsMaxCells * kSsMaxCells;             // 4096
constexpr int kSCellsPerLane = kSCells / kST;                  // the scan's share of a lane: 16 consecutive cells
// beside d0 (<= 256) in a proposal's second word: the point takes part (in the search: is visible), it has a candidate
constexpr int kPropPart = 1 << 16, kPropCandidate = 1 << 17;
constexpr int kMTile = 1024;                                   // keypoints per LDS tile of the match
constexpr int kMObs = 4;                                       // observation descriptors a lane of the match keeps in registers

// what both proposal kernels and the resolution read
struct CorrArgs {
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
    SsParams prm;
    unsigned long long *keys;   // [batch][kp_stride], all ones ahead of the proposals
    int2 *prop;                 // [batch][pt_stride]: (k0 or -1, d0 | flags)
    int32_t *kp_of_point, *dist;
    double *corr_points;
    float2 *corr_xy;
    int32_t *corr_point, *corr_kp, *n_corr, *stats;
};

struct SearchView {   // what only the projection needs
    const double *R, *T;
    int width, height;
};

__device__ __forceinline__ void load_desc(const uint8_t *row, uint32_t (&w)[8]) {   // a 32-byte row, 16-byte aligned
    const uint4 a = reinterpret_cast<const uint4 *>(row)[0], b = reinterpret_cast<const uint4 *>(row)[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

__global__ __launch_bounds__(kST) void search_propose_kernel(CorrArgs a, SearchView s, VsK Kc) {
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
    const SsGrid g = ss_grid(s.width, s.height, a.prm.radius);
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
        int run = vs_block_excl_scan<kST>(mine, scan_lds, total);
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
        cam.R[k] = s.R[(size_t)b * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) cam.T[k] = s.T[(size_t)b * 3 + k];
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
        const bool visible = ss_visible(K, cam, cam_ok, P.x, P.y, P.z, o0, o1, a.obs_stride, s.width, s.height, u, v);
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
        pr.y = (proposes ? (int)best.d0 : 0) | (visible ? kPropPart : 0) | (any ? kPropCandidate : 0);
        a.prop[(size_t)b * a.pt_stride + i] = pr;
        if (proposes) atomicMin(&a.keys[(size_t)b * a.kp_stride + best.k0], ss_key(best.d0, (uint32_t)i));
    }
}

// ---- vslam_match_points: every point against every keypoint.  Grid (ceil(pt_stride / 256), batch), one lane per point with up to
// four of its observation descriptors in registers (further ones are read again per keypoint); the item's keypoint descriptors
// pass through LDS in tiles of 1024 (32 KB: VSLAM_MAX_KP x 32 B would not fit), and every lane reads the same row of the tile, a
// broadcast.  The choice, the proposal rule and the keys are search_math.h's, as the search's.
__global__ __launch_bounds__(kST) void match_propose_kernel(CorrArgs a) {
    __shared__ uint4 tile[2 * kMTile];
    __shared__ uint8_t cand[kMTile];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    if (blockIdx.x * kST >= n) return;   // the whole workgroup: the resolution writes the rows from n on
    const int n_kp = min(max(a.n_kp[b], 0), a.kp_stride);
    const int32_t *taken = a.taken ? a.taken + (size_t)b * a.kp_stride : nullptr;
    const int32_t *OO = a.obs_offsets + (size_t)b * (a.pt_stride + 1);
    const uint8_t *OD = a.obs_desc + (size_t)b * a.obs_stride * VSLAM_DESC_BYTES;
    const uint4 *D = reinterpret_cast<const uint4 *>(a.desc + (size_t)b * a.kp_stride * VSLAM_DESC_BYTES);
    const int i = blockIdx.x * kST + tid;
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
        for (int j = tid; j < 2 * m; j += kST) tile[j] = D[2 * (size_t)base + j];
        for (int j = tid; j < m; j += kST) cand[j] = (taken && taken[base + j] >= 0) ? 0 : 1;
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
__global__ __launch_bounds__(kST) void corr_resolve_kernel(CorrArgs a) {
    __shared__ int scan_lds[kST / 64];
    __shared__ int counts[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    if (tid < 3) counts[tid] = 0;
    __syncthreads();
    const unsigned long long *keys = a.keys + (size_t)b * a.kp_stride;
    const float2 *XY = a.xy + (size_t)b * a.kp_stride;
    int run = 0, part = 0, with_candidate = 0, proposing = 0;
    for (int base = 0; base < a.pt_stride; base += kST) {   // ascending chunks: the compacted order is the points' order
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
        const int pos = run + vs_block_flag_scan<kST>(found, scan_lds, chunk);
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

// the threshold and the ratio of the choice, which the search and the match share
bool choice_ok(int dist_threshold, int ratio10) { return dist_threshold >= 1 && dist_threshold <= 257 && ratio10 >= 0 && ratio10 <= 10; }

bool params_ok(const vslam_search_params &p) {
    return std::isfinite(p.radius_px) && p.radius_px > 0.0 && p.radius_px <= 64.0 && choice_ok(p.dist_threshold, p.ratio10);
}

bool K_finite(const float *h_K) {
    bool ok = true;
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(h_K[k]);
    return ok;
}

// the two arena slots, the fill of the keys, the caller's proposals (propose(a) launches them) and the resolution; everything has
// been checked
template <typename Propose>
int launch_corr(vslam_ctx *ctx, CorrArgs a, int batch, const char *propose_name, Propose propose) {
    int rc;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "corr_keys", sizeof(unsigned long long) * (size_t)batch * a.kp_stride, &ptr))) return rc;
    a.keys = static_cast<unsigned long long *>(ptr);
    if ((rc = vs_arena_get(ctx, "corr_prop", sizeof(int2) * (size_t)batch * a.pt_stride, &ptr))) return rc;
    a.prop = static_cast<int2 *>(ptr);
    VS_HIP(ctx, hipMemsetAsync(a.keys, 0xFF, sizeof(unsigned long long) * (size_t)batch * a.kp_stride, ctx->stream));
    {
        VsProfScope ps(ctx, propose_name);
        propose(a);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "corr_resolve_kernel");
        corr_resolve_kernel<<<batch, kST, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int launch_search(vslam_ctx *ctx, const CorrArgs &a, const SearchView &s, int batch, const float *h_K) {
    return launch_corr(ctx, a, batch, "search_propose_kernel", [&](const CorrArgs &c) {
        search_propose_kernel<<<dim3(vs_div_up(c.pt_stride, kSPts), batch), kST, 0, ctx->stream>>>(c, s, vs_pack_K(h_K));
    });
}

WorldSearch world_search_args(vslam_world *world, int f1, double *R, double *T, double *stats) {
    WorldSearch w;
    w.max_frames = world->max_frames; w.kp_stride = world->kp_stride; w.f1 = f1;
    w.Twc = world->Twc; w.pose = world->pose; w.carry = world->carry; w.carry_idx = world->carry_idx;
    w.R = R; w.T = T; w.stats = stats;
    return w;
}
}  // namespace

bool vs_match_params_ok(const vslam_match_params &p) { return choice_ok(p.dist_threshold, p.ratio10); }

int vs_world_map_view(vslam_ctx *ctx, vslam_world *world, vslam_map *map, vslam_map_arrays *m) {
    VS_REQUIRE(ctx, vs_world_of_map(ctx, world, map), VSLAM_ERR_INVALID);
    const int rc = vslam_map_view(map, m);
    if (rc != VSLAM_OK) return rc;
    VS_REQUIRE(ctx, m->frames == world->frames, VSLAM_ERR_INVALID);
    return VSLAM_OK;
}

int vs_world_corr_begin(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                        const double *d_stats, VsWorldCorr *c) {
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &c->m))) return rc;
    VS_REQUIRE(ctx, c->m.frames >= 1, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xy_cur, 8);
    VS_ALIGNED(ctx, d_desc_cur, 16);
    VS_ALIGNED(ctx, d_stats, 8);
    const size_t T = c->m.tracks, P = c->m.map_capacity, O = c->m.obs_capacity, Kp = c->m.kp_stride;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_corr_i32", sizeof(int32_t) * T * ((P + 1) + 2 * P), &ptr))) return rc;
    c->off = static_cast<int32_t *>(ptr); c->kp_of_point = c->off + T * (P + 1); c->dist = c->kp_of_point + T * P;
    if ((rc = vs_arena_get(ctx, "world_corr_desc", T * O * VSLAM_DESC_BYTES, &ptr))) return rc;
    c->obs_desc = static_cast<uint8_t *>(ptr);
    if ((rc = vs_arena_get(ctx, "world_corr_f64", sizeof(double) * T * (16 + 3 * Kp), &ptr))) return rc;
    c->R = static_cast<double *>(ptr); c->T = c->R + T * 9; c->mark = c->T + T * 3; c->corr_points = c->mark + T * 4;
    if ((rc = vs_arena_get(ctx, "world_corr_xy", sizeof(float) * 2 * T * Kp, &ptr))) return rc;
    c->corr_xy = static_cast<float *>(ptr);
    return vs_world_csr(ctx, world, map, c->off, nullptr, nullptr, c->obs_desc);
}

int vs_world_search_writeback(vslam_ctx *ctx, vslam_world *world, int f1, double *R, double *T, double *mark) {
    world_search_writeback_kernel<<<world->tracks, kST, 0, ctx->stream>>>(world_search_args(world, f1, R, T, mark), nullptr);
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
    CorrArgs a;
    a.points = reinterpret_cast<const float4 *>(d_points); a.n_points = d_n_points; a.pt_stride = pt_stride;
    a.obs_offsets = d_obs_offsets; a.obs_desc = d_obs_desc; a.obs_stride = obs_stride;
    a.xy = reinterpret_cast<const float2 *>(d_xy); a.desc = d_desc; a.n_kp = d_n_kp; a.kp_stride = kp_stride; a.taken = d_kp_taken;
    a.prm = ss_params(p.radius_px, p.dist_threshold, p.ratio10);
    a.keys = nullptr; a.prop = nullptr;
    a.kp_of_point = d_kp_of_point; a.dist = d_dist; a.corr_points = d_corr_points; a.corr_xy = reinterpret_cast<float2 *>(d_corr_xy);
    a.corr_point = d_corr_point; a.corr_kp = d_corr_kp; a.n_corr = d_n_corr; a.stats = d_stats;
    return launch_search(ctx, a, SearchView{d_R, d_T, width, height}, batch, h_K);
}

int vslam_world_search(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                       const int32_t *d_n_cur, const float *h_K, int width, int height, const vslam_search_params *search,
                       const vslam_resect_params *resect, int32_t *d_corr_point, int32_t *d_corr_kp, int32_t *d_n_corr,
                       double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy_cur && d_desc_cur && d_n_cur && h_K && d_corr_point && d_corr_kp && d_n_corr, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_world_of_map(ctx, world, map), VSLAM_ERR_INVALID);   // ahead of the image's size, whose code is another
    VS_REQUIRE(ctx, width > 0 && height > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, width <= 16384 && height <= 16384, VSLAM_ERR_CAPACITY);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_cur, d_corr_point, d_corr_kp, d_n_corr) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_search_params p;
    vslam_search_params_default(&p);
    if (search) p = *search;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, !resect || vs_resect_params_ok(*resect), VSLAM_ERR_INVALID);
    VsWorldCorr c;   // R, T: the pose searched from, resected in place; mark: the resection's statistics
    int rc;
    if ((rc = vs_world_corr_begin(ctx, world, map, d_xy_cur, d_desc_cur, d_stats, &c))) return rc;
    const int T = c.m.tracks, Kp = c.m.kp_stride;
    const WorldSearch w = world_search_args(world, c.m.frames - 1, c.R, c.T, c.mark);
    world_search_pose_kernel<<<vs_div_up(T, kST), kST, 0, ctx->stream>>>(w, T);
    VS_HIP(ctx, hipGetLastError());
    CorrArgs a;
    a.points = reinterpret_cast<const float4 *>(world->world_points); a.n_points = static_cast<const int32_t *>(c.m.d_sizes);
    a.pt_stride = c.m.map_capacity;
    a.obs_offsets = c.off; a.obs_desc = c.obs_desc; a.obs_stride = c.m.obs_capacity;
    a.xy = reinterpret_cast<const float2 *>(d_xy_cur); a.desc = d_desc_cur; a.n_kp = d_n_cur; a.kp_stride = Kp; a.taken = nullptr;
    a.prm = ss_params(p.radius_px, p.dist_threshold, p.ratio10);
    a.keys = nullptr; a.prop = nullptr;
    a.kp_of_point = c.kp_of_point; a.dist = c.dist; a.corr_points = c.corr_points; a.corr_xy = reinterpret_cast<float2 *>(c.corr_xy);
    a.corr_point = d_corr_point; a.corr_kp = d_corr_kp; a.n_corr = d_n_corr; a.stats = nullptr;
    if ((rc = launch_search(ctx, a, SearchView{c.R, c.T, width, height}, T, h_K))) return rc;
    if (!resect) return VSLAM_OK;
    if ((rc = vslam_resect_poses(ctx, c.corr_points, c.corr_xy, d_n_corr, T, Kp, h_K, resect, c.R, c.T, c.mark))) return rc;
    world_search_writeback_kernel<<<T, kST, 0, ctx->stream>>>(w, d_stats);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
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
    VS_REQUIRE(ctx, vs_match_params_ok(p), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_points, 16);   // float4 rows
    VS_ALIGNED(ctx, d_desc, 16);     // descriptor rows move as uint4 pairs
    VS_ALIGNED(ctx, d_obs_desc, 16);
    VS_ALIGNED(ctx, d_xy, 8);        // float2 rows
    VS_ALIGNED(ctx, d_corr_xy, 8);
    VS_ALIGNED(ctx, d_corr_points, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_points, d_obs_offsets, d_n_kp, d_kp_taken, d_kp_of_point, d_dist, d_corr_point, d_corr_kp, d_n_corr,
                                d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    CorrArgs a;
    a.points = reinterpret_cast<const float4 *>(d_points); a.n_points = d_n_points; a.pt_stride = pt_stride;
    a.obs_offsets = d_obs_offsets; a.obs_desc = d_obs_desc; a.obs_stride = obs_stride;
    a.xy = reinterpret_cast<const float2 *>(d_xy); a.desc = d_desc; a.n_kp = d_n_kp; a.kp_stride = kp_stride; a.taken = d_kp_taken;
    a.prm = ss_params(1.0, p.dist_threshold, p.ratio10);   // no disc: the radius is not read
    a.keys = nullptr; a.prop = nullptr;
    a.kp_of_point = d_kp_of_point; a.dist = d_dist; a.corr_points = d_corr_points; a.corr_xy = reinterpret_cast<float2 *>(d_corr_xy);
    a.corr_point = d_corr_point; a.corr_kp = d_corr_kp; a.n_corr = d_n_corr; a.stats = d_stats;
    return launch_corr(ctx, a, batch, "match_propose_kernel", [&](const CorrArgs &c) {
        match_propose_kernel<<<dim3(vs_div_up(c.pt_stride, kST), batch), kST, 0, ctx->stream>>>(c);
    });
}

}  // extern "C"
