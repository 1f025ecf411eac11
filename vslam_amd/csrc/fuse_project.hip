// Geometric fusing (include/vslam_fuse_project.h): every point of an item searched by projection in every camera of the item that
// does not see it yet, one-to-one per keypoint, with the point that already holds the keypoint, for a batch of independent items.
//   fuse_project_holders_kernel   grid (batch): one workgroup per item.  The CSR is checked (a broken one: the item's flag is 0 and
//                                 every later kernel leaves the item empty); then the smallest point index of every (cam, kp) cell
//                                 by an integer atomicMin over the valid entries.
//   fuse_project_propose_kernel   grid (ceil(pt_stride / 1024), cam_stride, batch): a workgroup takes one camera and 1024 points.  It
//                                 bins the camera's keypoints into the search's grid in LDS (a counting sort, as search.hip's
//                                 proposals do for their one frame: integer atomics for the counts, a scan, uint16 indices per
//                                 cell), then one lane per point: is the pair tried, is the point visible, the cells under its
//                                 window, the Hamming minima over the point's observations inside the disc.  A proposing pair takes
//                                 atomicMin on the 64-bit key d0 << 32 | i of cell (c, k0); every pair leaves one word (k0, d0,
//                                 flags).  The fill order inside a grid cell differs from run to run; the choice is a minimum over
//                                 (d, k), so it does not matter.
//   fuse_project_count_kernel     grid (cam_stride, batch): per camera the pairs tried, visible, proposing, found (the key at (c, k0)
//                                 is the pair's own) and found with a holder.
//   fuse_project_fill_kernel      grid (cam_stride, batch): a camera's found pairs start behind those of the cameras below it (a scan
//                                 of the counts) and are compacted in ascending chunks of 256 points, so the order is (c, i);
//                                 writes stop at found_stride.  Camera 0's workgroup writes d_n_found and d_stats.
//   on the world (vslam_world_fuse_project, and the two host functions through which fuse.hip's world_fuse_run reads the extra log):
//   fuse_project_frames_kernel (the camera mask of a frame range), fuse_project_append_kernel (the found pairs and their keypoints'
//   descriptors onto the log), fuse_project_merge_kernel (the map's log with every point's extras appended to its row) and
//   fuse_project_gather_desc_kernel (a merged row's descriptor from the map's or the log's).
// What decides something is search_math.h's, fuse_math.h's and fuse_project_math.h's.  No floating-point atomics, no scratch.
#include <cmath>

#include "block_scan.h"
#include "ctx.h"
#include "../../include/vslam_fuse.h"
#include "../../include/vslam_fuse_project.h"
#include "fuse_project_math.h"

#pragma clang fp contract(off)

using namespace vs_search;
using namespace vs_fuse;
using namespace vs_fuse_project;

namespace {
constexpr int kPT = 256;                                       // lanes per workgroup
constexpr int kPPts = 1024;                                    // points per workgroup of the proposals
constexpr int kPCells = kSsMaxCells * kSsMaxCells;             // 4096
constexpr int kPCellsPerLane = kPCells / kPT;                  // the scan's share of a lane: 16 consecutive cells
constexpr int kPCounts = 8;                                    // per camera: tried, visible, proposing, found, with a holder; 3 spare
constexpr int kMaxCams = 1024;

struct FpArgs {
    const float4 *points;
    const int32_t *n_points;
    int pt_stride;
    const int32_t *off, *cam, *kp;
    const uint8_t *obs_desc;
    int obs_stride;
    const double *R, *T;
    const int32_t *n_cams;
    int cam_stride;
    const float2 *xy;
    const uint8_t *desc;
    const int32_t *n_kp;
    int kp_cams;                // cameras from one item's keypoint arrays (xy, desc, n_kp) to the next: >= every camera taking part
    int kp_stride;
    const int32_t *cam_mask;
    SsParams prm;
    int width, height;
    unsigned long long *keys;   // [batch][cam_stride][kp_stride], kFpNoKey ahead of the proposals
    int32_t *holder;            // [batch][cam_stride][kp_stride], kFpNoHolder ahead of the holders
    int32_t *prop;              // [batch][cam_stride][pt_stride]: fp_pack's word of every pair of a camera taking part and i < n
    int32_t *counts;            // [batch][cam_stride][kPCounts]
    int32_t *sound;             // [batch]: 1 where the CSR is sound
    int32_t *found_point, *found_cam, *found_kp, *found_dist, *found_holder;
    int found_stride;
    int32_t *n_found, *stats;
    int stats_stride;           // int32 from one item's stats to the next: 6, or 8 on the world
};

__device__ __forceinline__ void load_desc(const uint8_t *row, uint32_t (&w)[8]) {   // a 32-byte row, 16-byte aligned
    const uint4 a = reinterpret_cast<const uint4 *>(row)[0], b = reinterpret_cast<const uint4 *>(row)[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// camera c of item b, and whether it takes part
__device__ __forceinline__ bool load_cam(const FpArgs &a, int b, int c, LmCam &cam) {
    const size_t at = (size_t)b * a.cam_stride + c;
#pragma unroll
    for (int k = 0; k < 9; k++) cam.R[k] = a.R[at * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) cam.T[k] = a.T[at * 3 + k];
    const int C = min(max(a.n_cams[b], 0), a.cam_stride);
    return fp_cam_part(cam, c, C, a.cam_mask ? a.cam_mask + (size_t)b * a.cam_stride : nullptr);
}

__global__ __launch_bounds__(kPT) void fuse_project_holders_kernel(FpArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int S = a.pt_stride, KS = a.kp_stride;
    const int n = min(max(a.n_points[b], 0), S);
    const int32_t *OFF = a.off + (size_t)b * (S + 1);
    const int32_t *CAM = a.cam + (size_t)b * a.obs_stride, *KP = a.kp + (size_t)b * a.obs_stride;
    int32_t *H = a.holder + (size_t)b * a.cam_stride * KS;
    bool bad = false;
    for (int i = tid; i <= n; i += kPT) bad = bad || !fu_offset_ok(i > 0 ? OFF[i - 1] : 0, OFF[i], a.obs_stride);
    const bool broken = __syncthreads_or(bad);
    if (tid == 0) a.sound[b] = broken ? 0 : 1;
    if (broken) return;
    for (int i = tid; i < n; i += kPT) {
        for (int o = OFF[i], e = OFF[i + 1]; o < e; o++) {
            const int c = CAM[o], k = KP[o];
            if (fu_valid(c, k, a.cam_stride, KS)) atomicMin(&H[(size_t)c * KS + k], i);
        }
    }
}

__global__ __launch_bounds__(kPT) void fuse_project_propose_kernel(FpArgs a, VsK Kc) {
    __shared__ uint32_t cell_end[kPCells];        // counts, then starts, then (behind the fill) the end of every cell
    __shared__ uint16_t cell_kp[VSLAM_MAX_KP];    // keypoint indices, cell by cell
    __shared__ int scan_lds[kPT / 64];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    const int first = blockIdx.x * kPPts;
    if (first >= n || !a.sound[b]) return;   // the whole workgroup
    LmCam cam;
    if (!load_cam(a, b, c, cam)) return;     // the whole workgroup: the counts skip the camera too
    const size_t bc = (size_t)b * a.cam_stride + c, kc = (size_t)b * a.kp_cams + c;
    const int n_kp = min(max(a.n_kp[kc], 0), a.kp_stride);
    const float2 *XY = a.xy + kc * a.kp_stride;
    const SsGrid g = ss_grid(a.width, a.height, a.prm.radius);
    const int cells = g.nx * g.ny;

    // ---- the grid: count, scan, fill
    for (int q = tid; q < cells; q += kPT) cell_end[q] = 0;
    __syncthreads();
    auto cell_of = [&](int k) -> int {   // -1: no candidate of any point
        const float2 p = XY[k];
        if (!(isfinite(p.x) && isfinite(p.y))) return -1;
        return ss_cell((double)p.y, g.inv_c, g.ny) * g.nx + ss_cell((double)p.x, g.inv_c, g.nx);
    };
    for (int k = tid; k < n_kp; k += kPT) {
        const int q = cell_of(k);
        if (q >= 0) atomicAdd(&cell_end[q], 1u);
    }
    __syncthreads();
    {
        const int q0 = tid * kPCellsPerLane;
        int mine = 0;
#pragma unroll
        for (int j = 0; j < kPCellsPerLane; j++) mine += q0 + j < cells ? (int)cell_end[q0 + j] : 0;
        int total;
        int run = vs_block_excl_scan<kPT>(mine, scan_lds, total);
#pragma unroll
        for (int j = 0; j < kPCellsPerLane; j++) {
            if (q0 + j < cells) {
                const int cnt = (int)cell_end[q0 + j];
                cell_end[q0 + j] = (uint32_t)run;
                run += cnt;
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < n_kp; k += kPT) {
        const int q = cell_of(k);
        if (q >= 0) cell_kp[atomicAdd(&cell_end[q], 1u)] = (uint16_t)k;   // at most n_kp <= VSLAM_MAX_KP entries in all
    }
    __syncthreads();

    // ---- the points: one lane each
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = (double)Kc.v[k];
    const int32_t *OO = a.off + (size_t)b * (a.pt_stride + 1);
    const int32_t *OC = a.cam + (size_t)b * a.obs_stride, *OK = a.kp + (size_t)b * a.obs_stride;
    const uint8_t *OD = a.obs_desc + (size_t)b * a.obs_stride * VSLAM_DESC_BYTES;
    const uint8_t *D = a.desc + kc * a.kp_stride * VSLAM_DESC_BYTES;
    unsigned long long *KEYS = a.keys + bc * a.kp_stride;
    int32_t *PROP = a.prop + bc * a.pt_stride;
    const double reach = a.prm.radius + kSsMargin;
    for (int p = tid; p < kPPts; p += kPT) {
        const int i = first + p;
        if (i >= n) break;
        const float4 P = a.points[(size_t)b * a.pt_stride + i];
        const int o0 = OO[i], o1 = OO[i + 1];
        const bool tried = fp_point_part(P.x, P.y, P.z, o0, o1, a.obs_stride) && !fp_seen(OC, OK, o0, o1, c, a.kp_stride);
        double u, v;
        const bool visible = tried && ss_visible(K, cam, true, P.x, P.y, P.z, o0, o1, a.obs_stride, a.width, a.height, u, v);
        SsBest best;
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
        PROP[i] = fp_pack(tried, visible, proposes, best.k0, best.d0);
        if (proposes) atomicMin(&KEYS[best.k0], ss_key(best.d0, (uint32_t)i));
    }
}

// a pair's word -> has it found its keypoint
__device__ __forceinline__ bool pair_found(int32_t w, int i, const unsigned long long *KEYS) {
    return (w & kFpProposes) && KEYS[fp_k0(w)] == ss_key((uint32_t)fp_d0(w), (uint32_t)i);
}

__global__ __launch_bounds__(kPT) void fuse_project_count_kernel(FpArgs a) {
    __shared__ int sums[5];
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const size_t bc = (size_t)b * a.cam_stride + c;
    if (tid < 5) sums[tid] = 0;
    __syncthreads();
    LmCam cam;
    if (a.sound[b] && load_cam(a, b, c, cam)) {   // the same for every lane
        const int n = min(max(a.n_points[b], 0), a.pt_stride);
        const unsigned long long *KEYS = a.keys + bc * a.kp_stride;
        const int32_t *H = a.holder + bc * a.kp_stride, *PROP = a.prop + bc * a.pt_stride;
        int tried = 0, visible = 0, proposing = 0, found = 0, held = 0;
        for (int i = tid; i < n; i += kPT) {
            const int32_t w = PROP[i];
            tried += (w & kFpTried) ? 1 : 0;
            visible += (w & kFpVisible) ? 1 : 0;
            proposing += (w & kFpProposes) ? 1 : 0;
            if (pair_found(w, i, KEYS)) {
                found++;
                held += H[fp_k0(w)] != kFpNoHolder ? 1 : 0;
            }
        }
        atomicAdd(&sums[0], tried);
        atomicAdd(&sums[1], visible);
        atomicAdd(&sums[2], proposing);
        atomicAdd(&sums[3], found);
        atomicAdd(&sums[4], held);
    }
    __syncthreads();
    if (tid < 5) a.counts[bc * kPCounts + tid] = sums[tid];
}

__global__ __launch_bounds__(kPT) void fuse_project_fill_kernel(FpArgs a) {
    __shared__ int scan_lds[kPT / 64];
    __shared__ int sums[6];   // the found pairs of the cameras below c; then the five counts over every camera
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const size_t bc = (size_t)b * a.cam_stride + c;
    const int32_t *CNT = a.counts + (size_t)b * a.cam_stride * kPCounts;
    if (tid < 6) sums[tid] = 0;
    __syncthreads();
    int below = 0, all[5] = {0, 0, 0, 0, 0};
    for (int q = tid; q < a.cam_stride; q += kPT) {
        below += q < c ? CNT[q * kPCounts + 3] : 0;
        if (c == 0) {
#pragma unroll
            for (int j = 0; j < 5; j++) all[j] += CNT[q * kPCounts + j];
        }
    }
    atomicAdd(&sums[0], below);
    if (c == 0) {
#pragma unroll
        for (int j = 0; j < 5; j++) atomicAdd(&sums[1 + j], all[j]);
    }
    __syncthreads();
    if (c == 0) {
        const int written = min(sums[4], a.found_stride);
        if (tid == 0) a.n_found[b] = written;
        if (a.stats) {
            if (tid < 5) a.stats[(size_t)b * a.stats_stride + tid] = sums[1 + tid];
            if (tid == 5) a.stats[(size_t)b * a.stats_stride + 5] = written;
        }
    }
    int run = sums[0];
    if (CNT[c * kPCounts + 3] == 0 || run >= a.found_stride) return;   // the whole workgroup: nothing of this camera is written
    const int n = min(max(a.n_points[b], 0), a.pt_stride);
    const unsigned long long *KEYS = a.keys + bc * a.kp_stride;
    const int32_t *H = a.holder + bc * a.kp_stride, *PROP = a.prop + bc * a.pt_stride;
    for (int base = 0; base < n; base += kPT) {   // ascending chunks: the compacted order is the points' order
        const int i = base + tid;
        const int32_t w = i < n ? PROP[i] : 0;
        const bool found = i < n && pair_found(w, i, KEYS);
        int chunk;
        const int pos = run + vs_block_flag_scan<kPT>(found, scan_lds, chunk);
        if (found && pos < a.found_stride) {
            const size_t slot = (size_t)b * a.found_stride + pos;
            const int k = fp_k0(w), h = H[k];
            a.found_point[slot] = i;
            a.found_cam[slot] = c;
            a.found_kp[slot] = k;
            a.found_dist[slot] = fp_d0(w);
            a.found_holder[slot] = h == kFpNoHolder ? -1 : h;
        }
        run += chunk;
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

// the arena slots, the fill of the keys and the holders, and the four launches; everything has been checked
int launch_fuse_project(vslam_ctx *ctx, FpArgs a, int batch, const float *h_K) {
    const size_t cells = (size_t)batch * a.cam_stride * a.kp_stride, pairs = (size_t)batch * a.cam_stride * a.pt_stride;
    const size_t cams = (size_t)batch * a.cam_stride;
    int rc;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "fuse_project_cells", cells * (sizeof(unsigned long long) + sizeof(int32_t)), &ptr))) return rc;
    a.keys = static_cast<unsigned long long *>(ptr);
    a.holder = reinterpret_cast<int32_t *>(a.keys + cells);
    if ((rc = vs_arena_get(ctx, "fuse_project_work", sizeof(int32_t) * (pairs + cams * kPCounts + batch), &ptr))) return rc;
    a.prop = static_cast<int32_t *>(ptr);
    a.counts = a.prop + pairs;
    a.sound = a.counts + cams * kPCounts;
    VS_HIP(ctx, hipMemsetAsync(a.keys, 0x7F, cells * (sizeof(unsigned long long) + sizeof(int32_t)), ctx->stream));
    {
        VsProfScope ps(ctx, "fuse_project_holders_kernel");
        fuse_project_holders_kernel<<<batch, kPT, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "fuse_project_propose_kernel");
        fuse_project_propose_kernel<<<dim3(vs_div_up(a.pt_stride, kPPts), a.cam_stride, batch), kPT, 0, ctx->stream>>>(a, vs_pack_K(h_K));
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "fuse_project_count_kernel");
        fuse_project_count_kernel<<<dim3(a.cam_stride, batch), kPT, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    {
        VsProfScope ps(ctx, "fuse_project_fill_kernel");
        fuse_project_fill_kernel<<<dim3(a.cam_stride, batch), kPT, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

// ---- on the world
__device__ __forceinline__ int ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct ExtraLog {
    int32_t *point, *frame, *kp;   // [tracks][capacity]
    uint8_t *desc;                 // [tracks][capacity][32]
    int32_t *n;                    // [tracks]
    int capacity;
};

ExtraLog log_of(const vslam_world *w) { return ExtraLog{w->extra_point, w->extra_frame, w->extra_kp, w->extra_desc, w->n_extra, w->extra_capacity}; }

// the cameras of frames lo <= f < hi take part
__global__ __launch_bounds__(kPT) void fuse_project_frames_kernel(int32_t *mask, int max_frames, int lo, int hi) {
    const int f = blockIdx.x * kPT + threadIdx.x;
    if (f < max_frames) mask[(size_t)blockIdx.y * max_frames + f] = f >= lo && f < hi ? 0 : -1;
}

// grid (tracks): the found pairs of a track appended to its log while there is room, with the keypoints' descriptors; the two counts
// behind the kernel's six
__global__ __launch_bounds__(kPT) void fuse_project_append_kernel(FpArgs a, ExtraLog g) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int held = min(max(g.n[b], 0), g.capacity);
    const int take = min(min(max(a.n_found[b], 0), a.found_stride), g.capacity - held);
    for (int j = tid; j < take; j += kPT) {
        const size_t from = (size_t)b * a.found_stride + j, to = (size_t)b * g.capacity + held + j;
        const int c = a.found_cam[from], k = a.found_kp[from];
        g.point[to] = a.found_point[from];
        g.frame[to] = c;
        g.kp[to] = k;
        const uint4 *src = reinterpret_cast<const uint4 *>(a.desc + (((size_t)b * a.kp_cams + c) * a.kp_stride + k) * VSLAM_DESC_BYTES);
        uint4 *dst = reinterpret_cast<uint4 *>(g.desc + to * VSLAM_DESC_BYTES);
        dst[0] = src[0];
        dst[1] = src[1];
    }
    __syncthreads();   // every lane has read g.n
    if (tid == 0) {
        g.n[b] = held + take;
        a.stats[(size_t)b * a.stats_stride + 6] = take;
        a.stats[(size_t)b * a.stats_stride + 7] = held + take;
    }
}

// grid (tracks): the map's log with every point's admitted extras appended to its row.  The extras of every point are counted
// (integer atomics), the rows' new starts are a scan over ascending chunks of points, every lane moves its own point's row, and the
// extras take their places in ascending chunks of 256: an extra stands behind the earlier extras of its point, those of earlier
// chunks by the point's running position, those of its own chunk counted in LDS.  Words that one lane writes and another reads
// (counts, running positions) move by relaxed device-scope atomics; barriers order them.
__global__ __launch_bounds__(kPT) void fuse_project_merge_kernel(ExtraLog g, const int32_t *sizes, int P, int O, const int32_t *log_off,
                                                                 const int32_t *log_frame, const int32_t *log_kp, int32_t *off, int32_t *frame,
                                                                 int32_t *kp, int32_t *src, int32_t *work) {
    __shared__ int scan_lds[kPT / 64];
    __shared__ int sh_p[kPT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(sizes[b], 0), P);
    const int32_t *LO = log_off + (size_t)b * (P + 1), *LF = log_frame + (size_t)b * O, *LK = log_kp + (size_t)b * O;
    int32_t *OFF = off + (size_t)b * (P + 1), *FR = frame + (size_t)b * O, *KP = kp + (size_t)b * O, *SRC = src + (size_t)b * O;
    int32_t *CNT = work + (size_t)b * 2 * P, *RUN = CNT + P;
    const int32_t *EP = g.point + (size_t)b * g.capacity, *EF = g.frame + (size_t)b * g.capacity, *EK = g.kp + (size_t)b * g.capacity;
    const int total = min(max(LO[n], 0), O);
    const int admit = min(min(max(g.n[b], 0), g.capacity), O - total);
    for (int i = tid; i < n; i += kPT) st(&CNT[i], 0);
    __syncthreads();
    for (int e = tid; e < admit; e += kPT) {
        const int p = EP[e];
        if (p >= 0 && p < n) atomicAdd(&CNT[p], 1);
    }
    __syncthreads();
    int run = 0;
    for (int base = 0; base < n; base += kPT) {   // ascending chunks: the rows keep the points' order
        const int i = base + tid;
        const int mine = i < n ? ld(&CNT[i]) : 0;
        int chunk;
        const int before = run + vs_block_excl_scan<kPT>(mine, scan_lds, chunk);
        if (i < n) {
            const int o0 = LO[i], o1 = LO[i + 1];
            OFF[i] = o0 + before;
            for (int o = o0; o < o1; o++) {   // o + before < total + admit <= O
                FR[o + before] = LF[o];
                KP[o + before] = LK[o];
                SRC[o + before] = o;
            }
            st(&RUN[i], o1 + before);
        }
        run += chunk;
    }
    for (int i = n + tid; i <= P; i += kPT) OFF[i] = total + run;
    __syncthreads();
    for (int base = 0; base < admit; base += kPT) {   // ascending chunks: a point's extras keep the order they were appended in
        const int e = base + tid;
        int p = -1;
        if (e < admit) {
            p = EP[e];
            if (!(p >= 0 && p < n)) p = -1;
        }
        sh_p[tid] = p;
        __syncthreads();
        if (p >= 0) {
            int at = ld(&RUN[p]);
            for (int j = 0; j < tid; j++) at += sh_p[j] == p ? 1 : 0;
            FR[at] = EF[e];
            KP[at] = EK[e];
            SRC[at] = O + e;
        }
        __syncthreads();
        if (p >= 0) atomicAdd(&RUN[p], 1);
        __syncthreads();
    }
}

// the descriptors of a fusion's merged rows over such lists; rows past the track's total keep their bits
__global__ __launch_bounds__(kPT) void fuse_project_gather_desc_kernel(const int32_t *out_off, const int32_t *out_src, const int32_t *src,
                                                                       const uint4 *log_desc, const uint4 *extra_desc, int capacity, uint4 *desc,
                                                                       int P, int O) {
    const int b = blockIdx.y, idx = blockIdx.x * kPT + threadIdx.x, o = idx >> 1, half = idx & 1;
    const int total = min(max(out_off[(size_t)b * (P + 1) + P], 0), O);
    if (o >= total) return;
    const int from = src[(size_t)b * O + out_src[(size_t)b * O + o]];
    desc[((size_t)b * O + o) * 2 + half] = from < O ? log_desc[((size_t)b * O + from) * 2 + half]
                                                    : extra_desc[((size_t)b * capacity + (from - O)) * 2 + half];
}

// the extra log, made on the first vslam_world_fuse_project of a world and freed with it
int extras_make(vslam_ctx *ctx, vslam_world *world, int obs_capacity) {
    if (world->n_extra) {
        VS_REQUIRE(ctx, world->extra_capacity == obs_capacity, VSLAM_ERR_INVALID);
        return VSLAM_OK;
    }
    const size_t rows = (size_t)world->tracks * obs_capacity;
    void *ptr = nullptr;
    VS_HIP(ctx, hipMalloc(&ptr, sizeof(int32_t) * (3 * rows + world->tracks) + rows * VSLAM_DESC_BYTES));
    world->owned.push_back(ptr);
    world->extra_desc = static_cast<uint8_t *>(ptr);   // first: 16-byte rows
    world->extra_point = reinterpret_cast<int32_t *>(world->extra_desc + rows * VSLAM_DESC_BYTES);
    world->extra_frame = world->extra_point + rows;
    world->extra_kp = world->extra_frame + rows;
    world->n_extra = world->extra_kp + rows;
    world->extra_capacity = obs_capacity;
    VS_HIP(ctx, hipMemsetAsync(world->n_extra, 0, sizeof(int32_t) * (size_t)world->tracks, ctx->stream));
    return VSLAM_OK;
}
}  // namespace

int vs_world_extras_merge(vslam_ctx *ctx, vslam_world *world, const int32_t *sizes, int P, int O, const int32_t *log_off, const int32_t *log_frame,
                          const int32_t *log_kp, int32_t *off, int32_t *frame, int32_t *kp, int32_t *src, int32_t *work) {
    VsProfScope ps(ctx, "fuse_project_merge_kernel");
    fuse_project_merge_kernel<<<world->tracks, kPT, 0, ctx->stream>>>(log_of(world), sizes, P, O, log_off, log_frame, log_kp, off, frame, kp, src, work);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vs_world_extras_gather_desc(vslam_ctx *ctx, vslam_world *world, int P, int O, const int32_t *out_off, const int32_t *out_src, const int32_t *src,
                                const uint8_t *log_desc, uint8_t *desc) {
    VsProfScope ps(ctx, "fuse_project_gather_desc_kernel");
    fuse_project_gather_desc_kernel<<<dim3(vs_div_up(2 * O, kPT), world->tracks), kPT, 0, ctx->stream>>>(
        out_off, out_src, src, reinterpret_cast<const uint4 *>(log_desc), reinterpret_cast<const uint4 *>(world->extra_desc), world->extra_capacity,
        reinterpret_cast<uint4 *>(desc), P, O);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

extern "C" {

int vslam_fuse_project(vslam_ctx *ctx, const float *d_points, const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets,
                       const int32_t *d_obs_cam, const int32_t *d_obs_kp, const uint8_t *d_obs_desc, int obs_stride, const double *d_R,
                       const double *d_T, const int32_t *d_n_cams, int cam_stride, const float *d_xy, const uint8_t *d_desc,
                       const int32_t *d_n_kp, int kp_stride, const int32_t *d_cam_mask, const float *h_K, int width, int height, int batch,
                       const vslam_search_params *params, int32_t *d_found_point, int32_t *d_found_cam, int32_t *d_found_kp,
                       int32_t *d_found_dist, int32_t *d_found_holder, int found_stride, int32_t *d_n_found, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_points && d_n_points && d_obs_offsets && d_obs_cam && d_obs_kp && d_obs_desc && d_R && d_T && d_n_cams && d_xy && d_desc &&
                        d_n_kp && h_K, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_found_point && d_found_cam && d_found_kp && d_found_dist && d_found_holder && d_n_found, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && pt_stride > 0 && obs_stride > 0 && cam_stride > 0 && kp_stride > 0 && found_stride > 0 && width > 0 && height > 0,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP && cam_stride <= kMaxCams && width <= 16384 && height <= 16384, VSLAM_ERR_CAPACITY);
    VS_REQUIRE(ctx, batch <= 65535, VSLAM_ERR_CAPACITY);   // the grid's z
    vslam_search_params p;
    vslam_search_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_points, 16);   // float4 rows
    VS_ALIGNED(ctx, d_desc, 16);     // descriptor rows move as uint4 pairs
    VS_ALIGNED(ctx, d_obs_desc, 16);
    VS_ALIGNED(ctx, d_xy, 8);        // float2 rows
    VS_REQUIRE(ctx, vs_ptr_bits(d_R, d_T) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_points, d_obs_offsets, d_obs_cam, d_obs_kp, d_n_cams, d_n_kp, d_cam_mask, d_found_point, d_found_cam,
                                d_found_kp, d_found_dist, d_found_holder, d_n_found, d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    FpArgs a;
    a.points = reinterpret_cast<const float4 *>(d_points); a.n_points = d_n_points; a.pt_stride = pt_stride;
    a.off = d_obs_offsets; a.cam = d_obs_cam; a.kp = d_obs_kp; a.obs_desc = d_obs_desc; a.obs_stride = obs_stride;
    a.R = d_R; a.T = d_T; a.n_cams = d_n_cams; a.cam_stride = cam_stride;
    a.xy = reinterpret_cast<const float2 *>(d_xy); a.desc = d_desc; a.n_kp = d_n_kp; a.kp_cams = cam_stride; a.kp_stride = kp_stride;
    a.cam_mask = d_cam_mask;
    a.prm = ss_params(p.radius_px, p.dist_threshold, p.ratio10);
    a.width = width; a.height = height;
    a.keys = nullptr; a.holder = nullptr; a.prop = nullptr; a.counts = nullptr; a.sound = nullptr;
    a.found_point = d_found_point; a.found_cam = d_found_cam; a.found_kp = d_found_kp; a.found_dist = d_found_dist;
    a.found_holder = d_found_holder; a.found_stride = found_stride; a.n_found = d_n_found; a.stats = d_stats; a.stats_stride = 6;
    return launch_fuse_project(ctx, a, batch, h_K);
}

int vslam_world_fuse_project(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp,
                             int xy_frames, const float *h_K, int width, int height, int frame_lo, int frame_hi,
                             const vslam_search_params *search, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy && d_desc && d_n_kp && h_K, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &m))) return rc;
    VS_REQUIRE(ctx, xy_frames >= m.frames && width > 0 && height > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, frame_lo >= 0 && frame_lo <= frame_hi && frame_hi <= m.frames, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, m.max_frames <= kMaxCams && width <= 16384 && height <= 16384 && m.tracks <= 65535, VSLAM_ERR_CAPACITY);
    vslam_search_params p;
    vslam_search_params_default(&p);
    if (search) p = *search;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xy, 8);
    VS_ALIGNED(ctx, d_desc, 16);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_kp, d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    if ((rc = vs_world_fusion_make(ctx, world))) return rc;   // ahead of the log: making d_fuse_to resets the fusion state
    if ((rc = extras_make(ctx, world, m.obs_capacity))) return rc;
    const size_t T = m.tracks, P = m.map_capacity, O = m.obs_capacity, Fr = m.max_frames;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_fuse_project_i32", sizeof(int32_t) * T * ((P + 1) + 2 * O + Fr + 1 + 5 * O + 1 + 8), &ptr))) return rc;
    int32_t *off = static_cast<int32_t *>(ptr), *frame = off + T * (P + 1), *kp = frame + T * O, *mask = kp + T * O, *n_cams = mask + T * Fr,
            *found = n_cams + T, *n_found = found + 5 * T * O, *stats = n_found + T;
    if ((rc = vs_arena_get(ctx, "world_fuse_project_desc", T * O * VSLAM_DESC_BYTES, &ptr))) return rc;
    uint8_t *obs_desc = static_cast<uint8_t *>(ptr);
    if ((rc = vs_arena_get(ctx, "world_fuse_project_f64", sizeof(double) * T * Fr * 12, &ptr))) return rc;
    double *R = static_cast<double *>(ptr), *Tv = R + T * Fr * 9;
    if ((rc = vs_world_csr(ctx, world, map, off, frame, kp, obs_desc))) return rc;
    if ((rc = vs_world_cameras(ctx, world, m.max_frames, m.frames, R, Tv, n_cams))) return rc;
    fuse_project_frames_kernel<<<dim3(vs_div_up(m.max_frames, kPT), m.tracks), kPT, 0, ctx->stream>>>(mask, m.max_frames, frame_lo, frame_hi);
    VS_HIP(ctx, hipGetLastError());
    FpArgs a;
    a.points = reinterpret_cast<const float4 *>(world->world_points); a.n_points = static_cast<const int32_t *>(m.d_sizes); a.pt_stride = m.map_capacity;
    a.off = off; a.cam = frame; a.kp = kp; a.obs_desc = obs_desc; a.obs_stride = m.obs_capacity;
    a.R = R; a.T = Tv; a.n_cams = n_cams; a.cam_stride = m.max_frames;
    a.xy = reinterpret_cast<const float2 *>(d_xy); a.desc = d_desc; a.n_kp = d_n_kp; a.kp_cams = xy_frames; a.kp_stride = m.kp_stride;
    a.cam_mask = mask;
    a.prm = ss_params(p.radius_px, p.dist_threshold, p.ratio10);
    a.width = width; a.height = height;
    a.keys = nullptr; a.holder = nullptr; a.prop = nullptr; a.counts = nullptr; a.sound = nullptr;
    a.found_point = found; a.found_cam = found + T * O; a.found_kp = found + 2 * T * O; a.found_dist = found + 3 * T * O;
    a.found_holder = found + 4 * T * O; a.found_stride = m.obs_capacity; a.n_found = n_found; a.stats = d_stats ? d_stats : stats; a.stats_stride = 8;
    if ((rc = launch_fuse_project(ctx, a, m.tracks, h_K))) return rc;
    fuse_project_append_kernel<<<m.tracks, kPT, 0, ctx->stream>>>(a, log_of(world));
    VS_HIP(ctx, hipGetLastError());
    world->fusion |= 4;
    return vslam_world_fuse(ctx, world, map, nullptr);
}

int vslam_world_fuse_project_view(vslam_world *world, int32_t **d_extra_point, int32_t **d_extra_frame, int32_t **d_extra_kp,
                                  uint8_t **d_extra_desc, int32_t **d_n_extra, int32_t *capacity) {
    if (!world || !d_extra_point || !d_extra_frame || !d_extra_kp || !d_extra_desc || !d_n_extra) return VSLAM_ERR_INVALID;
    const bool exist = world->fusion & 4;
    *d_extra_point = exist ? world->extra_point : nullptr;
    *d_extra_frame = exist ? world->extra_frame : nullptr;
    *d_extra_kp = exist ? world->extra_kp : nullptr;
    *d_extra_desc = exist ? world->extra_desc : nullptr;
    *d_n_extra = exist ? world->n_extra : nullptr;
    if (capacity) *capacity = exist ? world->extra_capacity : 0;
    return VSLAM_OK;
}

}  // extern "C"
