// Fusing map points that share an observation and culling the unsupported ones (include/vslam_fuse.h), for a batch of independent
// items.
//   fuse_points_kernel   grid (batch): one workgroup per item.  The CSR is checked; labels start as the points' own indices and live
//                        in d_fuse_to.  A round posts every point's label into the cell (cam, kp) of each of its valid observations
//                        (integer atomicMin on a table [cam_stride][kp_stride] from the arena, filled once with kNone: labels only
//                        decrease, so a cell never needs to be reset between rounds), lets every point take the minimum over its
//                        cells, and jumps once through the label's label.  A round that changes nothing ends the loop; it is capped
//                        at n + 1 rounds.  After it a cell belongs to one group, so the same table, reset where it was touched,
//                        takes a second minimum over input rows: an entry is kept iff its cell holds its own row.  The rows'
//                        places: ascending chunks of 256 points, every lane adding up the kept counts of the earlier lanes of its
//                        chunk that have its survivor (LDS) on top of the group's running count; then a scan over the survivors.
//   cull_points_kernel   grid (ceil(pt_stride / 256), batch): one lane per point (fuse_math.h's fu_cull_point), the four counts by
//                        integer atomics behind a fill of d_stats.
//   on the world (vslam_world_fuse, vslam_world_cull, vslam_world_observations and vs_world_csr, the helper through which every world
//   call obtains its CSR): fuse_identity_kernel (d_fuse_to = "no fusion"), fuse_gather_desc_kernel (the merged rows' descriptors
//   through d_out_src), world_fuse_apply_kernel (the new d_fuse_to, NaN rows for the newly absorbed), world_cameras_kernel (camera f =
//   recorded frame f from d_Twc; vs_world_cameras is its launch for tracks.hip too), world_cull_apply_kernel (-1 and a NaN row for the culled, -1 for the members of a culled survivor).
// Words that one lane writes and another reads inside the fusion (labels, cells, running counts, row starts) move by relaxed
// device-scope atomic loads and stores, which do not stay in a lane's nearest cache; barriers order them.  Integers only there; no
// floating-point atomics and no scratch anywhere.
#include <cmath>

#include "block_scan.h"
#include "ctx.h"
#include "../../include/vslam_fuse.h"
#include "../../include/vslam_search.h"
#include "fuse_math.h"

#pragma clang fp contract(off)

using namespace vs_fuse;

namespace {
constexpr int kFT = 256;             // lanes per workgroup
constexpr int kNone = 0x7F7F7F7F;    // what the fill (bytes of 0x7F) leaves in a cell: above every label and every row
constexpr int kMaxCams = 1024;

__device__ __forceinline__ int ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct FuseArgs {
    const int32_t *n_points;
    int pt_stride;
    const int32_t *off, *cam, *kp;
    int obs_stride, cam_stride, kp_stride;
    const int32_t *mask;
    int32_t *fuse_to, *out_off, *out_cam, *out_kp, *out_src, *stats;
    int32_t *cells;   // [batch][cam_stride * kp_stride], kNone
    int32_t *work;    // [batch][3][pt_stride]: a group's running count, a member's place in its group's row, "has absorbed"
};

__global__ __launch_bounds__(kFT) void fuse_points_kernel(FuseArgs a) {
    __shared__ int scan_lds[kFT / 64];
    __shared__ int sh_s[kFT], sh_c[kFT];
    __shared__ int counts[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int S = a.pt_stride, KS = a.kp_stride;
    const int n = min(max(a.n_points[b], 0), S);
    const int32_t *OFF = a.off + (size_t)b * (S + 1);
    const int32_t *CAM = a.cam + (size_t)b * a.obs_stride, *KP = a.kp + (size_t)b * a.obs_stride;
    const int32_t *MASK = a.mask ? a.mask + (size_t)b * S : nullptr;
    int32_t *FT = a.fuse_to + (size_t)b * S;
    int32_t *OUT_OFF = a.out_off + (size_t)b * (S + 1);
    int32_t *OUT_CAM = a.out_cam + (size_t)b * a.obs_stride, *OUT_KP = a.out_kp + (size_t)b * a.obs_stride;
    int32_t *OUT_SRC = a.out_src ? a.out_src + (size_t)b * a.obs_stride : nullptr;
    int32_t *CELLS = a.cells + (size_t)b * a.cam_stride * KS;
    int32_t *RUN = a.work + (size_t)b * 3 * S, *WITHIN = RUN + S, *MULTI = WITHIN + S;
    if (tid < 3) counts[tid] = 0;

    // ---- the CSR: offsets[0 .. n] start at >= 0, never decrease, end at <= obs_stride
    bool bad = false;
    for (int i = tid; i <= n; i += kFT) bad = bad || !fu_offset_ok(i > 0 ? OFF[i - 1] : 0, OFF[i], a.obs_stride);
    if (__syncthreads_or(bad)) {
        for (int i = tid; i < S; i += kFT) FT[i] = i;
        for (int i = tid; i <= S; i += kFT) OUT_OFF[i] = 0;
        if (a.stats && tid < 4) a.stats[(size_t)b * 4 + tid] = 0;
        return;
    }

    // ---- labels: a point's mask is read before its label is written (d_mask may be d_fuse_to)
    for (int i = tid; i < S; i += kFT) {
        const bool part = i < n && (!MASK || MASK[i] >= 0);
        st(&FT[i], i < n && !part ? -1 : i);
        if (i < n) {
            st(&RUN[i], 0);
            st(&MULTI[i], 0);
        }
    }
    __syncthreads();

    // every valid entry of the points taking part that this lane owns: f(row, cell)
    auto each_entry = [&](int i, int label, auto f) {
        if (label < 0) return;
        for (int o = OFF[i], e = OFF[i + 1]; o < e; o++) {
            const int c = CAM[o], k = KP[o];
            if (fu_valid(c, k, a.cam_stride, KS)) f(o, &CELLS[(size_t)c * KS + k]);
        }
    };

    // ---- rounds, capped: labels only decrease, so a correct run ends by the unchanged round long before
    for (int round = 0; round <= n; round++) {
        for (int i = tid; i < n; i += kFT) {
            const int L = ld(&FT[i]);
            each_entry(i, L, [&](int, int32_t *cell) { atomicMin(cell, L); });
        }
        __syncthreads();
        bool changed = false;
        for (int i = tid; i < n; i += kFT) {
            const int L = ld(&FT[i]);
            int m = L;
            each_entry(i, L, [&](int, int32_t *cell) { m = min(m, ld(cell)); });
            if (m < L) {
                st(&FT[i], m);
                changed = true;
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += kFT) {   // a label is the index of a point taking part, whose own label is one too
            const int L = ld(&FT[i]);
            if (L < 0) continue;
            const int LL = ld(&FT[L]);
            if (LL < L) {
                st(&FT[i], LL);
                changed = true;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }

    // ---- kept entries: the smallest input row of every cell
    for (int i = tid; i < n; i += kFT) each_entry(i, ld(&FT[i]), [&](int, int32_t *cell) { st(cell, kNone); });
    __syncthreads();
    for (int i = tid; i < n; i += kFT) each_entry(i, ld(&FT[i]), [&](int o, int32_t *cell) { atomicMin(cell, o); });
    __syncthreads();

    // ---- a member's place in its group's row, in ascending chunks
    int taking = 0, absorbed = 0;
    for (int base = 0; base < n; base += kFT) {
        const int i = base + tid;
        int s = -1, c = 0;
        if (i < n) {
            s = ld(&FT[i]);
            each_entry(i, s, [&](int o, int32_t *cell) { c += ld(cell) == o ? 1 : 0; });
            if (s >= 0) {
                taking++;
                if (s != i) {
                    absorbed++;
                    st(&MULTI[s], 1);
                }
            }
        }
        sh_s[tid] = s;
        sh_c[tid] = c;
        __syncthreads();
        if (s >= 0) {
            int w = ld(&RUN[s]);
            for (int j = 0; j < tid; j++) w += sh_s[j] == s ? sh_c[j] : 0;
            WITHIN[i] = w;   // read again by this lane only
        }
        __syncthreads();
        if (s >= 0 && c > 0) atomicAdd(&RUN[s], c);
        __syncthreads();
    }

    // ---- the merged offsets: a survivor's row is its group's count, every other row is empty
    int run = 0, multi = 0;
    for (int base = 0; base < n; base += kFT) {
        const int i = base + tid;
        int v = 0;
        if (i < n && ld(&FT[i]) == i) {
            v = ld(&RUN[i]);
            multi += ld(&MULTI[i]);
        }
        int chunk;
        const int pos = run + vs_block_excl_scan<kFT>(v, scan_lds, chunk);
        if (i < n) st(&OUT_OFF[i], pos);
        run += chunk;
    }
    for (int i = n + tid; i <= S; i += kFT) OUT_OFF[i] = run;
    __syncthreads();

    // ---- the entries: at most as many as the input's valid ones, so below offsets[n] <= obs_stride
    for (int i = tid; i < n; i += kFT) {
        const int s = ld(&FT[i]);
        if (s < 0) continue;
        int pos = ld(&OUT_OFF[s]) + WITHIN[i];
        each_entry(i, s, [&](int o, int32_t *cell) {
            if (ld(cell) != o) return;
            OUT_CAM[pos] = CAM[o];
            OUT_KP[pos] = KP[o];
            if (OUT_SRC) OUT_SRC[pos] = o;
            pos++;
        });
    }
    if (!a.stats) return;
    atomicAdd(&counts[0], taking);
    atomicAdd(&counts[1], multi);
    atomicAdd(&counts[2], absorbed);
    __syncthreads();
    if (tid < 3) a.stats[(size_t)b * 4 + tid] = counts[tid];
    if (tid == 3) a.stats[(size_t)b * 4 + 3] = run;
}

struct CullArgs {
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
    FuCull prm;
    int32_t *keep, *counts, *stats;
};

__global__ __launch_bounds__(kFT) void cull_points_kernel(CullArgs a, VsK Kc) {
    __shared__ int sums[4];
    const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * kFT + tid;
    if (tid < 4) sums[tid] = 0;
    __syncthreads();
    const int S = a.pt_stride;
    const int n = min(max(a.n_points[b], 0), S);
    const int C = min(max(a.n_cams[b], 0), a.cam_stride);
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = (double)Kc.v[k];
    int keep = -1, n_usable = 0, n_good = 0;
    if (i < n) {
        const float4 P = a.points[(size_t)b * S + i];
        const int32_t *OFF = a.off + (size_t)b * (S + 1);
        keep = fu_cull_point(K, P.x, P.y, P.z, OFF[i], OFF[i + 1], a.obs_stride, a.cam + (size_t)b * a.obs_stride,
                             a.kp + (size_t)b * a.obs_stride, C, a.kp_stride, a.R + (size_t)b * a.cam_stride * 9,
                             a.T + (size_t)b * a.cam_stride * 3, a.xy + (size_t)b * a.xy_item, a.prm, n_usable, n_good);
    }
    if (i < S) {
        a.keep[(size_t)b * S + i] = keep;
        if (a.counts) {
            a.counts[((size_t)b * S + i) * 2] = n_usable;
            a.counts[((size_t)b * S + i) * 2 + 1] = n_good;
        }
    }
    if (keep >= 0) {
        atomicAdd(&sums[0], 1);
        atomicAdd(&sums[keep ? 1 : 2], 1);
        if (n_good) atomicAdd(&sums[3], n_good);
    }
    __syncthreads();
    if (tid < 4 && sums[tid]) atomicAdd(&a.stats[(size_t)b * 4 + tid], sums[tid]);
}

bool cull_params_ok(const vslam_cull_params &p) {
    return std::isfinite(p.inlier_px) && p.inlier_px > 0.0 && p.min_good >= 1 && p.mature_good >= 1 && p.mature_age >= 0 &&
           p.mature_age <= (1 << 20) && p.good10 >= 0 && p.good10 <= 10;
}

// ---- on the world
constexpr uint32_t kQuietNaN = 0x7FC00000u;

__device__ __forceinline__ void nan_row(float *row) {
    uint32_t *w = reinterpret_cast<uint32_t *>(row);
    w[0] = w[1] = w[2] = kQuietNaN;
    w[3] = 0u;
}

__global__ __launch_bounds__(kFT) void fuse_identity_kernel(int32_t *fuse_to, int P) {
    const int i = blockIdx.x * kFT + threadIdx.x;
    if (i < P) fuse_to[(size_t)blockIdx.y * P + i] = i;
}

// the descriptors of the merged rows: row o of an item is the map's row src[o]; rows past the item's total keep their bits
__global__ __launch_bounds__(kFT) void fuse_gather_desc_kernel(const int32_t *off, const int32_t *src, const uint4 *desc_in, uint4 *desc_out,
                                                               int P, int O) {
    const int b = blockIdx.y, idx = blockIdx.x * kFT + threadIdx.x, o = idx >> 1, half = idx & 1;
    const int total = min(max(off[(size_t)b * (P + 1) + P], 0), O);
    if (o >= total) return;
    const int from = src[(size_t)b * O + o];
    desc_out[((size_t)b * O + o) * 2 + half] = desc_in[((size_t)b * O + from) * 2 + half];
}

// behind a fusion with d_mask = d_fuse_to: the newly absorbed points' rows, and the new d_fuse_to
__global__ __launch_bounds__(kFT) void world_fuse_apply_kernel(const int32_t *fresh, int32_t *fuse_to, float *world_points, int P) {
    const int b = blockIdx.y, i = blockIdx.x * kFT + threadIdx.x;
    if (i >= P) return;
    const size_t at = (size_t)b * P + i;
    const int was = fuse_to[at], now = fresh[at];
    if (now >= 0 && now != i && was == i) nan_row(world_points + at * 4);
    fuse_to[at] = now;
}

// camera f = recorded frame f, from d_Twc as include/vslam_adjust.h forms "camera c"
__global__ __launch_bounds__(kFT) void world_cameras_kernel(const double *Twc, int max_frames, int frames, double *R, double *T, int32_t *n_cams) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) n_cams[b] = frames;
    for (int f = threadIdx.x; f < frames; f += kFT) {
        const double *M = Twc + ((size_t)b * max_frames + f) * 16;
        double *Rf = R + ((size_t)b * max_frames + f) * 9, *Tf = T + ((size_t)b * max_frames + f) * 3;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) Rf[3 * r + c] = M[4 * c + r];
            Tf[r] = -((M[r] * M[3] + M[4 + r] * M[7]) + M[8 + r] * M[11]);
        }
    }
}

// behind the cull: a culled point gets -1 and a NaN row, every point whose survivor was culled gets -1.  `keep` is read, d_fuse_to
// is written at the lane's own index only.
__global__ __launch_bounds__(kFT) void world_cull_apply_kernel(const int32_t *keep, int32_t *fuse_to, float *world_points, int P) {
    const int b = blockIdx.y, i = blockIdx.x * kFT + threadIdx.x;
    if (i >= P) return;
    const size_t at = (size_t)b * P + i;
    const int to = fuse_to[at];
    if (keep[at] == 0) {
        nan_row(world_points + at * 4);
        fuse_to[at] = -1;
    } else if (to >= 0 && to != i && to < P && keep[(size_t)b * P + to] == 0) {
        fuse_to[at] = -1;
    }
}

// the arena slots, the fill of the cells and the launch; everything has been checked
int launch_fuse(vslam_ctx *ctx, FuseArgs a, int batch) {
    const size_t cells = sizeof(int32_t) * (size_t)batch * a.cam_stride * a.kp_stride;
    int rc;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "fuse_cells", cells, &ptr))) return rc;
    a.cells = static_cast<int32_t *>(ptr);
    if ((rc = vs_arena_get(ctx, "fuse_work", sizeof(int32_t) * (size_t)batch * 3 * a.pt_stride, &ptr))) return rc;
    a.work = static_cast<int32_t *>(ptr);
    VS_HIP(ctx, hipMemsetAsync(a.cells, 0x7F, cells, ctx->stream));
    {
        VsProfScope ps(ctx, "fuse_points_kernel");
        fuse_points_kernel<<<batch, kFT, 0, ctx->stream>>>(a);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int launch_cull(vslam_ctx *ctx, const CullArgs &a, int batch, const float *h_K) {
    VS_HIP(ctx, hipMemsetAsync(a.stats, 0, sizeof(int32_t) * 4 * (size_t)batch, ctx->stream));
    {
        VsProfScope ps(ctx, "cull_points_kernel");
        cull_points_kernel<<<dim3(vs_div_up(a.pt_stride, kFT), batch), kFT, 0, ctx->stream>>>(a, vs_pack_K(h_K));
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

bool K_finite(const float *h_K) {
    bool ok = true;
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(h_K[k]);
    return ok;
}

// d_fuse_to, made on the first fusion or cull of a world (identity: "no fusion")
int world_fusion_make(vslam_ctx *ctx, vslam_world *world) {
    if (world->fuse_to) return VSLAM_OK;
    void *ptr = nullptr;
    VS_HIP(ctx, hipMalloc(&ptr, sizeof(int32_t) * (size_t)world->tracks * world->map_capacity));
    world->owned.push_back(ptr);
    world->fuse_to = static_cast<int32_t *>(ptr);
    return vs_world_fusion_reset(ctx, world);
}

// The map's CSR fused with d_mask = the world's d_fuse_to, whatever the world's state: the merged CSR into (off, frame, kp), both
// nullable as a pair, the labels into `to` (nullable), the merged rows' descriptors into desc (nullable).
int world_fuse_run(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const vslam_map_arrays &m, int32_t *off, int32_t *frame, int32_t *kp,
                   int32_t *to, int32_t *stats, uint8_t *desc) {
    const size_t T = m.tracks, P = m.map_capacity, O = m.obs_capacity;
    VS_REQUIRE(ctx, m.max_frames <= kMaxCams, VSLAM_ERR_CAPACITY);
    int rc;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_fuse_i32", sizeof(int32_t) * T * ((P + 1) + 5 * O + P), &ptr))) return rc;
    int32_t *log_off = static_cast<int32_t *>(ptr), *log_frame = log_off + T * (P + 1), *log_kp = log_frame + T * O;
    int32_t *tmp_frame = log_kp + T * O, *tmp_kp = tmp_frame + T * O, *src = tmp_kp + T * O, *tmp_to = src + T * O;
    uint8_t *log_desc = nullptr;
    if (desc) {
        if ((rc = vs_arena_get(ctx, "world_fuse_desc", T * O * VSLAM_DESC_BYTES, &ptr))) return rc;
        log_desc = static_cast<uint8_t *>(ptr);
    }
    if ((rc = vslam_map_observations(ctx, map, log_off, log_frame, log_kp))) return rc;
    if (desc && (rc = vslam_map_observation_descriptors(ctx, map, log_off, log_desc))) return rc;
    const int32_t *in_off = log_off, *in_frame = log_frame, *in_kp = log_kp;
    int32_t *ext_src = nullptr;
    if (world->fusion & 4) {   // extras exist (include/vslam_fuse_project.h): the fusion's input is the log with them appended
        if ((rc = vs_arena_get(ctx, "world_fuse_extras", sizeof(int32_t) * T * ((P + 1) + 3 * O + 2 * P), &ptr))) return rc;
        int32_t *ext_off = static_cast<int32_t *>(ptr), *ext_frame = ext_off + T * (P + 1), *ext_kp = ext_frame + T * O;
        ext_src = ext_kp + T * O;
        if ((rc = vs_world_extras_merge(ctx, world, static_cast<const int32_t *>(m.d_sizes), m.map_capacity, m.obs_capacity, log_off, log_frame, log_kp,
                                        ext_off, ext_frame, ext_kp, ext_src, ext_src + T * O)))
            return rc;
        in_off = ext_off; in_frame = ext_frame; in_kp = ext_kp;
    }
    FuseArgs a;
    a.n_points = static_cast<const int32_t *>(m.d_sizes); a.pt_stride = m.map_capacity; a.off = in_off; a.cam = in_frame; a.kp = in_kp;
    a.obs_stride = m.obs_capacity; a.cam_stride = m.max_frames; a.kp_stride = m.kp_stride; a.mask = world->fuse_to;
    a.fuse_to = to ? to : tmp_to; a.out_off = off; a.out_cam = frame ? frame : tmp_frame; a.out_kp = kp ? kp : tmp_kp; a.out_src = src;
    a.stats = stats;
    if ((rc = launch_fuse(ctx, a, m.tracks))) return rc;
    if (desc && ext_src) return vs_world_extras_gather_desc(ctx, world, m.map_capacity, m.obs_capacity, off, src, ext_src, log_desc, desc);
    if (desc) {
        VsProfScope ps(ctx, "fuse_gather_desc_kernel");
        fuse_gather_desc_kernel<<<dim3(vs_div_up(2 * m.obs_capacity, kFT), m.tracks), kFT, 0, ctx->stream>>>(
            off, src, reinterpret_cast<const uint4 *>(log_desc), reinterpret_cast<uint4 *>(desc), m.map_capacity, m.obs_capacity);
        VS_HIP(ctx, hipGetLastError());
    }
    return VSLAM_OK;
}
}  // namespace

int vs_world_fusion_reset(vslam_ctx *ctx, vslam_world *world) {
    world->fusion = 0;
    if (world->n_extra) VS_HIP(ctx, hipMemsetAsync(world->n_extra, 0, sizeof(int32_t) * (size_t)world->tracks, ctx->stream));
    if (!world->fuse_to) return VSLAM_OK;
    fuse_identity_kernel<<<dim3(vs_div_up(world->map_capacity, kFT), world->tracks), kFT, 0, ctx->stream>>>(world->fuse_to, world->map_capacity);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vs_world_fusion_make(vslam_ctx *ctx, vslam_world *world) { return world_fusion_make(ctx, world); }

int vs_world_cameras(vslam_ctx *ctx, vslam_world *world, int max_frames, int frames, double *R, double *T, int32_t *n_cams) {
    world_cameras_kernel<<<world->tracks, kFT, 0, ctx->stream>>>(world->Twc, max_frames, frames, R, T, n_cams);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vs_world_csr(vslam_ctx *ctx, vslam_world *world, vslam_map *map, int32_t *off, int32_t *frame, int32_t *kp, uint8_t *desc) {
    int rc;
    if (!(world->fusion & 1)) {   // no fusion: the map's own lists, by the map's own launches
        if (frame && (rc = vslam_map_observations(ctx, map, off, frame, kp))) return rc;
        if (desc && (rc = vslam_map_observation_descriptors(ctx, map, off, desc))) return rc;
        return VSLAM_OK;
    }
    vslam_map_arrays m;
    if ((rc = vslam_map_view(map, &m))) return rc;
    return world_fuse_run(ctx, world, map, m, off, frame, kp, nullptr, nullptr, desc);
}

extern "C" {

int vslam_cull_params_default(vslam_cull_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->inlier_px = 6.0; out->min_good = 2; out->mature_good = 3; out->mature_age = 3; out->good10 = 5;
    return VSLAM_OK;
}

int vslam_fuse_points(vslam_ctx *ctx, const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets, const int32_t *d_obs_cam,
                      const int32_t *d_obs_kp, int obs_stride, int cam_stride, int kp_stride, const int32_t *d_mask, int batch,
                      int32_t *d_fuse_to, int32_t *d_out_offsets, int32_t *d_out_cam, int32_t *d_out_kp, int32_t *d_out_src,
                      int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_n_points && d_obs_offsets && d_obs_cam && d_obs_kp && d_fuse_to && d_out_offsets && d_out_cam && d_out_kp, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && pt_stride > 0 && obs_stride > 0 && cam_stride > 0 && kp_stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP && cam_stride <= kMaxCams, VSLAM_ERR_CAPACITY);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_points, d_obs_offsets, d_obs_cam, d_obs_kp, d_mask, d_fuse_to, d_out_offsets, d_out_cam, d_out_kp, d_out_src,
                                d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    FuseArgs a;
    a.n_points = d_n_points; a.pt_stride = pt_stride; a.off = d_obs_offsets; a.cam = d_obs_cam; a.kp = d_obs_kp;
    a.obs_stride = obs_stride; a.cam_stride = cam_stride; a.kp_stride = kp_stride; a.mask = d_mask;
    a.fuse_to = d_fuse_to; a.out_off = d_out_offsets; a.out_cam = d_out_cam; a.out_kp = d_out_kp; a.out_src = d_out_src; a.stats = d_stats;
    a.cells = nullptr; a.work = nullptr;
    return launch_fuse(ctx, a, batch);
}

int vslam_cull_points(vslam_ctx *ctx, const float *d_points, const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets,
                      const int32_t *d_obs_cam, const int32_t *d_obs_kp, int obs_stride, const double *d_R, const double *d_T,
                      const int32_t *d_n_cams, int cam_stride, const float *d_xy, int kp_stride, const float *h_K, int batch,
                      const vslam_cull_params *params, int32_t *d_keep, int32_t *d_counts, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_points && d_n_points && d_obs_offsets && d_obs_cam && d_obs_kp && d_R && d_T && d_n_cams && d_xy && h_K && d_keep && d_stats,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && pt_stride > 0 && obs_stride > 0 && cam_stride > 0 && kp_stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP && cam_stride <= kMaxCams, VSLAM_ERR_CAPACITY);
    vslam_cull_params p;
    vslam_cull_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, cull_params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_points, 16);   // float4 rows
    VS_ALIGNED(ctx, d_xy, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_R, d_T) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_points, d_obs_offsets, d_obs_cam, d_obs_kp, d_n_cams, d_keep, d_counts, d_stats) % 4 == 0, VSLAM_ERR_INVALID);
    CullArgs a;
    a.points = reinterpret_cast<const float4 *>(d_points); a.n_points = d_n_points; a.pt_stride = pt_stride;
    a.off = d_obs_offsets; a.cam = d_obs_cam; a.kp = d_obs_kp; a.obs_stride = obs_stride;
    a.R = d_R; a.T = d_T; a.n_cams = d_n_cams; a.cam_stride = cam_stride; a.xy = d_xy; a.xy_item = (size_t)cam_stride * kp_stride * 2; a.kp_stride = kp_stride;
    a.prm = fu_cull(p.inlier_px, p.min_good, p.mature_good, p.mature_age, p.good10);
    a.keep = d_keep; a.counts = d_counts; a.stats = d_stats;
    return launch_cull(ctx, a, batch, h_K);
}

int vslam_world_fusion_view(vslam_world *world, int32_t **d_fuse_to, int32_t *state) {
    if (!world || !d_fuse_to) return VSLAM_ERR_INVALID;
    *d_fuse_to = world->fusion ? world->fuse_to : nullptr;
    if (state) *state = world->fusion;
    return VSLAM_OK;
}

int vslam_world_fuse(vslam_ctx *ctx, vslam_world *world, vslam_map *map, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &m))) return rc;
    VS_REQUIRE(ctx, m.max_frames <= kMaxCams, VSLAM_ERR_CAPACITY);
    VS_ALIGNED(ctx, d_stats, 4);
    if ((rc = world_fusion_make(ctx, world))) return rc;
    const size_t T = m.tracks, P = m.map_capacity, O = m.obs_capacity;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_fuse_out", sizeof(int32_t) * T * ((P + 1) + P), &ptr))) return rc;
    int32_t *off = static_cast<int32_t *>(ptr), *fresh = off + T * (P + 1);
    (void)O;
    if ((rc = world_fuse_run(ctx, world, map, m, off, nullptr, nullptr, fresh, d_stats, nullptr))) return rc;
    world_fuse_apply_kernel<<<dim3(vs_div_up(m.map_capacity, kFT), m.tracks), kFT, 0, ctx->stream>>>(fresh, world->fuse_to, world->world_points,
                                                                                                   m.map_capacity);
    VS_HIP(ctx, hipGetLastError());
    world->fusion |= 1;
    return VSLAM_OK;
}

int vslam_world_cull(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy, int xy_frames, const float *h_K,
                     const vslam_cull_params *params, int32_t *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_xy && h_K, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &m))) return rc;
    VS_REQUIRE(ctx, xy_frames >= m.frames, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, m.max_frames <= kMaxCams, VSLAM_ERR_CAPACITY);
    vslam_cull_params p;
    vslam_cull_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, cull_params_ok(p), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, K_finite(h_K), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_xy, 8);
    VS_ALIGNED(ctx, d_stats, 4);
    if ((rc = world_fusion_make(ctx, world))) return rc;
    const size_t T = m.tracks, P = m.map_capacity, O = m.obs_capacity, Fr = m.max_frames;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "world_cull_i32", sizeof(int32_t) * T * ((P + 1) + 2 * O + P + 5), &ptr))) return rc;
    int32_t *off = static_cast<int32_t *>(ptr), *frame = off + T * (P + 1), *kp = frame + T * O, *keep = kp + T * O, *n_cams = keep + T * P,
            *stats = n_cams + T;
    if ((rc = vs_arena_get(ctx, "world_cull_f64", sizeof(double) * T * Fr * 12, &ptr))) return rc;
    double *R = static_cast<double *>(ptr), *Tv = R + T * Fr * 9;
    if ((rc = vs_world_csr(ctx, world, map, off, frame, kp, nullptr))) return rc;
    if ((rc = vs_world_cameras(ctx, world, m.max_frames, m.frames, R, Tv, n_cams))) return rc;
    CullArgs a;
    a.points = reinterpret_cast<const float4 *>(world->world_points); a.n_points = static_cast<const int32_t *>(m.d_sizes); a.pt_stride = m.map_capacity;
    a.off = off; a.cam = frame; a.kp = kp; a.obs_stride = m.obs_capacity;
    a.R = R; a.T = Tv; a.n_cams = n_cams; a.cam_stride = m.max_frames; a.xy = d_xy; a.xy_item = (size_t)xy_frames * m.kp_stride * 2;
    a.kp_stride = m.kp_stride;
    a.prm = fu_cull(p.inlier_px, p.min_good, p.mature_good, p.mature_age, p.good10);
    a.keep = keep; a.counts = nullptr; a.stats = d_stats ? d_stats : stats;
    if ((rc = launch_cull(ctx, a, m.tracks, h_K))) return rc;
    world_cull_apply_kernel<<<dim3(vs_div_up(m.map_capacity, kFT), m.tracks), kFT, 0, ctx->stream>>>(keep, world->fuse_to, world->world_points,
                                                                                                   m.map_capacity);
    VS_HIP(ctx, hipGetLastError());
    world->fusion |= 2;
    return VSLAM_OK;
}

int vslam_world_observations(vslam_ctx *ctx, vslam_world *world, vslam_map *map, int32_t *d_offsets, int32_t *d_frame_ids, int32_t *d_point_ids,
                             uint8_t *d_desc) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_offsets && d_frame_ids && d_point_ids, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &m))) return rc;
    VS_REQUIRE(ctx, vs_ptr_bits(d_offsets, d_frame_ids, d_point_ids) % 4 == 0, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_desc, 16);   // descriptor rows move as uint4 pairs
    return vs_world_csr(ctx, world, map, d_offsets, d_frame_ids, d_point_ids, d_desc);
}

}  // extern "C"
