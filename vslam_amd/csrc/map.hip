// Device-resident PointMap for gfx950: what the reference's main loop does BETWEEN frame pairs.
//
// Replaces, for `tracks` independent sequences advanced in lockstep (batch = tracks), the bookkeeping of
// src/vslam.cpp:60-270 and src/PointMap.cpp:3-34: frame.R_t / frame.pose (:83-88), the propagation of map_point_ids through
// the matches (:105-118), the observation pushes of the association loop (:153-156), add_reprojection_inliers and the
// colour pick (:236-251).  The floating-point stages in between are the existing launchers (pose.hip, assoc.hip), fed with
// this state.
//
// Observations live in a chronological per-track LOG: entry = (map point, rank within that map point, frame id, keypoint,
// the keypoint's descriptor).  The rank is fixed when the entry is written, by ordered compaction (match index, map index,
// new-point index), never by the arrival order of atomics; the CSR view that association and vslam_map_observations read is
// position = offsets[map point] + rank, i.e. the reference's push order per map point.
//
// A step works on per-step copies (counts, the current frame's map_point_ids) and publishes them in its last kernel, so a track
// that runs out of map or observation slots anywhere in the step is left exactly as it was.
#include <algorithm>

#include "block_scan.h"
#include "ctx.h"
#include "../../include/vslam_search.h"

struct vslam_map {
    vslam_ctx *ctx = nullptr;
    int tracks = 0, max_frames = 0, kp_stride = 0, map_capacity = 0, obs_capacity = 0;
    int frames = 1;   // frames recorded so far (frame 0 is implicit: identity pose, no ids)
    // state
    float *points = nullptr;      // [tracks][map_capacity][4]
    uint8_t *colors = nullptr;    // [tracks][map_capacity][3]
    int32_t *sizes = nullptr;     // [tracks]
    int32_t *ids = nullptr;       // [tracks][max_frames][kp_stride]
    float *R_t = nullptr;         // [tracks][max_frames][16]
    float *pose = nullptr;        // [tracks][max_frames][16]
    int32_t *obs_cnt = nullptr;   // [tracks][map_capacity] observations per map point
    int32_t *n_obs = nullptr;     // [tracks] log entries
    int32_t *log_map = nullptr, *log_rank = nullptr, *log_frame = nullptr, *log_kp = nullptr;   // [tracks][obs_capacity]
    uint8_t *log_desc = nullptr;  // [tracks][obs_capacity][32]
    // per-step work
    int32_t *cnt_work = nullptr;  // [tracks][map_capacity]
    int32_t *first = nullptr;     // [tracks][map_capacity] lowest unranked match per map point (propagation)
    int32_t *claim = nullptr;     // [tracks][map_capacity]
    int32_t *offsets = nullptr;   // [tracks][map_capacity + 1]
    uint8_t *csr_desc = nullptr;  // [tracks][obs_capacity][32]
    int32_t *n_map_eff = nullptr, *pend = nullptr, *fail = nullptr;   // [tracks]
    int32_t *ids_work = nullptr;  // [tracks][kp_stride] the current frame's map_point_ids
    int32_t *kwin = nullptr, *krank = nullptr;   // [tracks][kp_stride]
    float *R = nullptr, *t = nullptr, *c2 = nullptr, *points4d = nullptr;
    int32_t *inlier_idx = nullptr, *n_inliers = nullptr;
    double *error = nullptr;
    // staging of one frame step of vslam_track_sequences ([tracks][...] views of [tracks][frames][...] arrays)
    float *st_xy[2] = {nullptr, nullptr};
    uint8_t *st_desc[2] = {nullptr, nullptr};
    int32_t *st_n[2] = {nullptr, nullptr};
    int32_t *st_nodes = nullptr, *st_matches = nullptr, *st_best = nullptr;
    float *st_F = nullptr;
    vslam_world *world = nullptr;   // vslam_map_attach_world: stepped and reset with the map
    std::vector<void *> owned;
};

namespace {

constexpr int kMT = 256;   // threads of the per-track kernels: one workgroup per track

__device__ __forceinline__ void copy_desc(uint8_t *dst, const uint8_t *src) {   // 32-byte rows, 16-byte aligned
    const uint4 a = reinterpret_cast<const uint4 *>(src)[0], b = reinterpret_cast<const uint4 *>(src)[1];
    reinterpret_cast<uint4 *>(dst)[0] = a;
    reinterpret_cast<uint4 *>(dst)[1] = b;
}

struct MapDev {   // what the kernels need of vslam_map
    int max_frames, kp_stride, map_capacity, obs_capacity;
    float *points;
    uint8_t *colors;
    int32_t *sizes, *ids;
    float *R_t, *pose;
    int32_t *obs_cnt, *n_obs, *log_map, *log_rank, *log_frame, *log_kp;
    uint8_t *log_desc;
    int32_t *cnt_work, *first, *claim, *offsets;
    uint8_t *csr_desc;
    int32_t *n_map_eff, *pend, *fail, *ids_work, *kwin, *krank;
};

__global__ __launch_bounds__(kMT) void map_reset_kernel(MapDev m) {
    const int b = blockIdx.y;
    const size_t per = (size_t)m.max_frames * m.kp_stride;
    for (size_t i = (size_t)blockIdx.x * kMT + threadIdx.x; i < per; i += (size_t)gridDim.x * kMT) m.ids[b * per + i] = -1;
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < m.max_frames * 16; i += kMT) {
            const float v = ((i & 15) % 5 == 0) ? 1.f : 0.f;
            m.R_t[(size_t)b * m.max_frames * 16 + i] = v;
            m.pose[(size_t)b * m.max_frames * 16 + i] = v;
        }
        if (threadIdx.x == 0) {
            m.sizes[b] = 0;
            m.n_obs[b] = 0;
        }
    }
}

// start of a step: the per-step copies
__global__ __launch_bounds__(kMT) void map_begin_kernel(MapDev m, const int32_t *__restrict__ best) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool active = best[(size_t)b * 4] >= 0;
    const int size = m.sizes[b];
    for (int i = tid; i < size; i += kMT) m.cnt_work[(size_t)b * m.map_capacity + i] = m.obs_cnt[(size_t)b * m.map_capacity + i];
    for (int i = tid; i < m.kp_stride; i += kMT) {
        m.ids_work[(size_t)b * m.kp_stride + i] = -1;   // src/Frame.cpp:73
        m.kwin[(size_t)b * m.kp_stride + i] = -1;
    }
    if (tid == 0) {
        m.n_map_eff[b] = active ? size : 0;
        m.pend[b] = 0;
        m.fail[b] = 0;
    }
}

// frame.R_t = [R | t; 0 0 0 1], frame.pose = last_frame.pose * frame.R_t (src/vslam.cpp:83-88): the 4 x 4 product as OpenCV's
// small GEMM forms it, exact double products summed left to right in double, one rounding.  A pair without a model keeps
// R_t = identity and carries the pose over.
__global__ __launch_bounds__(64) void map_pose_kernel(MapDev m, int tracks, int fid, const int32_t *__restrict__ best,
                                                      const float *__restrict__ R, const float *__restrict__ t) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= tracks) return;
    float *Rt = m.R_t + ((size_t)b * m.max_frames + fid) * 16;
    float *P = m.pose + ((size_t)b * m.max_frames + fid) * 16;
    const float *L = m.pose + ((size_t)b * m.max_frames + fid - 1) * 16;
    if (best[(size_t)b * 4] < 0) {
        for (int i = 0; i < 16; i++) {
            Rt[i] = (i % 5 == 0) ? 1.f : 0.f;
            P[i] = L[i];
        }
        return;
    }
    float A[16];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) A[r * 4 + c] = R[(size_t)b * 9 + r * 3 + c];
        A[r * 4 + 3] = t[(size_t)b * 3 + r];
    }
    A[12] = A[13] = A[14] = 0.f;
    A[15] = 1.f;
    for (int i = 0; i < 16; i++) Rt[i] = A[i];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const double s0 = (double)L[r * 4 + 0] * (double)A[0 * 4 + c], s1 = (double)L[r * 4 + 1] * (double)A[1 * 4 + c];
            const double s2 = (double)L[r * 4 + 2] * (double)A[2 * 4 + c], s3 = (double)L[r * 4 + 3] * (double)A[3 * 4 + c];
            P[r * 4 + c] = (float)(((s0 + s1) + s2) + s3);
        }
}

// src/vslam.cpp:105-118 for one track per workgroup.  Match k with id = last.map_point_ids[m.first] > 0 (map point 0 is never
// propagated) gives cur.map_point_ids[m.second] = id -- the LATER of two matches onto one m.second wins -- and pushes the
// observation (frame, m.second) onto map point id, every such match, in match order.
__global__ __launch_bounds__(kMT) void map_propagate_kernel(MapDev m, int fid, const int32_t *__restrict__ best,
                                                            const int32_t *__restrict__ matches,
                                                            const uint8_t *__restrict__ desc_cur,
                                                            const int32_t *__restrict__ n_last, const int32_t *__restrict__ n_cur) {
    __shared__ int lds[kMT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = m.kp_stride;
    const bool active = best[(size_t)b * 4] >= 0;
    const int n = active ? min(max(best[(size_t)b * 4 + 3], 0), K) : 0;
    const int size = m.sizes[b];
    const int2 *M = reinterpret_cast<const int2 *>(matches) + (size_t)b * K;
    const int32_t *last = m.ids + ((size_t)b * m.max_frames + fid - 1) * K;
    int32_t *cur = m.ids_work + (size_t)b * K;
    int32_t *kwin = m.kwin + (size_t)b * K, *krank = m.krank + (size_t)b * K;
    int32_t *first = m.first + (size_t)b * m.map_capacity, *cnt = m.cnt_work + (size_t)b * m.map_capacity;

    // which matches push, and the winner per current keypoint
    int mine = 0;
    for (int k = tid; k < n; k += kMT) {
        const int2 mt = M[k];
        int id = -1;
        if (mt.x >= 0 && mt.x < min(n_last[b], K) && mt.y >= 0 && mt.y < min(n_cur[b], K)) id = last[mt.x];   // keypoints the frames hold
        const bool push = id > 0 && id < size;
        krank[k] = push ? -1 : -2;   // -1: pushes, rank not known yet
        if (push) {
            atomicMax(&kwin[mt.y], k);
            mine++;
        }
    }
    int total;
    vs_block_excl_scan<kMT>(mine, lds, total);
    const int base = m.n_obs[b];
    if (base + total > m.obs_capacity) {   // nothing partial: the whole step of this track is dropped
        if (tid == 0) {
            m.fail[b] = 1;
            m.n_map_eff[b] = 0;
        }
        return;
    }
    if (total == 0) return;
    for (int k = tid; k < n; k += kMT) {
        if (krank[k] != -1) continue;
        const int2 mt = M[k];
        if (kwin[mt.y] == k) cur[mt.y] = last[mt.x];
    }
    // rank inside the map point's list: round r ranks, per map point, its lowest match not ranked yet
    for (int r = 0;; r++) {
        for (int k = tid; k < n; k += kMT)
            if (krank[k] == -1) first[last[M[k].x]] = 0x7FFFFFFF;
        __syncthreads();
        for (int k = tid; k < n; k += kMT)
            if (krank[k] == -1) atomicMin(&first[last[M[k].x]], k);
        __syncthreads();
        int left = 0;
        for (int k = tid; k < n; k += kMT) {
            if (krank[k] != -1) continue;
            const int id = last[M[k].x];
            if (first[id] == k) krank[k] = cnt[id] + r;
            else left = 1;
        }
        if (!__syncthreads_or(left)) break;
    }
    // ordered compaction by match index
    int run = base;
    for (int k0 = 0; k0 < n; k0 += kMT) {
        const int k = k0 + tid;
        const bool push = k < n && krank[k] >= 0;
        int chunk;
        const int pos = run + vs_block_excl_scan<kMT>(push ? 1 : 0, lds, chunk);
        run += chunk;
        if (push) {
            const int2 mt = M[k];
            const int id = last[mt.x];
            const size_t e = (size_t)b * m.obs_capacity + pos;
            m.log_map[e] = id;
            m.log_rank[e] = krank[k];
            m.log_frame[e] = fid;
            m.log_kp[e] = mt.y;
            copy_desc(m.log_desc + e * VSLAM_DESC_BYTES, desc_cur + ((size_t)b * K + mt.y) * VSLAM_DESC_BYTES);
        }
    }
    __syncthreads();
    for (int k = tid; k < n; k += kMT)
        if (krank[k] >= 0) atomicAdd(&cnt[last[M[k].x]], 1);   // a sum: the order does not show
    if (tid == 0) m.pend[b] = total;
}

// offsets[i] = sum of cnt[0 .. i) for i <= n[b]; the rest of the row (to `fill_to`) repeats the total when asked for
__global__ __launch_bounds__(kMT) void map_offsets_kernel(const int32_t *__restrict__ cnt, const int32_t *__restrict__ n_all,
                                                          int map_capacity, int fill_to, int32_t *__restrict__ offsets) {
    __shared__ int lds[kMT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(n_all[b], map_capacity);
    const int32_t *c = cnt + (size_t)b * map_capacity;
    int32_t *o = offsets + (size_t)b * (map_capacity + 1);
    int run = 0;
    for (int i0 = 0; i0 < n; i0 += kMT) {
        const int i = i0 + tid;
        const int v = i < n ? c[i] : 0;
        int chunk;
        const int ex = vs_block_excl_scan<kMT>(v, lds, chunk);
        if (i < n) o[i] = run + ex;
        run += chunk;
    }
    for (int i = n + tid; i <= max(n, fill_to); i += kMT) o[i] = run;
}

// log -> CSR: entry e lands at offsets[map point] + rank.  Two lanes per entry (a 32-byte descriptor = two uint4).
__global__ __launch_bounds__(kMT) void map_csr_kernel(MapDev m, const int32_t *__restrict__ n_entries_extra,
                                                      const int32_t *__restrict__ n_map, const int32_t *__restrict__ offsets,
                                                      uint8_t *__restrict__ csr_desc, int32_t *__restrict__ csr_frame,
                                                      int32_t *__restrict__ csr_kp) {
    const int b = blockIdx.y;
    const int g = blockIdx.x * kMT + threadIdx.x;
    const int e = g >> 1, half = g & 1;
    if (n_map[b] <= 0) return;
    const int n = min(m.n_obs[b] + (n_entries_extra ? n_entries_extra[b] : 0), m.obs_capacity);
    if (e >= n) return;
    const size_t src = (size_t)b * m.obs_capacity + e;
    const int id = m.log_map[src];
    if (id < 0 || id >= m.map_capacity) return;
    const int pos = offsets[(size_t)b * (m.map_capacity + 1) + id] + m.log_rank[src];
    if (pos < 0 || pos >= m.obs_capacity) return;
    const size_t dst = (size_t)b * m.obs_capacity + pos;
    if (csr_desc)
        reinterpret_cast<uint4 *>(csr_desc + dst * VSLAM_DESC_BYTES)[half] =
            reinterpret_cast<const uint4 *>(m.log_desc + src * VSLAM_DESC_BYTES)[half];
    if (csr_frame && half == 0) {
        csr_frame[dst] = m.log_frame[src];
        csr_kp[dst] = m.log_kp[src];
    }
}

// src/vslam.cpp:153-156: every claim of the association pushes (frame, keypoint) onto its map point, in map order
__global__ __launch_bounds__(kMT) void map_assoc_push_kernel(MapDev m, int fid, const uint8_t *__restrict__ desc_cur) {
    __shared__ int lds[kMT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(m.n_map_eff[b], m.map_capacity);   // 0 for a track without a model or already dropped
    if (n <= 0) return;
    const int K = m.kp_stride;
    const int32_t *claim = m.claim + (size_t)b * m.map_capacity;
    int32_t *cnt = m.cnt_work + (size_t)b * m.map_capacity;
    int mine = 0;
    for (int i = tid; i < n; i += kMT) mine += (claim[i] >= 0 && claim[i] < K) ? 1 : 0;
    int total;
    vs_block_excl_scan<kMT>(mine, lds, total);
    const int base = m.n_obs[b] + m.pend[b];
    if (base + total > m.obs_capacity) {
        if (tid == 0) m.fail[b] = 1;
        return;
    }
    int run = base;
    for (int i0 = 0; i0 < n; i0 += kMT) {
        const int i = i0 + tid;
        const int kp = i < n ? claim[i] : -1;
        const bool push = kp >= 0 && kp < K;
        int chunk;
        const int pos = run + vs_block_excl_scan<kMT>(push ? 1 : 0, lds, chunk);
        run += chunk;
        if (push) {
            const size_t e = (size_t)b * m.obs_capacity + pos;
            m.log_map[e] = i;
            m.log_rank[e] = cnt[i];
            cnt[i] += 1;
            m.log_frame[e] = fid;
            m.log_kp[e] = kp;
            copy_desc(m.log_desc + e * VSLAM_DESC_BYTES, desc_cur + ((size_t)b * K + kp) * VSLAM_DESC_BYTES);
        }
    }
    if (tid == 0) m.pend[b] += total;
}

// add_reprojection_inliers (src/PointMap.cpp:3-34) + the colour pick (src/vslam.cpp:247), then the step is published:
// kept match j becomes map point size + j = (x, y, z, 1) with the observations (last frame, m.first), (frame, m.second) and the
// colour image.at(int(x2), int(y2)) -- ROW int(x2), COLUMN int(y2), as the reference writes it; (0, 0, 0) where that lies
// outside the image.
__global__ __launch_bounds__(kMT) void map_append_kernel(MapDev m, int fid, const int32_t *__restrict__ best,
                                                         const int32_t *__restrict__ matches, const float *__restrict__ xy_cur,
                                                         const uint8_t *__restrict__ desc_last, const uint8_t *__restrict__ desc_cur,
                                                         const float *__restrict__ points4d, const int32_t *__restrict__ inlier_idx,
                                                         const int32_t *__restrict__ n_inliers, const uint8_t *__restrict__ bgr,
                                                         size_t bgr_track_stride, int img_w, int img_h, int row_stride,
                                                         int32_t *__restrict__ errflag) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = m.kp_stride;
    const bool active = best[(size_t)b * 4] >= 0;
    int32_t *row = m.ids + ((size_t)b * m.max_frames + fid) * K;
    if (!active) return;   // the map is untouched; R_t / pose were written by map_pose_kernel, the ids row stays -1
    const int size = m.sizes[b], k = min(max(n_inliers[b], 0), K);
    const int base = m.n_obs[b] + m.pend[b];
    const bool fail = m.fail[b] || size + k > m.map_capacity || base + 2 * k > m.obs_capacity;
    if (fail) {   // dropped like a pair without a model, and reported
        float *Rt = m.R_t + ((size_t)b * m.max_frames + fid) * 16, *P = m.pose + ((size_t)b * m.max_frames + fid) * 16;
        const float *L = m.pose + ((size_t)b * m.max_frames + fid - 1) * 16;
        if (tid < 16) {
            Rt[tid] = (tid % 5 == 0) ? 1.f : 0.f;
            P[tid] = L[tid];
        }
        if (tid == 0) atomicOr(errflag, 1);
        return;
    }
    const int2 *M = reinterpret_cast<const int2 *>(matches) + (size_t)b * K;
    const uint8_t *img = bgr + (size_t)b * bgr_track_stride;
    for (int j = tid; j < k; j += kMT) {
        const int r = inlier_idx[(size_t)b * K + j];
        if (r < 0 || r >= K) continue;
        const int2 mt = M[r];
        if (mt.x < 0 || mt.x >= K || mt.y < 0 || mt.y >= K) continue;
        const float4 P = reinterpret_cast<const float4 *>(points4d)[(size_t)b * K + r];
        const size_t p = (size_t)b * m.map_capacity + size + j;
        reinterpret_cast<float4 *>(m.points)[p] = make_float4(P.x, P.y, P.z, 1.f);
        const float2 q = reinterpret_cast<const float2 *>(xy_cur)[(size_t)b * K + mt.y];
        const int ir = (int)q.x, ic = (int)q.y;
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (ir >= 0 && ir < img_h && ic >= 0 && ic < img_w) {
            const uint8_t *px = img + (size_t)ir * row_stride + (size_t)ic * 3;
            c0 = px[0];
            c1 = px[1];
            c2 = px[2];
        }
        m.colors[p * 3 + 0] = c0;
        m.colors[p * 3 + 1] = c1;
        m.colors[p * 3 + 2] = c2;
        const size_t e = (size_t)b * m.obs_capacity + base + 2 * j;
        m.log_map[e] = size + j;
        m.log_rank[e] = 0;
        m.log_frame[e] = fid - 1;
        m.log_kp[e] = mt.x;
        copy_desc(m.log_desc + e * VSLAM_DESC_BYTES, desc_last + ((size_t)b * K + mt.x) * VSLAM_DESC_BYTES);
        m.log_map[e + 1] = size + j;
        m.log_rank[e + 1] = 1;
        m.log_frame[e + 1] = fid;
        m.log_kp[e + 1] = mt.y;
        copy_desc(m.log_desc + (e + 1) * VSLAM_DESC_BYTES, desc_cur + ((size_t)b * K + mt.y) * VSLAM_DESC_BYTES);
        m.obs_cnt[p] = 2;
    }
    // publish
    for (int i = tid; i < size; i += kMT) m.obs_cnt[(size_t)b * m.map_capacity + i] = m.cnt_work[(size_t)b * m.map_capacity + i];
    for (int i = tid; i < K; i += kMT) row[i] = m.ids_work[(size_t)b * K + i];
    __syncthreads();
    if (tid == 0) {
        m.sizes[b] = size + k;
        m.n_obs[b] = base + 2 * k;
    }
}

__global__ void map_flag_kernel(int32_t *errflag) { atomicOr(errflag, 1); }

// rows of `words` uint32 from a pitched source into a packed destination
__global__ __launch_bounds__(kMT) void map_rows_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, size_t words,
                                                       size_t src_pitch_words) {
    const int b = blockIdx.y;
    for (size_t i = (size_t)blockIdx.x * kMT + threadIdx.x; i < words; i += (size_t)gridDim.x * kMT)
        dst[b * words + i] = src[b * src_pitch_words + i];
}

// seeds [tracks][frames - 1] -> [tracks * frames - 1] for the flattened frame run (a pair that straddles two tracks gets 0)
__global__ __launch_bounds__(kMT) void map_seeds_kernel(const uint32_t *__restrict__ seeds, int tracks, int frames,
                                                        uint32_t *__restrict__ flat) {
    const int i = blockIdx.x * kMT + threadIdx.x;
    if (i >= tracks * frames - 1) return;
    const int t = i / frames, f = i - t * frames;
    flat[i] = f < frames - 1 ? seeds[(size_t)t * (frames - 1) + f] : 0u;
}

MapDev dev_of(const vslam_map *m) {
    MapDev d;
    d.max_frames = m->max_frames; d.kp_stride = m->kp_stride; d.map_capacity = m->map_capacity; d.obs_capacity = m->obs_capacity;
    d.points = m->points; d.colors = m->colors; d.sizes = m->sizes; d.ids = m->ids; d.R_t = m->R_t; d.pose = m->pose;
    d.obs_cnt = m->obs_cnt; d.n_obs = m->n_obs; d.log_map = m->log_map; d.log_rank = m->log_rank; d.log_frame = m->log_frame;
    d.log_kp = m->log_kp; d.log_desc = m->log_desc; d.cnt_work = m->cnt_work; d.first = m->first; d.claim = m->claim;
    d.offsets = m->offsets; d.csr_desc = m->csr_desc; d.n_map_eff = m->n_map_eff; d.pend = m->pend; d.fail = m->fail;
    d.ids_work = m->ids_work; d.kwin = m->kwin; d.krank = m->krank;
    return d;
}

template <typename T>
int map_alloc(vslam_ctx *ctx, vslam_map *m, T **out, size_t count) {
    void *p = nullptr;
    VS_HIP(ctx, hipMalloc(&p, sizeof(T) * (count ? count : 1)));
    m->owned.push_back(p);
    *out = static_cast<T *>(p);
    return VSLAM_OK;
}

int map_copy_rows(vslam_ctx *ctx, void *dst, const void *src, size_t row_bytes, size_t src_pitch_bytes, int rows) {
    const size_t words = row_bytes / 4;
    const int blocks = (int)std::min<size_t>((words + kMT - 1) / kMT, 1024);
    map_rows_kernel<<<dim3(blocks ? blocks : 1, rows), kMT, 0, ctx->stream>>>(static_cast<uint32_t *>(dst), static_cast<const uint32_t *>(src),
                                                                            words, src_pitch_bytes / 4);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

// one iteration of src/vslam.cpp:60-270 for every track; features / matches are [tracks][...] arrays
int map_step(vslam_ctx *ctx, vslam_map *m, const float *xy_last, const uint8_t *desc_last, const int32_t *n_last,
             const float *xy_cur, const uint8_t *desc_cur, const int32_t *nodes_cur, const int32_t *n_cur, const int32_t *matches,
             const int32_t *best, const float *F, const uint8_t *bgr_cur, size_t bgr_track_stride, int width, int height,
             int row_stride, const float *h_K, float radius, uint32_t dist_threshold, float reproj_threshold_sq) {
    int32_t *errflag = nullptr;
    int rc;
    if ((rc = vs_device_errflag(ctx, &errflag))) return rc;
    if (m->frames >= m->max_frames) {   // no slot for this frame: nothing happens to any track
        map_flag_kernel<<<1, 1, 0, ctx->stream>>>(errflag);
        VS_HIP(ctx, hipGetLastError());
        return VSLAM_OK;
    }
    const int T = m->tracks, fid = m->frames;
    const MapDev d = dev_of(m);
    if (m->world && (rc = vs_world_before_map_step(ctx, m->world, m->sizes))) return rc;
    {
        VsProfScope ps(ctx, "map_begin_kernel");
        map_begin_kernel<<<T, kMT, 0, ctx->stream>>>(d, best);
    }
    if ((rc = vs_launch_extract_Rt(ctx, F, best, T, h_K, m->R, m->t, m->c2))) return rc;
    const bool refine = ctx->pose_refine;
    if (refine) {   // VSLAM_OPT_POSE_REFINE: the pose entered into the map, association, the filter and the append see the adjusted values
        if ((rc = vs_launch_triangulate(ctx, xy_last, xy_cur, matches, best, T, m->kp_stride, h_K, m->c2, m->points4d))) return rc;
        if ((rc = vs_launch_refine_pairs(ctx, xy_last, xy_cur, matches, best, T, m->kp_stride, h_K, 4.f * reproj_threshold_sq,
                                         kVsPoseRefineIterations, m->R, m->t, m->c2, m->points4d, nullptr)))
            return rc;
    }
    {
        VsProfScope ps(ctx, "map_pose_kernel");
        map_pose_kernel<<<vs_div_up(T, 64), 64, 0, ctx->stream>>>(d, T, fid, best, m->R, m->t);
    }
    {
        VsProfScope ps(ctx, "map_propagate_kernel");
        map_propagate_kernel<<<T, kMT, 0, ctx->stream>>>(d, fid, best, matches, desc_cur, n_last, n_cur);
    }
    {
        VsProfScope ps(ctx, "map_offsets_kernel");
        map_offsets_kernel<<<T, kMT, 0, ctx->stream>>>(m->cnt_work, m->n_map_eff, m->map_capacity, 0, m->offsets);
    }
    {
        VsProfScope ps(ctx, "map_csr_kernel");
        map_csr_kernel<<<dim3(vs_div_up(2 * m->obs_capacity, kMT), T), kMT, 0, ctx->stream>>>(d, m->pend, m->n_map_eff, m->offsets,
                                                                                           m->csr_desc, nullptr, nullptr);
    }
    VS_HIP(ctx, hipGetLastError());
    if ((rc = vs_launch_associate(ctx, m->points, m->n_map_eff, T, m->map_capacity, m->c2, width, height, nodes_cur, xy_cur,
                                  desc_cur, n_cur, m->kp_stride, m->offsets, m->csr_desc, m->obs_capacity, radius, dist_threshold,
                                  m->ids_work, m->claim)))
        return rc;
    {
        VsProfScope ps(ctx, "map_assoc_push_kernel");
        map_assoc_push_kernel<<<T, kMT, 0, ctx->stream>>>(d, fid, desc_cur);
    }
    if (!refine && (rc = vs_launch_triangulate(ctx, xy_last, xy_cur, matches, best, T, m->kp_stride, h_K, m->c2, m->points4d))) return rc;
    if ((rc = vs_launch_reproj_filter(ctx, m->points4d, xy_last, xy_cur, matches, best, T, m->kp_stride, h_K, m->c2, m->ids_work,
                                      reproj_threshold_sq, m->inlier_idx, m->n_inliers, m->error)))
        return rc;
    {
        VsProfScope ps(ctx, "map_append_kernel");
        map_append_kernel<<<T, kMT, 0, ctx->stream>>>(d, fid, best, matches, xy_cur, desc_last, desc_cur, m->points4d, m->inlier_idx,
                                                      m->n_inliers, bgr_cur, bgr_track_stride, width, height, row_stride, errflag);
    }
    VS_HIP(ctx, hipGetLastError());
    m->frames = fid + 1;
    // the world frame follows on the step's own R, t and points4d; the rows appended above are lifted
    if (m->world && (rc = vs_world_after_map_step(ctx, m->world, matches, best, m->points4d, m->R, m->t, n_last, n_cur, m->points,
                                                  m->sizes, xy_cur, h_K)))
        return rc;
    return VSLAM_OK;
}

}  // namespace

extern "C" {

int vslam_map_destroy(vslam_map *map) {
    if (!map) return VSLAM_ERR_INVALID;
    if (map->ctx) {
        (void)hipSetDevice(map->ctx->device);
        (void)hipStreamSynchronize(map->ctx->stream);
    }
    for (void *p : map->owned) (void)hipFree(p);
    delete map;
    return VSLAM_OK;
}

int vslam_map_reset(vslam_ctx *ctx, vslam_map *map) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, map && map->ctx == ctx, VSLAM_ERR_INVALID);
    const size_t per = (size_t)map->max_frames * map->kp_stride, TM = (size_t)map->tracks * map->map_capacity;
    // defined contents everywhere a view can look
    VS_HIP(ctx, hipMemsetAsync(map->points, 0, sizeof(float) * 4 * TM, ctx->stream));
    VS_HIP(ctx, hipMemsetAsync(map->colors, 0, 3 * TM, ctx->stream));
    VS_HIP(ctx, hipMemsetAsync(map->obs_cnt, 0, sizeof(int32_t) * TM, ctx->stream));
    const int blocks = (int)std::min<size_t>((per + kMT - 1) / kMT, 256);
    map_reset_kernel<<<dim3(blocks, map->tracks), kMT, 0, ctx->stream>>>(dev_of(map));
    VS_HIP(ctx, hipGetLastError());
    map->frames = 1;
    if (map->world) return vslam_world_reset(ctx, map->world);
    return VSLAM_OK;
}

int vslam_map_attach_world(vslam_map *map, vslam_world *world) {
    if (!map || !map->ctx) return VSLAM_ERR_INVALID;
    vslam_ctx *ctx = map->ctx;
    if (!world) {
        map->world = nullptr;
        return VSLAM_OK;
    }
    VS_REQUIRE(ctx, world->ctx == ctx, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, world->tracks == map->tracks && world->max_frames == map->max_frames && world->kp_stride == map->kp_stride,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, world->frames == map->frames, VSLAM_ERR_INVALID);
    const int rc = vs_world_bind(ctx, world, map->map_capacity);
    if (rc != VSLAM_OK) return rc;
    map->world = world;
    return VSLAM_OK;
}

int vslam_map_create(vslam_ctx *ctx, int tracks, int max_frames, int kp_stride, int map_capacity, int obs_capacity,
                     vslam_map **out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, out, VSLAM_ERR_INVALID);
    *out = nullptr;
    VS_REQUIRE(ctx, tracks > 0 && max_frames > 0 && kp_stride > 0 && map_capacity > 0 && obs_capacity > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    VS_REQUIRE(ctx, (size_t)tracks * obs_capacity < ((size_t)1 << 30) && (size_t)tracks * map_capacity < ((size_t)1 << 30),
               VSLAM_ERR_CAPACITY);
    vslam_map *m = new vslam_map;
    m->ctx = ctx;
    m->tracks = tracks; m->max_frames = max_frames; m->kp_stride = kp_stride; m->map_capacity = map_capacity;
    m->obs_capacity = obs_capacity;
    const size_t T = tracks, M = map_capacity, O = obs_capacity, K = kp_stride, Fr = max_frames;
    int rc = VSLAM_OK;
#define MAP_ALLOC(field, count) if (rc == VSLAM_OK) rc = map_alloc(ctx, m, &m->field, (count))
    MAP_ALLOC(points, T * M * 4); MAP_ALLOC(colors, T * M * 3); MAP_ALLOC(sizes, T); MAP_ALLOC(ids, T * Fr * K);
    MAP_ALLOC(R_t, T * Fr * 16); MAP_ALLOC(pose, T * Fr * 16); MAP_ALLOC(obs_cnt, T * M); MAP_ALLOC(n_obs, T);
    MAP_ALLOC(log_map, T * O); MAP_ALLOC(log_rank, T * O); MAP_ALLOC(log_frame, T * O); MAP_ALLOC(log_kp, T * O);
    MAP_ALLOC(log_desc, T * O * VSLAM_DESC_BYTES); MAP_ALLOC(cnt_work, T * M); MAP_ALLOC(first, T * M); MAP_ALLOC(claim, T * M);
    MAP_ALLOC(offsets, T * (M + 1)); MAP_ALLOC(csr_desc, T * O * VSLAM_DESC_BYTES); MAP_ALLOC(n_map_eff, T); MAP_ALLOC(pend, T);
    MAP_ALLOC(fail, T); MAP_ALLOC(ids_work, T * K); MAP_ALLOC(kwin, T * K); MAP_ALLOC(krank, T * K); MAP_ALLOC(R, T * 9);
    MAP_ALLOC(t, T * 3); MAP_ALLOC(c2, T * 12); MAP_ALLOC(points4d, T * K * 4); MAP_ALLOC(inlier_idx, T * K);
    MAP_ALLOC(n_inliers, T); MAP_ALLOC(error, T);
    for (int s = 0; s < 2; s++) {
        MAP_ALLOC(st_xy[s], T * K * 2); MAP_ALLOC(st_desc[s], T * K * VSLAM_DESC_BYTES); MAP_ALLOC(st_n[s], T);
    }
    MAP_ALLOC(st_nodes, T * K); MAP_ALLOC(st_matches, T * K * 2); MAP_ALLOC(st_best, T * 4); MAP_ALLOC(st_F, T * 9);
#undef MAP_ALLOC
    if (rc == VSLAM_OK) {   // scratch the existing launchers skip for a pair without a model
        hipError_t e = hipMemsetAsync(m->c2, 0, sizeof(float) * T * 12, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(m->R, 0, sizeof(float) * T * 9, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(m->t, 0, sizeof(float) * T * 3, ctx->stream);
        if (e != hipSuccess) {
            ctx->err = std::string("vslam_map_create: ") + hipGetErrorString(e);
            rc = VSLAM_ERR_HIP;
        }
    }
    if (rc == VSLAM_OK) rc = vslam_map_reset(ctx, m);
    if (rc != VSLAM_OK) {
        const std::string keep = ctx->err;
        vslam_map_destroy(m);
        ctx->err = keep;
        return rc;
    }
    *out = m;
    return VSLAM_OK;
}

int vslam_map_view(vslam_map *map, vslam_map_arrays *out) {
    if (!map || !out) return VSLAM_ERR_INVALID;
    out->tracks = map->tracks; out->max_frames = map->max_frames; out->kp_stride = map->kp_stride;
    out->map_capacity = map->map_capacity; out->obs_capacity = map->obs_capacity; out->frames = map->frames;
    out->d_points = map->points; out->d_colors = map->colors; out->d_sizes = map->sizes; out->d_map_point_ids = map->ids;
    out->d_R_t = map->R_t; out->d_pose = map->pose; out->d_obs_counts = map->obs_cnt; out->d_n_obs = map->n_obs;
    return VSLAM_OK;
}

int vslam_map_observations(vslam_ctx *ctx, vslam_map *map, int32_t *d_offsets, int32_t *d_frame_ids, int32_t *d_point_ids) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, map && map->ctx == ctx && d_offsets && d_frame_ids && d_point_ids, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_offsets, d_frame_ids, d_point_ids) % 4 == 0, VSLAM_ERR_INVALID);
    const MapDev d = dev_of(map);
    map_offsets_kernel<<<map->tracks, kMT, 0, ctx->stream>>>(map->obs_cnt, map->sizes, map->map_capacity, map->map_capacity, d_offsets);
    map_csr_kernel<<<dim3(vs_div_up(2 * map->obs_capacity, kMT), map->tracks), kMT, 0, ctx->stream>>>(d, nullptr, map->sizes, d_offsets,
                                                                                                   nullptr, d_frame_ids, d_point_ids);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_map_observation_descriptors(vslam_ctx *ctx, vslam_map *map, int32_t *d_offsets, uint8_t *d_desc) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, map && map->ctx == ctx && d_offsets && d_desc, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_offsets, 4);
    VS_ALIGNED(ctx, d_desc, 16);   // descriptor rows move as uint4 pairs
    const MapDev d = dev_of(map);
    map_offsets_kernel<<<map->tracks, kMT, 0, ctx->stream>>>(map->obs_cnt, map->sizes, map->map_capacity, map->map_capacity, d_offsets);
    map_csr_kernel<<<dim3(vs_div_up(2 * map->obs_capacity, kMT), map->tracks), kMT, 0, ctx->stream>>>(d, nullptr, map->sizes, d_offsets,
                                                                                                   d_desc, nullptr, nullptr);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_map_step(vslam_ctx *ctx, vslam_map *map, const float *d_xy_last, const uint8_t *d_desc_last, const int32_t *d_n_last,
                   const float *d_xy_cur, const uint8_t *d_desc_cur, const int32_t *d_nodes_cur, const int32_t *d_n_cur,
                   const int32_t *d_matches, const int32_t *d_best, const float *d_F, const uint8_t *d_bgr_cur, int width,
                   int height, int row_stride, const float *h_K, float radius, uint32_t dist_threshold,
                   float reproj_threshold_sq) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, map && map->ctx == ctx, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_xy_last && d_desc_last && d_n_last && d_xy_cur && d_desc_cur && d_nodes_cur && d_n_cur, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_matches && d_best && d_F && d_bgr_cur && h_K, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, width > 0 && height > 0 && row_stride >= 3 * width, VSLAM_ERR_INVALID);
    // descriptor rows move as uint4 pairs, matches and points as 8-byte pairs; the image is sampled by bytes
    VS_ALIGNED(ctx, d_desc_last, 16);
    VS_ALIGNED(ctx, d_desc_cur, 16);
    VS_ALIGNED(ctx, d_matches, 8);
    VS_ALIGNED(ctx, d_xy_last, 8);
    VS_ALIGNED(ctx, d_xy_cur, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_n_last, d_nodes_cur, d_n_cur, d_best, d_F) % 4 == 0, VSLAM_ERR_INVALID);
    return map_step(ctx, map, d_xy_last, d_desc_last, d_n_last, d_xy_cur, d_desc_cur, d_nodes_cur, d_n_cur, d_matches, d_best, d_F,
                    d_bgr_cur, (size_t)height * row_stride, width, height, row_stride, h_K, radius, dist_threshold,
                    reproj_threshold_sq);
}

int vslam_track_sequences(vslam_ctx *ctx, vslam_map *map, const uint8_t *d_bgr, int frames, int width, int height,
                          int row_stride, const vslam_extract_params *params, const uint32_t *d_seeds, int hyp, float threshold,
                          const float *h_K, float radius, uint32_t dist_threshold, float reproj_threshold_sq, float *d_xy,
                          uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n, int32_t *d_matches, int32_t *d_best, float *d_F) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, map && map->ctx == ctx, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, d_bgr && params && d_seeds && h_K && d_xy && d_desc && d_nodes && d_n && d_matches && d_best && d_F,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, frames >= 2 && width > 0 && height > 0 && row_stride >= 3 * width, VSLAM_ERR_INVALID);
    if (int arc = vs_frontend_aligned(ctx, d_seeds, d_xy, d_desc, d_nodes, d_n, d_matches, d_best, d_F)) return arc;
    const int T = map->tracks, K = map->kp_stride;
    int rc;
    if ((rc = vslam_map_reset(ctx, map))) return rc;
    uint32_t *flat_seeds = nullptr;
    if ((rc = vs_arena_get(ctx, "map.seeds", sizeof(uint32_t) * (size_t)T * frames, (void **)&flat_seeds))) return rc;
    map_seeds_kernel<<<vs_div_up(T * frames, kMT), kMT, 0, ctx->stream>>>(d_seeds, T, frames, flat_seeds);
    VS_HIP(ctx, hipGetLastError());
    if ((rc = vslam_frontend_sequence(ctx, d_bgr, T * frames, width, height, row_stride, params, K, flat_seeds, hyp, threshold,
                                      d_xy, d_desc, d_nodes, d_n, d_matches, d_best, d_F)))
        return rc;
    if (ctx->pose_refit)   // VSLAM_OPT_POSE_REFIT: all pairs at once (pair i = frames i, i + 1 of the flattened row), in place
        if ((rc = vs_launch_refit(ctx, d_xy, d_xy + 2 * (size_t)K, d_matches, d_best, T * frames - 1, K, d_F, d_F, nullptr))) return rc;
    // Frame f of every track as one [tracks][...] batch: the pose and association launchers take items at a stride of one
    // frame, the flattened arrays hold a track's frames side by side.
    const size_t fK = (size_t)frames * K;
    auto stage_frame = [&](int f, int slot) -> int {
        int r;
        if ((r = map_copy_rows(ctx, map->st_xy[slot], d_xy + (size_t)f * K * 2, sizeof(float) * 2 * K, sizeof(float) * 2 * fK, T))) return r;
        if ((r = map_copy_rows(ctx, map->st_desc[slot], d_desc + (size_t)f * K * VSLAM_DESC_BYTES, (size_t)VSLAM_DESC_BYTES * K,
                               (size_t)VSLAM_DESC_BYTES * fK, T)))
            return r;
        return map_copy_rows(ctx, map->st_n[slot], d_n + f, sizeof(int32_t), sizeof(int32_t) * frames, T);
    };
    if ((rc = stage_frame(0, 0))) return rc;
    const size_t img = (size_t)height * row_stride;
    for (int f = 1; f < frames; f++) {
        const int cur = f & 1, last = cur ^ 1;
        if ((rc = stage_frame(f, cur))) return rc;
        if ((rc = map_copy_rows(ctx, map->st_nodes, d_nodes + (size_t)f * K, sizeof(int32_t) * K, sizeof(int32_t) * fK, T))) return rc;
        if ((rc = map_copy_rows(ctx, map->st_matches, d_matches + (size_t)(f - 1) * K * 2, sizeof(int32_t) * 2 * K,
                                sizeof(int32_t) * 2 * fK, T)))
            return rc;
        if ((rc = map_copy_rows(ctx, map->st_best, d_best + (size_t)(f - 1) * 4, sizeof(int32_t) * 4, sizeof(int32_t) * 4 * frames, T)))
            return rc;
        if ((rc = map_copy_rows(ctx, map->st_F, d_F + (size_t)(f - 1) * 9, sizeof(float) * 9, sizeof(float) * 9 * frames, T))) return rc;
        if ((rc = map_step(ctx, map, map->st_xy[last], map->st_desc[last], map->st_n[last], map->st_xy[cur], map->st_desc[cur],
                           map->st_nodes, map->st_n[cur], map->st_matches, map->st_best, map->st_F, d_bgr + (size_t)f * img,
                           (size_t)frames * img, width, height, row_stride, h_K, radius, dist_threshold, reproj_threshold_sq)))
            return rc;
    }
    return VSLAM_OK;
}

}  // extern "C"

// the world attached to the map, or null (adjust.hip: vslam_world_adjust is valid only for that world)
vslam_world *vs_map_world(vslam_map *map) { return map ? map->world : nullptr; }
