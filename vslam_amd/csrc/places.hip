// Place recognition (include/vslam_places.h): words of descriptors, a vocabulary by k-majority, an index of frames and its query.
//   places_spread_kernel     the vocabulary as +-1 E2M1 nibbles, 128 bytes per word, rows padded to a multiple of 32 with the
//                            spread of an all-zero word (+1.0 nibbles)
//   places_assign_kernel     the matcher's arithmetic (match.hip, the FP4 form) with a train side every frame shares: a workgroup owns
//                            256 descriptors of one frame (8 waves x one 32-row operand tile, in registers), the spread words come by
//                            in tiles of 32 through LDS (double buffered), 4 MFMAs per tile and wave, one fma and one max per result
//                            for the running best key, merged over the 32 lanes that hold different words of a row at the end
//   training                 places_start_kernel, then per round spread + assign + a counting sort by word (places_hist_kernel,
//                            places_scan_kernel, places_scatter_kernel) + places_majority_kernel, one wave per word
//   the index                places_entry_kernel (a frame's term counts dense in LDS, two per dword, compacted ascending),
//                            places_scan_kernel (the CSR offsets), places_store_kernel (rows, df, tags, ids)
//   the query                places_norms_kernel (a wave per entry), places_score_kernel (the query's term counts dense in LDS, a
//                            wave per entry walks its sparse row), places_select_kernel (top_k passes of a block-wide first-in-order)
// Integer atomics only (sums: the order of arrival does not matter); no scratch.
#include "ctx.h"
#include "../../include/vslam_places.h"
#include "places_math.h"

using namespace vs_places;

struct vslam_places {
    vslam_ctx *ctx = nullptr;
    int n_words = 0, capacity = 0, max_kp = 0, row_cap = 0;   // row_cap = min(max_kp, n_words): distinct words an entry can have
    int size = 0;
    bool has_vocab = false;
    uint8_t *vocab = nullptr;     // [n_words][32]
    uint8_t *spread = nullptr;    // [n_pad][128]
    int32_t *weights = nullptr;   // [n_words]
    int32_t *df = nullptr;        // [n_words]
    int32_t *offsets = nullptr;   // [capacity + 1]
    int32_t *words = nullptr;     // [capacity x row_cap]
    int32_t *tf = nullptr;        // [capacity x row_cap]
    int32_t *norms = nullptr;     // [capacity]
    int32_t *tags = nullptr;      // [capacity][2]
};

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kPQ = 256;            // descriptors per workgroup of the assignment
constexpr int kPT = 32;             // words per tile
constexpr int kPStride = 144;       // bytes per spread word in LDS: 128 + 16, so that rows spread over the banks
constexpr int kPScale0 = 0x7F7F7F7F;   // E8M0 2^0
constexpr float kPPad = 33554432.f;    // "index" of a column beyond n_words: below every key of a real word
constexpr float kPNone = -67108864.f;  // no candidate yet
constexpr int kPBias = 0x05000000;     // biased integer form of a key for the cross-lane merge: u = kPBias - (int)key > 0
constexpr int kCells = kPlMaxWords / 2;   // dense term counts in LDS: two 16-bit counts per dword (a count is at most 16384)

__device__ __forceinline__ uint32_t spread8_pm1(uint32_t b) {   // 8 bits -> 8 nibbles: 0x2 (+1.0) | bit << 3 (sign)
    uint32_t x = (b | (b << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return (x << 3) | 0x22222222u;
}
__device__ __forceinline__ v4i spread32_pm1(uint32_t w) {       // 32 bits -> 32 nibbles (16 bytes)
    v4i r;
    r.x = (int)spread8_pm1(w & 0xFFu);
    r.y = (int)spread8_pm1((w >> 8) & 0xFFu);
    r.z = (int)spread8_pm1((w >> 16) & 0xFFu);
    r.w = (int)spread8_pm1(w >> 24);
    return r;
}
// v_max_f32 on values that are never NaN: a key is dot x 16384 - index with |dot| <= 256 an exact sum of +-1 products and the index
// at most kPPad; the start value kPNone is finite.  (fmaxf would quiet a signalling NaN first: one more instruction per result.)
__device__ __forceinline__ float max_nonan(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__global__ __launch_bounds__(256) void places_spread_kernel(const uint8_t *__restrict__ vocab, int n_words, int n_pad,
                                                            uint8_t *__restrict__ tx) {
    const int i = blockIdx.x * 256 + threadIdx.x;   // dword i & 7 of row i >> 3
    const int row = i >> 3;
    if (row >= n_pad) return;
    const uint32_t w = row < n_words ? reinterpret_cast<const uint32_t *>(vocab)[i] : 0u;
    *reinterpret_cast<v4i *>(tx + (size_t)row * 128 + (size_t)(i & 7) * 16) = spread32_pm1(w);
}

// n_arr null: every frame has kp_stride descriptors (training: one "frame" of n rows)
__global__ __launch_bounds__(512) void places_assign_kernel(const uint8_t *__restrict__ desc, const int32_t *__restrict__ n_arr,
                                                            int kp_stride, int per_frame, const uint8_t *__restrict__ tx, int n_words,
                                                            int32_t *__restrict__ word, int32_t *__restrict__ dist) {
    const int f = blockIdx.x / per_frame, qt = blockIdx.x - f * per_frame;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = n_arr ? min(max(n_arr[f], 0), kp_stride) : kp_stride;
    const int qbase = qt * kPQ;
    int32_t *word_f = word + (size_t)f * kp_stride;
    int32_t *dist_f = dist ? dist + (size_t)f * kp_stride : nullptr;
    if (qbase >= n) {   // uniform for the whole workgroup: rows at or past the count
        const int q = qbase + tid;
        if (tid < kPQ && q < kp_stride) {
            word_f[q] = -1;
            if (dist_f) dist_f[q] = -1;
        }
        return;
    }

    __shared__ __align__(16) uint8_t s_b[2][kPT * kPStride];
    const uint32_t *q32 = reinterpret_cast<const uint32_t *>(desc) + (size_t)f * kp_stride * 8;
    const int r = lane & 31, half = lane >> 5;
    // A operand: this lane's row of the wave's 32-row tile; step s takes dword 2 s + half of the descriptor
    v8i a[4];
    {
        const int q = min(qbase + wave * 32 + r, n - 1);   // rows past the end repeat the last one (never written)
        const uint2 *qrow = reinterpret_cast<const uint2 *>(q32 + (size_t)q * 8);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint2 w2 = qrow[s];
            const v4i x = spread32_pm1(half ? w2.y : w2.x);
            a[s] = v8i{x.x, x.y, x.z, x.w, 0, 0, 0, 0};
        }
    }
    float k1[16];
#pragma unroll
    for (int g = 0; g < 16; g++) k1[g] = kPNone;

    // staging: a tile is 32 spread rows of 128 bytes = 512 threads x 8 bytes; thread t carries bytes 16 sd + 8 shalf .. + 7 of row srow
    const int st = tid & 255, shalf = tid >> 8, srow = st >> 3, sd = st & 7;
    const uint8_t *txb = tx + (size_t)srow * 128 + sd * 16 + 8 * shalf;
    uint8_t *dst0 = &s_b[0][srow * kPStride + sd * 16 + 8 * shalf];
    // tx holds ntiles x 32 rows: the last tile's rows beyond n_words are the spread of an all-zero word
    const int ntiles = (n_words + kPT - 1) / kPT;
    auto fetch = [&](int tile) -> uint2 { return *reinterpret_cast<const uint2 *>(txb + (size_t)tile * (kPT * 128)); };
    auto put = [&](uint2 v, int buf) { *reinterpret_cast<uint2 *>(dst0 + buf * (kPT * kPStride)) = v; };

    put(fetch(0), 0);
    uint2 w_next = make_uint2(0u, 0u);
    if (ntiles > 1) w_next = fetch(1);
    __syncthreads();
    for (int tile = 0; tile < ntiles; tile++) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) put(w_next, buf ^ 1);   // the other buffer was last read two barriers ago
        if (tile + 2 < ntiles) w_next = fetch(tile + 2);
        const int t = tile * kPT + r;
        const float nidx = t < n_words ? -(float)t : -kPPad;   // a column beyond n_words: below every key of a real word
        v16f acc = v16f{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const uint8_t *src = &s_b[buf][r * kPStride + 16 * half];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const v4i bq = *reinterpret_cast<const v4i *>(src + 32 * s);
            const v8i bv = v8i{bq.x, bq.y, bq.z, bq.w, 0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[s], bv, acc, 4, 4, 0, kPScale0, 0, kPScale0);
        }
#pragma unroll
        for (int g = 0; g < 16; g++) k1[g] = max_nonan(k1[g], __builtin_fmaf(acc[g], kPlKeyScale, nidx));   // key = dot x 16384 - word
        __syncthreads();
    }

    // merge over the 32 lanes of a half (different words of the same rows) on the biased integer form (smaller = better)
#pragma unroll
    for (int g = 0; g < 16; g++) {
        uint32_t x = (uint32_t)(kPBias - (int)k1[g]);
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) x = min(x, (uint32_t)__shfl_xor((int)x, m, 64));
        if (r != g) continue;
        // lane (g, half) writes row (g & 3) + 8 (g >> 2) + 4 half of the wave's tile
        const int q = qbase + wave * 32 + (g & 3) + 8 * (g >> 2) + 4 * half;
        if (q >= kp_stride) continue;
        int d = -1, w = -1;
        if (q < n) pl_key_decode(kPBias - (int)x, d, w);
        word_f[q] = w;
        if (dist_f) dist_f[q] = d;
    }
}

// ---- training
__global__ __launch_bounds__(256) void places_start_kernel(const uint8_t *__restrict__ desc, int n, int n_words, uint8_t *__restrict__ vocab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words * 8) return;
    reinterpret_cast<uint32_t *>(vocab)[i] = reinterpret_cast<const uint32_t *>(desc)[(size_t)pl_start(i >> 3, n, n_words) * 8 + (i & 7)];
}

__global__ __launch_bounds__(256) void places_hist_kernel(const int32_t *__restrict__ word, int n, int32_t *__restrict__ sizes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&sizes[word[i]], 1);
}

// out[i] = base + counts[0] + .. + counts[i - 1] for i = 0 .. N, one workgroup; cursor (or null) [N] = out[0 .. N - 1].  base may be
// out itself (the CSR's running end): it is read before anything is written.
constexpr int kScanT = 1024;
__global__ __launch_bounds__(kScanT) void places_scan_kernel(const int32_t *__restrict__ counts, int N, const int32_t *base,
                                                              int32_t *out, int32_t *__restrict__ cursor) {
    __shared__ int part[kScanT];
    const int tid = threadIdx.x, per = (N + kScanT - 1) / kScanT;
    const int lo = min(tid * per, N), hi = min(lo + per, N);
    const int b0 = base ? base[0] : 0;
    int s = 0;
    for (int i = lo; i < hi; i++) s += counts[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = b0;
        for (int k = 0; k < kScanT; k++) {
            const int c = part[k];
            part[k] = run;
            run += c;
        }
        out[N] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int i = lo; i < hi; i++) {
        const int c = counts[i];
        out[i] = run;
        if (cursor) cursor[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(256) void places_scatter_kernel(const int32_t *__restrict__ word, int n, int32_t *__restrict__ cursor,
                                                             int32_t *__restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) order[atomicAdd(&cursor[word[i]], 1)] = i;
}

// one wave per word: lane l counts bits 4 l .. 4 l + 3 (dword l >> 3) over the word's members
__global__ __launch_bounds__(256) void places_majority_kernel(const uint8_t *__restrict__ desc, const int32_t *__restrict__ start,
                                                              const int32_t *__restrict__ order, int n_words, uint8_t *__restrict__ vocab) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_words) return;   // wave-uniform
    const int lo = start[w], hi = start[w + 1], members = hi - lo;
    if (members <= 0) return;   // a word without members keeps its bits
    const uint32_t *d32 = reinterpret_cast<const uint32_t *>(desc);
    const int dw = lane >> 3, sh = 4 * (lane & 7);
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int m = lo; m < hi; m++) {
        const uint32_t v = d32[(size_t)order[m] * 8 + dw] >> sh;
        c0 += v & 1u;
        c1 += (v >> 1) & 1u;
        c2 += (v >> 2) & 1u;
        c3 += (v >> 3) & 1u;
    }
    uint32_t nib = (pl_majority(c0, members) ? 1u : 0u) | (pl_majority(c1, members) ? 2u : 0u) | (pl_majority(c2, members) ? 4u : 0u) |
                   (pl_majority(c3, members) ? 8u : 0u);
    uint32_t v = nib << sh;
    v |= (uint32_t)__shfl_xor((int)v, 1, 64);
    v |= (uint32_t)__shfl_xor((int)v, 2, 64);
    v |= (uint32_t)__shfl_xor((int)v, 4, 64);
    if ((lane & 7) == 0) reinterpret_cast<uint32_t *>(vocab)[(size_t)w * 8 + dw] = v;
}

// ---- the index
__global__ __launch_bounds__(256) void places_weights_kernel(const int32_t *__restrict__ src, int n_words, int32_t *__restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) dst[i] = src ? pl_weight(src[i]) : 1;
}

// a frame's term counts, dense in LDS (all threads; the counts of words < n_words, cleared first)
__device__ __forceinline__ void dense_tf(uint32_t *hist, const int32_t *__restrict__ word_f, int n, int n_words) {
    const int cells = (n_words + 1) >> 1;
    for (int c = threadIdx.x; c < cells; c += blockDim.x) hist[c] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int w = word_f[i];
        atomicAdd(&hist[w >> 1], 1u << (16 * (w & 1)));
    }
    __syncthreads();
}
__device__ __forceinline__ int tf_of(const uint32_t *hist, int w) { return (int)((hist[w >> 1] >> (16 * (w & 1))) & 0xFFFFu); }

// one workgroup per frame: its distinct words ascending with their counts -> ewords / etf [frames][row_cap], distinct [frames]
__global__ __launch_bounds__(256) void places_entry_kernel(const int32_t *__restrict__ word, const int32_t *__restrict__ n_arr, int kp_stride,
                                                           int n_words, int row_cap, int32_t *__restrict__ ewords, int32_t *__restrict__ etf,
                                                           int32_t *__restrict__ distinct) {
    __shared__ uint32_t hist[kCells];
    __shared__ int part[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(n_arr[f], 0), kp_stride);
    dense_tf(hist, word + (size_t)f * kp_stride, n, n_words);
    const int per = (n_words + 255) / 256, lo = min(tid * per, n_words), hi = min(lo + per, n_words);
    int cnt = 0;
    for (int w = lo; w < hi; w++) cnt += tf_of(hist, w) != 0;
    part[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int k = 0; k < 256; k++) {
            const int c = part[k];
            part[k] = run;
            run += c;
        }
        distinct[f] = run;
    }
    __syncthreads();
    int pos = part[tid];   // at most min(n, n_words) <= row_cap rows in all
    for (int w = lo; w < hi; w++) {
        const int t = tf_of(hist, w);
        if (t) {
            ewords[(size_t)f * row_cap + pos] = w;
            etf[(size_t)f * row_cap + pos] = t;
            pos++;
        }
    }
}

__global__ __launch_bounds__(256) void places_store_kernel(const int32_t *__restrict__ ewords, const int32_t *__restrict__ etf,
                                                           const int32_t *__restrict__ distinct, int row_cap, int size,
                                                           const int32_t *__restrict__ offsets, const int32_t *__restrict__ tags_in,
                                                           int32_t *__restrict__ words, int32_t *__restrict__ tf, int32_t *__restrict__ df,
                                                           int32_t *__restrict__ tags, int32_t *__restrict__ ids) {
    const int f = blockIdx.x, e = size + f;
    const int base = offsets[e], d = distinct[f];
    for (int j = threadIdx.x; j < d; j += 256) {
        const int w = ewords[(size_t)f * row_cap + j];
        words[(size_t)base + j] = w;
        tf[(size_t)base + j] = etf[(size_t)f * row_cap + j];
        atomicAdd(&df[w], 1);
    }
    if (threadIdx.x == 0) {
        tags[2 * (size_t)e] = tags_in ? tags_in[2 * f] : 0;
        tags[2 * (size_t)e + 1] = tags_in ? tags_in[2 * f + 1] : 0;
        ids[f] = e;
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// a wave per entry
__global__ __launch_bounds__(256) void places_norms_kernel(const int32_t *__restrict__ offsets, const int32_t *__restrict__ words,
                                                           const int32_t *__restrict__ tf, const int32_t *__restrict__ weights, int size,
                                                           int32_t *__restrict__ norms) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= size) return;
    int s = 0;
    for (int j = offsets[e] + lane; j < offsets[e + 1]; j += 64) s += weights[words[j]] * tf[j];
    s = wave_sum(s);
    if (lane == 0) norms[e] = s;
}

__device__ __forceinline__ int query_limit(const int32_t *below, int q, int size) { return below ? min(max(below[q], 0), size) : size; }

constexpr int kEPB = 256;   // entries per workgroup of the scoring
// grid (chunks of kEPB entries, queries): score [queries][size] for the entries below the query's limit; chunk 0 writes norm(q)
__global__ __launch_bounds__(256) void places_score_kernel(const int32_t *__restrict__ word, const int32_t *__restrict__ n_arr, int kp_stride,
                                                           int n_words, const int32_t *__restrict__ weights, const int32_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ words, const int32_t *__restrict__ tf, int size,
                                                           const int32_t *__restrict__ below, int32_t *__restrict__ score,
                                                           int32_t *__restrict__ q_norm) {
    __shared__ uint32_t hist[kCells];
    __shared__ int s_norm;
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lim = query_limit(below, q, size);
    const int e0 = blockIdx.x * kEPB, e1 = min(e0 + kEPB, lim);
    if (blockIdx.x != 0 && e0 >= lim) return;   // uniform
    const int n = min(max(n_arr[q], 0), kp_stride);
    const int32_t *word_q = word + (size_t)q * kp_stride;
    if (tid == 0) s_norm = 0;
    dense_tf(hist, word_q, n, n_words);
    if (blockIdx.x == 0) {
        int s = 0;
        for (int i = tid; i < n; i += 256) s += weights[word_q[i]];   // the sum of weight x tf, a descriptor at a time
        s = wave_sum(s);
        if (lane == 0 && s) atomicAdd(&s_norm, s);
        __syncthreads();
        if (tid == 0) q_norm[q] = s_norm;
    }
    for (int e = e0 + wave; e < e1; e += 4) {
        int s = 0;
        for (int j = offsets[e] + lane; j < offsets[e + 1]; j += 64) {
            const int w = words[j];
            s += pl_term(weights[w], tf_of(hist, w), tf[j]);
        }
        s = wave_sum(s);
        if (lane == 0) score[(size_t)q * size + e] = s;
    }
}

// one workgroup per query: top_k times the first candidate in order behind the one before
__global__ __launch_bounds__(256) void places_select_kernel(const int32_t *__restrict__ score, const int32_t *__restrict__ norms,
                                                            const int32_t *__restrict__ q_norm, int size, const int32_t *__restrict__ below,
                                                            int top_k, int32_t *__restrict__ best_id, int32_t *__restrict__ best_score,
                                                            int32_t *__restrict__ best_den) {
    __shared__ int rs[256], rd[256], ri[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int lim = query_limit(below, q, size), nq = q_norm[q];
    int ps = 0, pd = 0, pi = -1;   // the candidate written last
    for (int k = 0; k < top_k; k++) {
        int bs = 0, bd = 0, bi = -1;
        if (k == 0 || pi >= 0) {
            for (int e = tid; e < lim; e += 256) {
                const int s = score[(size_t)q * size + e], d = max(nq, norms[e]);
                if (s <= 0 || d <= 0) continue;
                if (pi >= 0 && !pl_before(ps, pd, pi, s, d, e)) continue;
                if (bi < 0 || pl_before(s, d, e, bs, bd, bi)) {
                    bs = s;
                    bd = d;
                    bi = e;
                }
            }
        }
        rs[tid] = bs;
        rd[tid] = bd;
        ri[tid] = bi;
        __syncthreads();
        for (int m = 128; m > 0; m >>= 1) {
            if (tid < m && ri[tid + m] >= 0 && (ri[tid] < 0 || pl_before(rs[tid + m], rd[tid + m], ri[tid + m], rs[tid], rd[tid], ri[tid]))) {
                rs[tid] = rs[tid + m];
                rd[tid] = rd[tid + m];
                ri[tid] = ri[tid + m];
            }
            __syncthreads();
        }
        ps = rs[0];
        pd = rd[0];
        pi = ri[0];
        __syncthreads();
        if (pi < 0) ps = pd = 0;
        if (tid == 0) {
            best_id[(size_t)q * top_k + k] = pi;
            best_score[(size_t)q * top_k + k] = ps;
            best_den[(size_t)q * top_k + k] = pd;
        }
    }
}

int n_pad_of(int n_words) { return vs_div_up(n_words, kPT) * kPT; }

int launch_spread(vslam_ctx *ctx, const uint8_t *vocab, int n_words, uint8_t *tx) {
    VsProfScope ps(ctx, "places_spread_kernel");
    const int n_pad = n_pad_of(n_words);
    places_spread_kernel<<<vs_div_up(n_pad * 8, 256), 256, 0, ctx->stream>>>(vocab, n_words, n_pad, tx);
    return VSLAM_OK;
}

// rows = descriptors per frame (any positive count: training passes its n)
int launch_assign(vslam_ctx *ctx, const uint8_t *desc, const int32_t *n_arr, int rows, int frames, const uint8_t *tx, int n_words,
                  int32_t *word, int32_t *dist) {
    VsProfScope ps(ctx, "places_assign_kernel");
    const int per_frame = vs_div_up(rows, kPQ);
    places_assign_kernel<<<(unsigned)((size_t)frames * per_frame), 512, 0, ctx->stream>>>(desc, n_arr, rows, per_frame, tx, n_words, word, dist);
    return VSLAM_OK;
}

int frames_args_ok(vslam_ctx *ctx, const uint8_t *d_desc, const int32_t *d_n, int kp_stride, int frames) {
    VS_REQUIRE(ctx, d_desc && d_n, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, frames > 0 && kp_stride > 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, (size_t)frames * vs_div_up(kp_stride, kPQ) < (1u << 31), VSLAM_ERR_CAPACITY);
    VS_ALIGNED(ctx, d_desc, 16);
    VS_ALIGNED(ctx, d_n, 4);
    return VSLAM_OK;
}

int index_ok(vslam_ctx *ctx, vslam_places *idx) {
    VS_REQUIRE(ctx, idx && idx->ctx == ctx, VSLAM_ERR_INVALID);
    return VSLAM_OK;
}

int launch_norms(vslam_ctx *ctx, vslam_places *idx) {
    if (idx->size == 0) return VSLAM_OK;
    VsProfScope ps(ctx, "places_norms_kernel");
    places_norms_kernel<<<vs_div_up(idx->size, 4), 256, 0, ctx->stream>>>(idx->offsets, idx->words, idx->tf, idx->weights, idx->size, idx->norms);
    return VSLAM_OK;
}

}  // namespace

extern "C" {

int vslam_places_assign(vslam_ctx *ctx, const uint8_t *d_desc, const int32_t *d_n, int kp_stride, int frames, const uint8_t *d_vocab,
                        int n_words, int32_t *d_word, int32_t *d_dist) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_vocab && d_word, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, n_words >= 1 && n_words <= VSLAM_PLACES_MAX_WORDS, VSLAM_ERR_INVALID);
    int rc;
    if ((rc = frames_args_ok(ctx, d_desc, d_n, kp_stride, frames))) return rc;
    VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    VS_ALIGNED(ctx, d_vocab, 16);
    VS_REQUIRE(ctx, vs_ptr_bits(d_word, d_dist) % 4 == 0, VSLAM_ERR_INVALID);
    uint8_t *tx = nullptr;
    if ((rc = vs_arena_get(ctx, "places.spread", (size_t)n_pad_of(n_words) * 128, (void **)&tx))) return rc;
    launch_spread(ctx, d_vocab, n_words, tx);
    launch_assign(ctx, d_desc, d_n, kp_stride, frames, tx, n_words, d_word, d_dist);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_places_train(vslam_ctx *ctx, const uint8_t *d_desc, int n, int n_words, int iterations, uint8_t *d_vocab, int32_t *d_sizes) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_desc && d_vocab && d_sizes, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, n_words >= 1 && n_words <= VSLAM_PLACES_MAX_WORDS, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, n >= n_words, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, iterations >= 0 && iterations <= 64, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, n <= VSLAM_PLACES_MAX_TRAIN, VSLAM_ERR_CAPACITY);
    VS_ALIGNED(ctx, d_desc, 16);
    VS_ALIGNED(ctx, d_vocab, 16);
    VS_ALIGNED(ctx, d_sizes, 4);
    VS_REQUIRE(ctx, d_vocab + (size_t)n_words * 32 <= d_desc || d_desc + (size_t)n * 32 <= d_vocab, VSLAM_ERR_INVALID);
    int rc;
    uint8_t *tx = nullptr;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "places.spread", (size_t)n_pad_of(n_words) * 128, (void **)&tx))) return rc;
    if ((rc = vs_arena_get(ctx, "places.train", sizeof(int32_t) * (2 * (size_t)n + 2 * (size_t)n_words + 1), &ptr))) return rc;
    int32_t *word = static_cast<int32_t *>(ptr), *order = word + n, *start = order + n, *cursor = start + n_words + 1;
    {
        VsProfScope ps(ctx, "places_start_kernel");
        places_start_kernel<<<vs_div_up(n_words * 8, 256), 256, 0, ctx->stream>>>(d_desc, n, n_words, d_vocab);
    }
    if (iterations == 0) VS_HIP(ctx, hipMemsetAsync(d_sizes, 0, sizeof(int32_t) * (size_t)n_words, ctx->stream));
    for (int it = 0; it < iterations; it++) {
        launch_spread(ctx, d_vocab, n_words, tx);
        launch_assign(ctx, d_desc, nullptr, n, 1, tx, n_words, word, nullptr);
        VS_HIP(ctx, hipMemsetAsync(d_sizes, 0, sizeof(int32_t) * (size_t)n_words, ctx->stream));
        {
            VsProfScope ps(ctx, "places_hist_kernel");
            places_hist_kernel<<<vs_div_up(n, 256), 256, 0, ctx->stream>>>(word, n, d_sizes);
        }
        {
            VsProfScope ps(ctx, "places_scan_kernel");
            places_scan_kernel<<<1, kScanT, 0, ctx->stream>>>(d_sizes, n_words, nullptr, start, cursor);
        }
        {
            VsProfScope ps(ctx, "places_scatter_kernel");
            places_scatter_kernel<<<vs_div_up(n, 256), 256, 0, ctx->stream>>>(word, n, cursor, order);
        }
        {
            VsProfScope ps(ctx, "places_majority_kernel");
            places_majority_kernel<<<vs_div_up(n_words, 4), 256, 0, ctx->stream>>>(d_desc, start, order, n_words, d_vocab);
        }
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_places_create(vslam_ctx *ctx, int n_words, int capacity, int max_kp, vslam_places **out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, out, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, n_words >= 1 && n_words <= VSLAM_PLACES_MAX_WORDS, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, capacity >= 1 && max_kp >= 1, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, capacity <= VSLAM_PLACES_MAX_ENTRIES && max_kp <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
    const int row_cap = max_kp < n_words ? max_kp : n_words;
    VS_REQUIRE(ctx, (size_t)capacity * row_cap < ((size_t)1 << 31), VSLAM_ERR_CAPACITY);   // the CSR offsets are int32
    vslam_places *p = new vslam_places;
    p->ctx = ctx;
    p->n_words = n_words;
    p->capacity = capacity;
    p->max_kp = max_kp;
    p->row_cap = row_cap;
    const size_t rows = (size_t)capacity * row_cap;
    hipError_t e = hipMalloc((void **)&p->vocab, (size_t)n_words * 32);
    if (e == hipSuccess) e = hipMalloc((void **)&p->spread, (size_t)n_pad_of(n_words) * 128);
    if (e == hipSuccess) e = hipMalloc((void **)&p->weights, sizeof(int32_t) * (size_t)n_words);
    if (e == hipSuccess) e = hipMalloc((void **)&p->df, sizeof(int32_t) * (size_t)n_words);
    if (e == hipSuccess) e = hipMalloc((void **)&p->offsets, sizeof(int32_t) * ((size_t)capacity + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&p->words, sizeof(int32_t) * rows);
    if (e == hipSuccess) e = hipMalloc((void **)&p->tf, sizeof(int32_t) * rows);
    if (e == hipSuccess) e = hipMalloc((void **)&p->norms, sizeof(int32_t) * (size_t)capacity);
    if (e == hipSuccess) e = hipMalloc((void **)&p->tags, sizeof(int32_t) * 2 * (size_t)capacity);
    if (e == hipSuccess) e = hipMemsetAsync(p->vocab, 0, (size_t)n_words * 32, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->df, 0, sizeof(int32_t) * (size_t)n_words, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->offsets, 0, sizeof(int32_t) * ((size_t)capacity + 1), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->norms, 0, sizeof(int32_t) * (size_t)capacity, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->tags, 0, sizeof(int32_t) * 2 * (size_t)capacity, ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string("vslam_places_create: ") + hipGetErrorString(e);
        vslam_places_destroy(ctx, p);
        return VSLAM_ERR_HIP;
    }
    places_weights_kernel<<<vs_div_up(n_words, 256), 256, 0, ctx->stream>>>(nullptr, n_words, p->weights);
    *out = p;
    return VSLAM_OK;
}

int vslam_places_destroy(vslam_ctx *ctx, vslam_places *idx) {
    if (!ctx || !idx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, idx->ctx == ctx, VSLAM_ERR_INVALID);
    (void)hipStreamSynchronize(ctx->stream);
    for (void *p : {(void *)idx->vocab, (void *)idx->spread, (void *)idx->weights, (void *)idx->df, (void *)idx->offsets, (void *)idx->words,
                    (void *)idx->tf, (void *)idx->norms, (void *)idx->tags})
        if (p) (void)hipFree(p);
    delete idx;
    return VSLAM_OK;
}

int vslam_places_reset(vslam_ctx *ctx, vslam_places *idx) {
    if (!ctx) return VSLAM_ERR_INVALID;
    int rc;
    if ((rc = index_ok(ctx, idx))) return rc;
    VS_HIP(ctx, hipMemsetAsync(idx->df, 0, sizeof(int32_t) * (size_t)idx->n_words, ctx->stream));
    VS_HIP(ctx, hipMemsetAsync(idx->offsets, 0, sizeof(int32_t) * ((size_t)idx->capacity + 1), ctx->stream));
    idx->size = 0;
    return VSLAM_OK;
}

int vslam_places_set_weights(vslam_ctx *ctx, vslam_places *idx, const int32_t *d_weights) {
    if (!ctx) return VSLAM_ERR_INVALID;
    int rc;
    if ((rc = index_ok(ctx, idx))) return rc;
    VS_ALIGNED(ctx, d_weights, 4);
    VsProfScope ps(ctx, "places_weights_kernel");
    places_weights_kernel<<<vs_div_up(idx->n_words, 256), 256, 0, ctx->stream>>>(d_weights, idx->n_words, idx->weights);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_places_set_vocabulary(vslam_ctx *ctx, vslam_places *idx, const uint8_t *d_vocab, const int32_t *d_weights) {
    if (!ctx) return VSLAM_ERR_INVALID;
    int rc;
    if ((rc = index_ok(ctx, idx))) return rc;
    VS_REQUIRE(ctx, d_vocab, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, idx->size == 0, VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_vocab, 16);
    VS_ALIGNED(ctx, d_weights, 4);
    VS_HIP(ctx, hipMemcpyAsync(idx->vocab, d_vocab, (size_t)idx->n_words * 32, hipMemcpyDeviceToDevice, ctx->stream));
    launch_spread(ctx, idx->vocab, idx->n_words, idx->spread);
    idx->has_vocab = true;
    return vslam_places_set_weights(ctx, idx, d_weights);
}

int vslam_places_add(vslam_ctx *ctx, vslam_places *idx, const uint8_t *d_desc, const int32_t *d_n, int kp_stride, int frames,
                     const int32_t *d_tags, int32_t *d_ids) {
    if (!ctx) return VSLAM_ERR_INVALID;
    int rc;
    if ((rc = index_ok(ctx, idx))) return rc;
    VS_REQUIRE(ctx, idx->has_vocab && d_ids, VSLAM_ERR_INVALID);
    if ((rc = frames_args_ok(ctx, d_desc, d_n, kp_stride, frames))) return rc;
    VS_REQUIRE(ctx, vs_ptr_bits(d_tags, d_ids) % 4 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= idx->max_kp && (size_t)idx->size + (size_t)frames <= (size_t)idx->capacity, VSLAM_ERR_CAPACITY);
    const int W = idx->n_words, row_cap = kp_stride < W ? kp_stride : W;
    int32_t *word = nullptr;
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "places.word", sizeof(int32_t) * (size_t)frames * kp_stride, (void **)&word))) return rc;
    if ((rc = vs_arena_get(ctx, "places.entry", sizeof(int32_t) * (size_t)frames * (2 * (size_t)row_cap + 1), &ptr))) return rc;
    int32_t *ewords = static_cast<int32_t *>(ptr), *etf = ewords + (size_t)frames * row_cap, *distinct = etf + (size_t)frames * row_cap;
    launch_assign(ctx, d_desc, d_n, kp_stride, frames, idx->spread, W, word, nullptr);
    {
        VsProfScope ps(ctx, "places_entry_kernel");
        places_entry_kernel<<<frames, 256, 0, ctx->stream>>>(word, d_n, kp_stride, W, row_cap, ewords, etf, distinct);
    }
    {
        VsProfScope ps(ctx, "places_scan_kernel");
        places_scan_kernel<<<1, kScanT, 0, ctx->stream>>>(distinct, frames, idx->offsets + idx->size, idx->offsets + idx->size, nullptr);
    }
    {
        VsProfScope ps(ctx, "places_store_kernel");
        places_store_kernel<<<frames, 256, 0, ctx->stream>>>(ewords, etf, distinct, row_cap, idx->size, idx->offsets, d_tags, idx->words, idx->tf,
                                                            idx->df, idx->tags, d_ids);
    }
    VS_HIP(ctx, hipGetLastError());
    idx->size += frames;
    return VSLAM_OK;
}

int vslam_places_query(vslam_ctx *ctx, vslam_places *idx, const uint8_t *d_desc, const int32_t *d_n, int kp_stride, int queries,
                       const int32_t *d_below, int top_k, int32_t *d_best_id, int32_t *d_best_score, int32_t *d_best_den, int32_t *d_q_norm) {
    if (!ctx) return VSLAM_ERR_INVALID;
    int rc;
    if ((rc = index_ok(ctx, idx))) return rc;
    VS_REQUIRE(ctx, idx->has_vocab && d_best_id && d_best_score && d_best_den && d_q_norm, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, top_k >= 1 && top_k <= VSLAM_PLACES_MAX_TOP_K, VSLAM_ERR_INVALID);
    if ((rc = frames_args_ok(ctx, d_desc, d_n, kp_stride, queries))) return rc;
    VS_REQUIRE(ctx, queries <= 65535, VSLAM_ERR_CAPACITY);   // the scoring's grid takes the query as its second dimension
    VS_REQUIRE(ctx, vs_ptr_bits(d_below, d_best_id, d_best_score, d_best_den, d_q_norm) % 4 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, kp_stride <= idx->max_kp, VSLAM_ERR_CAPACITY);
    const int W = idx->n_words, size = idx->size;
    int32_t *word = nullptr, *score = nullptr;
    if ((rc = vs_arena_get(ctx, "places.word", sizeof(int32_t) * (size_t)queries * kp_stride, (void **)&word))) return rc;
    if ((rc = vs_arena_get(ctx, "places.score", sizeof(int32_t) * ((size_t)queries * size + 1), (void **)&score))) return rc;
    launch_assign(ctx, d_desc, d_n, kp_stride, queries, idx->spread, W, word, nullptr);
    launch_norms(ctx, idx);
    {
        VsProfScope ps(ctx, "places_score_kernel");
        const int chunks = size > 0 ? vs_div_up(size, kEPB) : 1;
        places_score_kernel<<<dim3(chunks, queries), 256, 0, ctx->stream>>>(word, d_n, kp_stride, W, idx->weights, idx->offsets, idx->words, idx->tf,
                                                                            size, d_below, score, d_q_norm);
    }
    {
        VsProfScope ps(ctx, "places_select_kernel");
        places_select_kernel<<<queries, 256, 0, ctx->stream>>>(score, idx->norms, d_q_norm, size, d_below, top_k, d_best_id, d_best_score,
                                                               d_best_den);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vslam_places_view(vslam_ctx *ctx, vslam_places *idx, vslam_places_arrays *out) {
    if (!ctx) return VSLAM_ERR_INVALID;
    int rc;
    if ((rc = index_ok(ctx, idx))) return rc;
    VS_REQUIRE(ctx, out, VSLAM_ERR_INVALID);
    launch_norms(ctx, idx);
    VS_HIP(ctx, hipGetLastError());
    out->n_words = idx->n_words;
    out->capacity = idx->capacity;
    out->max_kp = idx->max_kp;
    out->size = idx->size;
    out->d_offsets = idx->offsets;
    out->d_words = idx->words;
    out->d_tf = idx->tf;
    out->d_df = idx->df;
    out->d_norms = idx->norms;
    out->d_tags = idx->tags;
    out->d_weights = idx->weights;
    out->d_vocab = idx->vocab;
    return VSLAM_OK;
}

}  // extern "C"
