// RANSAC fundamental-matrix loop, stage 1 of 4: the random sets of 8 matches.
//
// Replaces RansacFilter::initialize_sets (the reference's src/RansacFilter.cpp:6-34):
//   std::mt19937(seed), :12                               -> ransac_mt_kernel     (the raw outputs; they depend on the seed alone)
//   uniform_int_distribution + draw without replacement,
//   :22-31                                                -> ransac_map_kernel<>  (Lemire mapping with rejection, then the sets)
// The stages behind it: ransac_solve.hip (a hypothesis per set), ransac_count.hip (inlier counts), ransac_select.hip (the
// accept rule and the all-sums scoring).
//
// Numerics: integers only.  The sets are the reference's, index for index, for every seed and match count: the generator
// is mt19937 as the standard defines it, the mapping is libstdc++'s (pinned; see ransac_map_kernel).  A pair that would
// need more raw outputs than were generated is reported through the device error word, never read past.
#include "ctx.h"

namespace {

// ------------------------------------------------------------------------------------------
// initialize_sets
// ------------------------------------------------------------------------------------------
constexpr int kSetThreads = 256;
constexpr int kMtN = 624, kMtM = 397;

__device__ __forceinline__ uint32_t mt_twist(uint32_t cur, uint32_t nxt, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7FFFFFFFu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
}
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= (y >> 18);
    return y;
}

// The draws come from two kernels.  The raw mt19937 outputs depend on the seed alone (ransac_mt_kernel: one workgroup per
// frame pair, the 624-word state in LDS, a block of 624 outputs per three dependency phases i < 227 | 227 <= i < 454 |
// i >= 454), so the batched front-end produces them on the auxiliary stream while the frames are still being extracted;
// only the mapping to draws, which needs the match count, sits between the matcher and the solver (ransac_map_kernel).
// A pair consumes hyp * 8 raw outputs plus one per Lemire rejection (p ~ n / 2^32 each, i.e. a handful per batch);
// kMtSpare extra outputs are generated, and a pair that would need more raises bit 1 of the context's device error word
// (vslam_ctx_synchronize reports VSLAM_ERR_CAPACITY) instead of reading past them.
constexpr int kMtSpare = kMtN;
static inline int vs_mt_blocks(int hyp) { return (hyp * VSLAM_SET_SIZE + kMtSpare + kMtN - 1) / kMtN; }

__global__ __launch_bounds__(kSetThreads) void ransac_mt_kernel(const uint32_t *__restrict__ seeds, int nblk,
                                                                uint32_t *__restrict__ raw) {
    const int b = blockIdx.x, tid = threadIdx.x;
    uint32_t *R = raw + (size_t)b * nblk * kMtN;
    __shared__ uint32_t mt[kMtN];
    if (tid == 0) {   // std::mt19937(seed) seeding recurrence
        uint32_t x = seeds[b];
        mt[0] = x;
        for (int i = 1; i < kMtN; i++) {
            x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
            mt[i] = x;
        }
    }
    __syncthreads();
    for (int blk = 0; blk < nblk; blk++) {
        uint32_t v = 0;
        if (tid < kMtN - kMtM) v = mt_twist(mt[tid], mt[tid + 1], mt[tid + kMtM]);
        __syncthreads();
        if (tid < kMtN - kMtM) mt[tid] = v;
        __syncthreads();
        const int i1 = tid + (kMtN - kMtM);   // 227 .. 453
        if (tid < kMtN - kMtM) v = mt_twist(mt[i1], mt[i1 + 1], mt[i1 - (kMtN - kMtM)]);
        __syncthreads();
        if (tid < kMtN - kMtM) mt[i1] = v;
        __syncthreads();
        const int i2 = tid + 2 * (kMtN - kMtM);   // 454 .. 623
        if (i2 < kMtN) v = mt_twist(mt[i2], mt[i2 == kMtN - 1 ? 0 : i2 + 1], mt[i2 - (kMtN - kMtM)]);
        __syncthreads();
        if (i2 < kMtN) mt[i2] = v;
        __syncthreads();
        for (int i = tid; i < kMtN; i += kSetThreads) R[(size_t)blk * kMtN + i] = mt_temper(mt[i]);
    }
}

// Mapping of the raw outputs to draws: libstdc++'s uniform_int_distribution<int>(0, size-1) for a 32-bit URBG is Lemire's
// multiply-shift with rejection (bits/uniform_int_dist.h _S_nd); a rejected output is consumed and the same draw retries
// with the next one, so a rejection shifts every later draw by one raw output.  With all outputs in memory every output
// is mapped in parallel under the current count of rejections; the earliest rejected output (if any: p ~ n / 2^32 per
// draw) finalises everything before it, bumps the count, and the pass repeats from there.  Usually one pass, a second
// one for about one pair in a hundred.  Then draws -> indices without replacement: available[r] = available.back();
// pop_back() (RansacFilter.cpp:26-31) tracked as a <= 8-entry sparse overlay on the identity array.
constexpr int kMapThreads = 1024;
// mi = RansacFilter::min_items: the reference draws min_items indices into sets that are 8 wide whatever min_items is
// (src/RansacFilter.cpp:17,22): entries mi .. 7 stay 0, and a hypothesis consumes mi raw outputs (+ rejections).
template <bool EIGHT>   // min_items == 8, the usual case: d & 7, no per-entry test
__global__ __launch_bounds__(kMapThreads) void ransac_map_kernel(const int32_t *__restrict__ m_arr, int hyp, int nblk, int mi_arg,
                                                                 const uint32_t *__restrict__ raw, int32_t *__restrict__ sets,
                                                                 uint32_t *__restrict__ draws, int32_t *__restrict__ errflag) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int mi = EIGHT ? VSLAM_SET_SIZE : mi_arg;
    const int n = m_arr[b];
    int32_t *S = sets + (size_t)b * hyp * VSLAM_SET_SIZE;
    uint32_t *D = draws + (size_t)b * hyp * VSLAM_SET_SIZE;
    const uint32_t *R = raw + (size_t)b * nblk * kMtN;
    const int total = hyp * mi, avail = nblk * kMtN;
    if (n < mi || n < 1 || mi == 0) {   // n < mi is UB in the reference (distribution over (0,-1)); defined here as zeros
        for (int i = tid; i < hyp * VSLAM_SET_SIZE; i += kMapThreads) S[i] = 0;
        return;
    }
    __shared__ int s_first;
    int lo = 0, rej = 0;
    while (true) {
        if (tid == 0) s_first = 0x7FFFFFFF;
        __syncthreads();
        if (total + rej > avail) {   // more rejections than spare outputs: practically unreachable; reported, never read past
            if (tid == 0) atomicOr(errflag, 2);
            for (int d = lo - rej + tid; d < total; d += kMapThreads) D[d] = 0;
            break;
        }
        for (int t = lo + tid; t < total + rej; t += kMapThreads) {
            const int d = t - rej;
            const uint32_t range = (uint32_t)(n - (EIGHT ? (d & 7) : d % mi));
            const uint64_t prod = (uint64_t)R[t] * (uint64_t)range;
            const uint32_t low = (uint32_t)prod;
            if (low < range && low < (0u - range) % range) atomicMin(&s_first, t);   // rejected: consumed, yields no draw
            else D[d] = (uint32_t)(prod >> 32);   // final if t lies before the first rejection, rewritten otherwise
        }
        __syncthreads();
        const int first = s_first;
        if (first == 0x7FFFFFFF) break;
        rej += 1;
        lo = first + 1;
        __syncthreads();
    }
    __syncthreads();
    __threadfence_block();
    for (int h = tid; h < hyp; h += kMapThreads) {
        int pos[VSLAM_SET_SIZE], val[VSLAM_SET_SIZE];
        int cnt = 0, size = n;
#pragma unroll
        for (int j = 0; j < VSLAM_SET_SIZE; j++) {
            if (!EIGHT && j >= mi) {
                S[(size_t)h * VSLAM_SET_SIZE + j] = 0;
                continue;
            }
            const int r = (int)D[(size_t)h * mi + j];
            int v = r, lv = size - 1, slot = -1;
#pragma unroll
            for (int k = 0; k < VSLAM_SET_SIZE; k++) {
                if (k < cnt && pos[k] == r) {
                    v = val[k];
                    slot = k;
                }
                if (k < cnt && pos[k] == size - 1) lv = val[k];
            }
            S[(size_t)h * VSLAM_SET_SIZE + j] = v;
            if (slot >= 0) {
#pragma unroll
                for (int k = 0; k < VSLAM_SET_SIZE; k++)
                    if (k == slot) val[k] = lv;
            } else {
#pragma unroll
                for (int k = 0; k < VSLAM_SET_SIZE; k++)
                    if (k == cnt) {
                        pos[k] = r;
                        val[k] = lv;
                    }
                cnt++;
            }
            size--;
        }
    }
}

}  // namespace

size_t vs_ransac_raw_words(int hyp) { return (size_t)vs_mt_blocks(hyp) * kMtN; }

int vs_launch_ransac_mt(vslam_ctx *ctx, const uint32_t *seeds, int batch, int hyp, uint32_t *raw) {
    VS_REQUIRE(ctx, seeds && raw, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && hyp > 0, VSLAM_ERR_INVALID);
    VsProfScope ps(ctx, "ransac_mt_kernel");
    ransac_mt_kernel<<<batch, kSetThreads, 0, ctx->stream>>>(seeds, vs_mt_blocks(hyp), raw);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vs_launch_ransac_map(vslam_ctx *ctx, const int32_t *m, int batch, int hyp, const uint32_t *raw, int32_t *sets,
                         uint32_t *draws) {
    VS_REQUIRE(ctx, m && raw && sets && draws, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && hyp > 0, VSLAM_ERR_INVALID);
    int32_t *flag = nullptr;
    int rc = vs_device_errflag(ctx, &flag);
    if (rc) return rc;
    VsProfScope ps(ctx, "ransac_sets_kernel");
    if (ctx->ransac_min_items == VSLAM_SET_SIZE)
        ransac_map_kernel<true><<<batch, kMapThreads, 0, ctx->stream>>>(m, hyp, vs_mt_blocks(hyp), VSLAM_SET_SIZE, raw, sets, draws, flag);
    else
        ransac_map_kernel<false><<<batch, kMapThreads, 0, ctx->stream>>>(m, hyp, vs_mt_blocks(hyp), ctx->ransac_min_items, raw, sets,
                                                                         draws, flag);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vs_launch_ransac_sets(vslam_ctx *ctx, const uint32_t *seeds, const int32_t *m, int batch, int hyp,
                          int32_t *sets, uint32_t *draws) {
    VS_REQUIRE(ctx, seeds && m && sets && draws, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && hyp > 0, VSLAM_ERR_INVALID);
    uint32_t *raw = nullptr;
    int rc = vs_arena_get(ctx, "mf.raw", sizeof(uint32_t) * vs_ransac_raw_words(hyp) * (size_t)batch, (void **)&raw);
    if (rc) return rc;
    if ((rc = vs_launch_ransac_mt(ctx, seeds, batch, hyp, raw))) return rc;
    return vs_launch_ransac_map(ctx, m, batch, hyp, raw, sets, draws);
}
