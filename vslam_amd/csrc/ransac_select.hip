// RANSAC fundamental-matrix loop, stage 4 of 4: residual sums, the accept rule, the winner's inlier mask.
//
// Replaces, of the reference's src/RansacFilter.cpp:
//   compute_fundamental_residual :105-140, all counts and all sums -> ransac_score_kernel  (VSLAM_OPT_RANSAC_ALL_SUMS only)
//   cv::sum :138, for the hypotheses that tie at the maximum count -> ransac_ties_kernel + ransac_tiesum_kernel
//   find_fundamental :36-67 (the sequential accept rule, :59) and
//   the inlier filter of src/Frame.cpp:96-102                      -> ransac_select_kernel
//   the three closing stages in one launch (the default)           -> ransac_finish_kernel
//
// Numerics: bit-exact.  The winner, its F, its mask and the matches kept are the reference's.  A residual sum is a
// sequential double accumulation in match index order whose float value breaks inlier-count ties (:59, :138).  In the
// all-sums kernel a lane owns a hypothesis and walks the matches in index order, which reproduces that sum with no
// cross-lane reduction; the match coordinates are the same for all 64 lanes, so LDS serves them as broadcasts.  On the
// default path only the hypotheses that can still win get their exact sum (ransac_ties_kernel says which).
#include "ransac_residual.h"

namespace {
using namespace vs_ransac;

constexpr int kScoreThreads = 256;
constexpr int kScoreTile = 1024;   // correspondences per LDS tile (16 B floats + 16 B doubles each: 32 KiB)

// One lane per hypothesis; correspondences gathered once per workgroup into LDS and read back as wave-uniform
// broadcasts, two at a time: corr[2j] = (x1a, x1b, y1a, y1b), corr[2j+1] = (x2a, x2b, y2a, y2b) for the
// correspondences a = 2j, b = 2j+1 of the tile; corrd[i] = ((double)x2, (double)y2) of correspondence i
// (converted once per match, not once per hypothesis).  grid = (ceil(hyp/256), batch).
__global__ __launch_bounds__(kScoreThreads) void ransac_score_kernel(
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, float threshold,
    const float *__restrict__ hypF, int32_t *__restrict__ hyp_count, float *__restrict__ hyp_sum) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int h = blockIdx.x * kScoreThreads + tid;
    const int m = m_arr[b];
    if (m < min_m) return;

    __shared__ __align__(16) float corr[kScoreTile * 4];
    __shared__ double2 corrd[kScoreTile];
    const float2 *P1 = reinterpret_cast<const float2 *>(xy1) + (size_t)b * kp_stride;
    const float2 *P2 = reinterpret_cast<const float2 *>(xy2) + (size_t)b * kp_stride;
    const int2 *PR = reinterpret_cast<const int2 *>(pairs) + (size_t)b * kp_stride;

    ResidualF R;
    const int hc = h < hyp ? h : hyp - 1;
    const float *src = hypF + ((size_t)b * hyp + hc) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) R.f[k] = src[k];
    residual_prepare(R);

    int count = 0;
    double total = 0;
    for (int base = 0; base < m; base += kScoreTile) {
        const int rows = min(kScoreTile, m - base);
        __syncthreads();
        for (int i = tid; i < ((rows + 1) & ~1); i += kScoreThreads) {
            const int2 pr = PR[base + min(i, rows - 1)];   // an odd tail is padded with its last correspondence
            const float2 a = P1[pr.x], c = P2[pr.y];
            float *d = corr + (i >> 1) * 8 + (i & 1);
            d[0] = a.x;
            d[2] = a.y;
            d[4] = c.x;
            d[6] = c.y;
            corrd[i] = make_double2((double)c.x, (double)c.y);
        }
        __syncthreads();
        const int full = rows >> 1;
#pragma unroll 2
        for (int j = 0; j < full; j++) {
            const float4 p = *reinterpret_cast<const float4 *>(corr + j * 8);
            const float4 r = *reinterpret_cast<const float4 *>(corr + j * 8 + 4);
            v2f x1, y1, x2, y2;
            x1.x = p.x; x1.y = p.y; y1.x = p.z; y1.y = p.w;
            x2.x = r.x; x2.y = r.y; y2.x = r.z; y2.y = r.w;
            const v2f e = residual_e2(R, x1, y1, x2, y2, corrd[2 * j], corrd[2 * j + 1]);
            count += (e.x <= threshold) ? 1 : 0;   // NaN <= thr is false, :130
            total += (double)e.x;                  // cv::sum in index order, :138
            count += (e.y <= threshold) ? 1 : 0;
            total += (double)e.y;
        }
        if (rows & 1) {
            const int i = rows - 1;
            const float *d = corr + (i >> 1) * 8;
            const double2 d2 = corrd[i];
            const float e = residual_e(R, make_float4(d[0], d[2], d[4], d[6]), d2.x, d2.y);
            count += (e <= threshold) ? 1 : 0;
            total += (double)e;
        }
    }
    if (h < hyp) {
        hyp_count[(size_t)b * hyp + h] = count;
        hyp_sum[(size_t)b * hyp + h] = (float)total;
    }
}

// C* = the pair's largest inlier count, and which of the hypotheses that reach it need their exact residual sum.
// The accept rule keeps, among the hypotheses with count C*, the one with the largest float sum (first index among equal
// sums; the NaN cases are spelled out at ransac_select_kernel).  The counting kernel left a cheap sum S~ and a bound err
// with |S~ - exact sum| <= err for every hypothesis, so a tied hypothesis whose S~ + err lies below the best S~ - err (by
// more than float rounding can close: factor 1 - 2^-20) cannot win and cannot tie after rounding: its hyp_sum becomes
// -inf (ordered below every real sum, never NaN).  The others — normally a handful — go on the list for
// ransac_tiesum_kernel.  Hypotheses with an uncertified cheap sum carry err = inf and always stay.
// tie_n[2b] = list length, tie_n[2b+1] = C*.  One workgroup per pair.
constexpr int kTieThreads = 256;
__device__ __forceinline__ void ransac_ties_body(const int b, const int32_t *__restrict__ m_arr, int min_m, int hyp,
                                                 int32_t *__restrict__ hyp_count,
                                                 const float *__restrict__ approx, float *__restrict__ hyp_sum,
                                                 int32_t *__restrict__ tie_idx, int32_t *__restrict__ tie_n) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_w[kTieThreads / 64];
    __shared__ float s_f[kTieThreads / 64];
    __shared__ int s_base;
    if (m_arr[b] < min_m) {
        if (tid == 0) {
            tie_n[2 * b] = 0;
            tie_n[2 * b + 1] = 0;
        }
        return;
    }
    int32_t *C = hyp_count + (size_t)b * hyp;
    const float2 *A = reinterpret_cast<const float2 *>(approx) + (size_t)b * hyp;
    float *Sm = hyp_sum + (size_t)b * hyp;
    int32_t *TI = tie_idx + (size_t)b * hyp;
    int mx = 0;
    for (int i = tid; i < hyp; i += kTieThreads) mx = max(mx, C[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_w[wave] = mx;
    if (tid == 0) s_base = 0;
    __syncthreads();
    mx = s_w[0];
    for (int w = 1; w < kTieThreads / 64; w++) mx = max(mx, s_w[w]);
    // best certified lower bound among the tied hypotheses
    float L = -INFINITY;
    for (int i = tid; i < hyp; i += kTieThreads)
        if (C[i] == mx) {
            const float2 a = A[i];
            const float lowb = a.x - a.y;
            if (lowb > L) L = lowb;   // false for NaN
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) L = fmaxf(L, __shfl_xor(L, off, 64));
    if (lane == 0) s_f[wave] = L;
    __syncthreads();
    L = s_f[0];
    for (int w = 1; w < kTieThreads / 64; w++) L = fmaxf(L, s_f[w]);
    const float cut = L > 0.f ? L * (1.f - 0x1p-20f) : -INFINITY;   // sums are >= 0: nothing is pruned against a bound <= 0
    __syncthreads();
    for (int i0 = 0; i0 < hyp; i0 += kTieThreads) {
        const int i = i0 + tid;
        bool keep = false;
        // which hypotheses below the maximum were counted in full depends on when the counting kernel learned its
        // bounds: the array is made canonical (and says so) — the maximum for those that reach it, -1 for the rest
        if (i < hyp && C[i] != mx) C[i] = -1;
        if (i < hyp && C[i] == mx) {
            const float2 a = A[i];
            keep = !(a.x + a.y < cut);   // NaN or inf bounds stay
            if (!keep) Sm[i] = -INFINITY;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; w++) off += s_w[w];
        if (keep) TI[off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int w = 0; w < kTieThreads / 64; w++) tot += s_w[w];
            s_base += tot;
        }
        __syncthreads();
    }
    if (tid == 0) {
        tie_n[2 * b] = s_base;
        tie_n[2 * b + 1] = mx;
    }
}
__global__ __launch_bounds__(kTieThreads) void ransac_ties_kernel(const int32_t *__restrict__ m_arr, int min_m, int hyp,
                                                                  int32_t *__restrict__ hyp_count,
                                                                  const float *__restrict__ approx, float *__restrict__ hyp_sum,
                                                                  int32_t *__restrict__ tie_idx, int32_t *__restrict__ tie_n) {
    ransac_ties_body(blockIdx.x, m_arr, min_m, hyp, hyp_count, approx, hyp_sum, tie_idx, tie_n);
}

// The exact residual sum (sequential double accumulation in match order, then one rounding to float: the value
// RansacFilter.cpp:138 returns) for the hypotheses in the tie list.  grid = (kTieGrid, batch), one wave each, looping over
// the list (normally one entry: a larger grid of workgroups that find nothing to do costs more than the work itself).
//   few ties : a wave per tied hypothesis; the lanes evaluate all matches (64 at a time), park every e in LDS, and the
//              sum then walks them in order (every lane computes the same total from broadcast reads);
//   many ties: a lane per tied hypothesis walking all matches (the shape of ransac_score_kernel), 64 per wave.
constexpr int kTieLaneMode = 192;
constexpr int kTieGrid = 4;
// WAVE_ONLY: the caller is one wave of a larger workgroup (ransac_finish_kernel): `slot` of `nslots` is that wave, and the
// LDS hand-overs below are inside the wave, where program order is enough (no workgroup barrier: the waves run different
// numbers of trips).
template <bool WAVE_ONLY>
__device__ __forceinline__ void ransac_tiesum_body(
    const int b, const int slot, const int nslots, const int lane, float *s_e, float4 *sc,
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, const float *__restrict__ hypF,
    const int32_t *__restrict__ tie_idx, const int32_t *__restrict__ tie_n, float *__restrict__ hyp_sum) {
    auto sync = [&]() {
        if (WAVE_ONLY) __builtin_amdgcn_wave_barrier();
        else __syncthreads();
    };
    const int m = min(m_arr[b], kp_stride);
    if (m < min_m) return;
    const int T = tie_n[2 * b];
    const int32_t *TI = tie_idx + (size_t)b * hyp;
    const float2 *P1 = reinterpret_cast<const float2 *>(xy1) + (size_t)b * kp_stride;
    const float2 *P2 = reinterpret_cast<const float2 *>(xy2) + (size_t)b * kp_stride;
    const int2 *PR = reinterpret_cast<const int2 *>(pairs) + (size_t)b * kp_stride;

    if (T >= kTieLaneMode) {
        for (int blk = slot; blk * 64 < T; blk += nslots) {
            const int k = blk * 64 + lane;
            const int h = TI[min(k, T - 1)];
            ResidualF R;
            const float *src = hypF + ((size_t)b * hyp + h) * 9;
#pragma unroll
            for (int j = 0; j < 9; j++) R.f[j] = src[j];
            residual_prepare(R);
            double total = 0;
            for (int i0 = 0; i0 < m; i0 += 64) {   // 64 matches staged by the wave, then walked in order as broadcasts
                const int2 pr = PR[min(i0 + lane, m - 1)];
                const float2 a = P1[pr.x], c = P2[pr.y];
                sync();
                sc[lane] = make_float4(a.x, a.y, c.x, c.y);
                sync();
                const int cnt = min(64, m - i0);
                for (int t = 0; t < cnt; t++) {
                    const float4 v = sc[t];
                    total += (double)residual_e(R, v, (double)v.z, (double)v.w);
                }
            }
            if (k < T) hyp_sum[(size_t)b * hyp + h] = (float)total;
        }
        return;
    }
    // s_e: kp_stride floats: every e of the hypothesis, then summed in order
    for (int k = slot; k < T; k += nslots) {
        const int h = TI[k];
        ResidualF R;
        const float *src = hypF + ((size_t)b * hyp + h) * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) R.f[j] = src[j];
        residual_prepare(R);
        sync();   // one wave: the previous hypothesis' reads are done
        // every e first, four matches per lane and round so that their gathers are in flight together ...
        for (int i0 = 0; i0 < m; i0 += 256) {
            int2 pr[4];
            float2 a[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) pr[u] = PR[min(i0 + u * 64 + lane, m - 1)];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                a[u] = P1[pr[u].x];
                c[u] = P2[pr[u].y];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u * 64 + lane;
                const float e = residual_e(R, make_float4(a[u].x, a[u].y, c[u].x, c[u].y), (double)c[u].x, (double)c[u].y);
                if (i < m) s_e[i] = e;
            }
        }
        sync();
        // ... then the sum, in match order (every lane walks the same broadcast reads and computes the same total);
        // sixteen values are fetched ahead of the dependent additions
        double total = 0;
        int t = 0;
        for (; t + 16 <= m; t += 16) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const float4 *>(s_e + t + 4 * u);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                total += (double)v[u].x;
                total += (double)v[u].y;
                total += (double)v[u].z;
                total += (double)v[u].w;
            }
        }
        for (; t < m; t++) total += (double)s_e[t];
        if (lane == 0) hyp_sum[(size_t)b * hyp + h] = (float)total;
    }
}

__global__ __launch_bounds__(64) void ransac_tiesum_kernel(
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, const float *__restrict__ hypF,
    const int32_t *__restrict__ tie_idx, const int32_t *__restrict__ tie_n, float *__restrict__ hyp_sum) {
    extern __shared__ __align__(16) float s_e_dyn[];
    __shared__ float4 sc[64];
    ransac_tiesum_body<false>(blockIdx.y, blockIdx.x, gridDim.x, threadIdx.x, s_e_dyn, sc, xy1, xy2, pairs, m_arr, min_m, kp_stride,
                              hyp, hypF, tie_idx, tie_n, hyp_sum);
}

// ------------------------------------------------------------------------------------------
// find_fundamental's accept rule + winner mask + inlier filter
// ------------------------------------------------------------------------------------------
constexpr int kSelThreads = 256;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
// monotone map float -> u32 (for non-NaN inputs), +0 and -0 collapse
__device__ __forceinline__ uint32_t float_order(float f) {
    if (f == 0.f) f = 0.f;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The reference scans hypotheses in order and accepts when count > best || (count == best &&
// sum > best_sum), starting from (0, 0.0f) (RansacFilter.cpp:44-45,59).  Closed form used here:
//   C* = max count, i0 = first index with count C*.
//   C* > 0 and sum[i0] is NaN      -> winner i0 (a NaN best_sum is never beaten at equal count)
//   otherwise                      -> first index among {count == C*, sum not NaN} with maximal sum
//                                     (for C* == 0 only if that sum > 0.0f, else nothing accepted)
__device__ __forceinline__ void ransac_select_body(
    const int b, const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, float threshold,
    const float *__restrict__ hypF, const int32_t *__restrict__ hyp_count,
    const float *__restrict__ hyp_sum, float *__restrict__ F_out, uint8_t *__restrict__ mask,
    int32_t *__restrict__ best, int32_t *__restrict__ matches) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int m = m_arr[b];
    __shared__ unsigned long long s_key[kSelThreads / 64];
    __shared__ int s_wave_cnt[kSelThreads / 64];
    __shared__ int s_base;
    uint8_t *MK = mask + (size_t)b * kp_stride;
    int32_t *BO = best + (size_t)b * 4;

    int winner = -1, win_count = 0;
    float win_sum = 0.f;
    if (m >= min_m) {
        const int32_t *C = hyp_count + (size_t)b * hyp;
        const float *Sm = hyp_sum + (size_t)b * hyp;
        unsigned long long k = 0;
        for (int i = tid; i < hyp; i += kSelThreads)   // -1 = "below the maximum" (the counting path's canonical form): never the key
            k = max(k, ((unsigned long long)(uint32_t)max(C[i], 0) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i));
        k = wave_max_u64(k);
        if (lane == 0) s_key[wave] = k;
        __syncthreads();
        k = s_key[0];
        for (int w = 1; w < kSelThreads / 64; w++) k = max(k, s_key[w]);
        __syncthreads();
        const int cstar = (int)(k >> 32);
        const int i0 = (int)(0xFFFFFFFFu - (uint32_t)k);
        const float s0 = Sm[i0];
        if (cstar > 0 && s0 != s0) {
            winner = i0;
            win_sum = s0;
        } else {
            unsigned long long k2 = 0;   // 0 == "no candidate" (float_order never returns 0 for finite/inf)
            for (int i = tid; i < hyp; i += kSelThreads) {
                const float s = Sm[i];
                if (C[i] == cstar && s == s)
                    k2 = max(k2, ((unsigned long long)float_order(s) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i));
            }
            k2 = wave_max_u64(k2);
            if (lane == 0) s_key[wave] = k2;
            __syncthreads();
            k2 = s_key[0];
            for (int w = 1; w < kSelThreads / 64; w++) k2 = max(k2, s_key[w]);
            __syncthreads();
            if (k2 != 0) {
                const int iw = (int)(0xFFFFFFFFu - (uint32_t)k2);
                const float sw = Sm[iw];
                if (cstar > 0 || sw > 0.0f) {
                    winner = iw;
                    win_sum = sw;
                }
            }
        }
        win_count = winner >= 0 ? cstar : 0;
    }

    if (tid == 0) s_base = 0;
    __syncthreads();

    ResidualF R;
    if (winner >= 0) {
        const float *src = hypF + ((size_t)b * hyp + winner) * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) R.f[k] = src[k];
        residual_prepare(R);
        if (tid < 9) F_out[(size_t)b * 9 + tid] = R.f[tid];   // temp_F.copyTo(fundamental), :63
    }
    const float2 *P1 = reinterpret_cast<const float2 *>(xy1) + (size_t)b * kp_stride;
    const float2 *P2 = reinterpret_cast<const float2 *>(xy2) + (size_t)b * kp_stride;
    const int2 *PR = reinterpret_cast<const int2 *>(pairs) + (size_t)b * kp_stride;
    int2 *MO = reinterpret_cast<int2 *>(matches) + (size_t)b * kp_stride;

    // winner's mask (inliers.swap, :64) and the ordered inlier filter of Frame.cpp:98-102
    for (int i0 = 0; i0 < m; i0 += kSelThreads) {
        const int i = i0 + tid;
        bool in = false;
        int2 pr = make_int2(0, 0);
        if (i < m) {
            pr = PR[i];
            if (winner >= 0) {
                const float2 a = P1[pr.x], c = P2[pr.y];
                in = residual_e(R, make_float4(a.x, a.y, c.x, c.y), (double)c.x, (double)c.y) <= threshold;
            }
            MK[i] = in ? 1 : 0;
        }
        const unsigned long long bal = __ballot(in);
        const int in_wave = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; w++) off += s_wave_cnt[w];
        if (in) MO[off + in_wave] = pr;
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int w = 0; w < kSelThreads / 64; w++) tot += s_wave_cnt[w];
            s_base += tot;
        }
        __syncthreads();
    }
    if (tid == 0) {
        BO[0] = winner;
        BO[1] = win_count;
        BO[2] = __float_as_int(win_sum);
        BO[3] = s_base;
    }
}
__global__ __launch_bounds__(kSelThreads) void ransac_select_kernel(
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, float threshold,
    const float *__restrict__ hypF, const int32_t *__restrict__ hyp_count,
    const float *__restrict__ hyp_sum, float *__restrict__ F_out, uint8_t *__restrict__ mask,
    int32_t *__restrict__ best, int32_t *__restrict__ matches) {
    ransac_select_body(blockIdx.x, xy1, xy2, pairs, m_arr, min_m, kp_stride, hyp, threshold, hypF, hyp_count, hyp_sum, F_out, mask,
                       best, matches);
}

// The three closing stages of the counting path in one launch, one workgroup per pair: which maximum-count hypotheses
// need their exact sum (ransac_ties_kernel), those sums (ransac_tiesum_kernel: the workgroup's four waves are its four
// slots), the accept rule and the winner's mask (ransac_select_kernel).  Each stage reads what the one before left in
// memory; they are separated by workgroup barriers, which order a workgroup's own global writes.  Saves two dependent
// launches per step (each mostly dispatch and drain at one workgroup per pair).
static_assert(kTieThreads == kSelThreads && kTieThreads == 64 * kTieGrid, "one shape for the fused closing kernel");
__global__ __launch_bounds__(kSelThreads) void ransac_finish_kernel(
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, float threshold,
    const float *__restrict__ hypF, int32_t *__restrict__ hyp_count, const float *__restrict__ approx,
    float *__restrict__ hyp_sum, int32_t *__restrict__ tie_idx, int32_t *__restrict__ tie_n, float *__restrict__ F_out,
    uint8_t *__restrict__ mask, int32_t *__restrict__ best, int32_t *__restrict__ matches) {
    extern __shared__ __align__(16) float s_e_all[];   // kTieGrid x kp_stride floats
    __shared__ float4 sc_all[kTieGrid][64];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ransac_ties_body(b, m_arr, min_m, hyp, hyp_count, approx, hyp_sum, tie_idx, tie_n);
    __syncthreads();
    ransac_tiesum_body<true>(b, wave, kTieGrid, lane, s_e_all + (size_t)wave * kp_stride, sc_all[wave], xy1, xy2, pairs, m_arr, min_m,
                             kp_stride, hyp, hypF, tie_idx, tie_n, hyp_sum);
    __syncthreads();
    ransac_select_body(b, xy1, xy2, pairs, m_arr, min_m, kp_stride, hyp, threshold, hypF, hyp_count, hyp_sum, F_out, mask, best,
                       matches);
}

}  // namespace

int vs_launch_ransac_evaluate(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs,
                              const int32_t *m, const float *hypF, int batch, int kp_stride, int hyp,
                              float threshold, float *F, uint8_t *mask, int32_t *best, int32_t *matches,
                              int32_t *hyp_count, float *hyp_sum) {
    VS_REQUIRE(ctx, xy1 && xy2 && pairs && m && hypF && F && mask && best && matches, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, hyp_count && hyp_sum, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && kp_stride > 0 && hyp > 0, VSLAM_ERR_INVALID);
    const int min_m = ctx->ransac_min_matches;   // items with fewer matches get no model (8 unless the caller brought its own F)
    if (ctx->ransac_all_sums) {
        VsProfScope ps(ctx, "ransac_score_kernel");
        dim3 grid(vs_div_up(hyp, kScoreThreads), batch);
        ransac_score_kernel<<<grid, kScoreThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, min_m, kp_stride, hyp,
                                                                     threshold, hypF, hyp_count, hyp_sum);
    } else {
        VS_REQUIRE(ctx, kp_stride <= VSLAM_MAX_KP, VSLAM_ERR_CAPACITY);
        int32_t *tie_idx = nullptr, *tie_n = nullptr;
        float *approx = nullptr;
        int rc;
        if ((rc = vs_arena_get(ctx, "ransac.approx", sizeof(float) * 2 * (size_t)batch * hyp, (void **)&approx))) return rc;
        if ((rc = vs_arena_get(ctx, "ransac.tie_idx", sizeof(int32_t) * (size_t)batch * hyp, (void **)&tie_idx))) return rc;
        if ((rc = vs_arena_get(ctx, "ransac.tie_n", sizeof(int32_t) * 2 * (size_t)batch, (void **)&tie_n))) return rc;
        if ((rc = vs_launch_ransac_count(ctx, xy1, xy2, pairs, m, hypF, batch, kp_stride, hyp, threshold, hyp_count, hyp_sum, approx)))
            return rc;
        // the closing stages: one launch when the four waves' sum buffers fit LDS (kp_stride <= 4096), else three
        const size_t fin_lds = sizeof(float) * (size_t)kTieGrid * kp_stride;
        static const bool split_finish = VS_EXPERIMENT_ENV("VSLAM_RANSAC_SPLIT_FINISH") != nullptr;   // A/B timing
        if (fin_lds <= 64 * 1024 && !split_finish) {
            VsProfScope ps(ctx, "ransac_finish_kernel");
            if (fin_lds > 32 * 1024 && (rc = vs_allow_dynamic_lds(ctx, ransac_finish_kernel, "ransac_finish", 64 * 1024))) return rc;
            ransac_finish_kernel<<<batch, kSelThreads, fin_lds, ctx->stream>>>(xy1, xy2, pairs, m, min_m, kp_stride, hyp, threshold, hypF,
                                                                              hyp_count, approx, hyp_sum, tie_idx, tie_n, F, mask, best,
                                                                              matches);
            VS_HIP(ctx, hipGetLastError());
            return VSLAM_OK;
        }
        {
            VsProfScope ps(ctx, "ransac_ties_kernel");
            ransac_ties_kernel<<<batch, kTieThreads, 0, ctx->stream>>>(m, min_m, hyp, hyp_count, approx, hyp_sum, tie_idx, tie_n);
        }
        {
            VsProfScope ps(ctx, "ransac_tiesum_kernel");
            dim3 grid(min(kTieGrid, vs_div_up(hyp, 64)), batch);
            if (sizeof(float) * (size_t)kp_stride > 40 * 1024 &&
                (rc = vs_allow_dynamic_lds(ctx, ransac_tiesum_kernel, "ransac_tiesum", sizeof(float) * VSLAM_MAX_KP)))
                return rc;
            ransac_tiesum_kernel<<<grid, 64, sizeof(float) * (size_t)kp_stride, ctx->stream>>>(xy1, xy2, pairs, m, min_m, kp_stride, hyp, hypF, tie_idx, tie_n,
                                                              hyp_sum);
        }
    }
    {
        VsProfScope ps(ctx, "ransac_select_kernel");
        ransac_select_kernel<<<batch, kSelThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, min_m, kp_stride, hyp,
                                                                     threshold, hypF, hyp_count, hyp_sum,
                                                                     F, mask, best, matches);
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

int vs_launch_ransac(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs,
                     const int32_t *m, const int32_t *sets, int batch, int kp_stride, int hyp,
                     float threshold, float *F, uint8_t *mask, int32_t *best, int32_t *matches,
                     float *hypF, int32_t *hyp_count, float *hyp_sum) {
    int rc = vs_launch_ransac_solve(ctx, xy1, xy2, pairs, m, sets, batch, kp_stride, hyp, hypF);
    if (rc) return rc;
    if ((rc = vs_aux_job_point(ctx, 3))) return rc;
    return vs_launch_ransac_evaluate(ctx, xy1, xy2, pairs, m, hypF, batch, kp_stride, hyp, threshold, F, mask,
                                     best, matches, hyp_count, hyp_sum);
}
