// RANSAC fundamental-matrix loop, stage 3 of 4: inlier counts, counts first (the default scoring path).
//
// Replaces the counting half of RansacFilter::compute_fundamental_residual (the reference's src/RansacFilter.cpp:105-140:
// the inlier test :130 for every hypothesis; the sums :138 are left to ransac_select.hip, for the few hypotheses that need
// one) -> ransac_rank_kernel, ransac_screen_kernel, ransac_cand_kernel, ransac_count_kernel<>.
//
// Numerics: the counts handed on are the reference's counts, bit for bit, for every hypothesis that reaches the pair's
// maximum count (all others report -1).  The cheap evaluation only decides what its certified error band allows; anything
// inside the band is decided by the exact sequence (residual_e, ransac_residual.h).  The derivation stands in front of the code.
#include "ransac_prune_tile.h"
#include "ransac_residual.h"

namespace {
using namespace vs_ransac;

// find_fundamental consults a hypothesis' residual SUM only to break ties among hypotheses whose inlier COUNT
// equals the running maximum (RansacFilter.cpp:59); every other sum is computed by the reference and thrown away,
// and a COUNT below the pair's maximum never reaches the accept rule either.  So the scoring is split:
//   ransac_rank_kernel    exact counts of 8 pilot hypotheses (a first lower bound on the maximum) and, from their
//                         inlier masks, the matches ordered by how many pilots miss them (most-missed first), laid
//                         out as four coordinate arrays;
//   ransac_screen_kernel  every hypothesis on the 128 most-missed matches (the head): how many of those it can have as
//                         inliers, how many it certainly has, and the sum of its cheap values there;
//   ransac_cand_kernel    exact full counts of the (up to 8) hypotheses that do best there -> the bound is now the
//                         pair's maximum count on almost every pair;
//   ransac_count_kernel   exact inlier count of every hypothesis that can reach the maximum (those that do are always
//                         counted in full), from a cheap evaluation of e with a certified error band; the few
//                         evaluations that land inside the band are re-done with the exact sequence (residual_e)
//                         -> these counts are the reference's counts, bit for bit;
//   ransac_ties_kernel    C* = max count per pair; of the hypotheses that reach it, those whose sum can still be
//                         the largest after rounding (the count kernel's cheap sums bound every exact sum);
//   ransac_tiesum_kernel  the exact, index-ordered double sum (cv::sum, :138) for those hypotheses only;
//   ransac_select_kernel  unchanged: it only ever reads the sums of hypotheses whose count is C*
//                         (pruned ones hold -inf).
// ransac_score_kernel in ransac_select.hip (all counts and all sums, exact) stays behind VSLAM_OPT_RANSAC_ALL_SUMS for callers that
// want every per-hypothesis sum (the per-hypothesis parity tests, RansacFilter::compute_fundamental_residual).
//
// The cheap evaluation.  With u = 2^-24 and everything finite, the reference computes (floats, round to nearest)
//   a_k = (f_3k x1 + f_3k+1 y1) + f_3k+2,  n = (x2 a0 + y2 a1) + a2,  nn = n n,  dd = a0 a0,  q = nn / dd,
//   t_0 = float(double(f0 x2 + f3 y2) + f6),  t_1 likewise,  e = ((q + a1 a1) + t0 t0) + t1 t1.
// The count kernel computes a_k, n, nn, dd with the SAME operations (they are cheap and any other order would need
// a cancellation-dependent bound), and replaces the rest by
//   q~ = nn * v_rcp_f32(dd)                        relative error <= 3.1 u  (rcp: 1 ulp)
//   t~_k = fma(f_3+k, y2, fma(f_k, x2, f_6+k))     |t~_k - t_k| <= 3.1 u S_k,  S_k = |f_k x2| + |f_3+k y2| + |f_6+k|
//   g = fma(t~1, t~1, fma(t~0, t~0, fma(a1, a1, q~)))
// All terms of e are squares, so every rounding is a relative error on a non-negative sum; with
// beta = 4.04 u (S_0 + S_1) (S bounded per hypothesis with the pair's largest |x2|, |y2|) and s = sqrt(thr):
//   g < lo = (s (1 - 2^-20) - 1.01 beta)^2                  =>  e <  thr   (e <= (sqrt(g) + 1.005 beta)^2 (1 + 12 u))
//   g > hi = (s (1 + 2^-20) + 2.5 beta)^2 (1 + 2^-20)       =>  e >  thr   (e >= ((sqrt(g)(1 - 1.7u) - beta)^2 - 2 beta^2)(1 - 9u))
// Anything else — g inside [lo, hi], NaN, a denormal / zero dd (where v_rcp_f32 is not a 1-ulp reciprocal), or a
// hypothesis / pair outside the range the bounds were derived for (|f| <= 2^10, coordinates <= 2^20, thr in
// [2^-20, 2^20], so nothing overflows before the true value does) — is decided by the exact sequence.  On image
// data the band is about 0.3 % of thr wide (beta is a few 1e-3: f32 cancellation in t~), i.e. about one evaluation
// in a thousand, so uncertain evaluations are not handled in place (a wave would leave the fast path for 6 % of its
// evaluations) but queued per wave in LDS as (hypothesis, match) words and evaluated 64 at a time with full lanes.
//
// Bail-out: a hypothesis matters to the accept rule only if its count is the pair's maximum, so work on a hypothesis
// stops once the matches looked at contain more certain outliers than ANY maximum-count hypothesis can have:
// potential inliers seen + all matches not seen < a count some hypothesis of the pair verifiably reaches (`bound`,
// never above the true maximum).  Such hypotheses report -1 (ransac_ties_kernel then writes -1 for every hypothesis
// below the maximum, so the array does not depend on timing).  How soon that happens depends on two things the three
// small kernels in front are there for.  (1) The bound: on clean data a third to two thirds of the hypotheses share one
// count (every true correspondence an inlier) and a handful reach one more; with a bound one short of the maximum that
// whole plateau has to be counted in full, with the maximum itself none of it (tools/bail_sim.py: 54 % -> 29 % of all
// evaluations).  (2) The order: the matches every decent hypothesis misses are looked at first, so the allowance of
// outliers is used up at once and the first real difference decides.  Counts do not depend on the order of the
// matches, the cheap sums only within their certified bound, and ransac_tiesum_kernel sums in list order.
// The test comes after every 256-match sub-block (a check every 128 cost more than it saved: the kernel is bound by what a
// sub-block costs, not by evaluations), and the walk begins BEHIND the head: the screen has evaluated the head for every
// hypothesis already, so a survivor starts with seen = n0 = min(m, 128) and pot = pot0, and its first sub-block is ranked
// matches [n0, n0 + 256).  With D = m - bound + 1 certain outliers needed, the first exit comes at 384 matches seen instead
// of 512 whenever D mod 256 lies in (0, 128] -- one sub-block less for most hypotheses of a pair with 40-45 % outliers.
//
// Full counts stay the reference's.  The screen hands on, beside pot0, the head's certain inliers (g < lo) and the sum of
// the head's cheap values, or "not certified" after a zero / denormal / NaN dd.  A survivor with pot0 == certain (every
// head evaluation decided outside the band, with a certified band: !B.ok gives lo = -1, certain = 0) takes that count; any
// other survivor that completes its walk evaluates the head block itself as one more sub-block -- band, queue and exact
// sequence as everywhere -- and uses its own sum of the head's cheap values instead of the screen's.
//
// The cheap sum S~ and its error.  Per evaluation |g - e| <= 12 u max(g, e) + beta (2 sqrt(g) + beta); summed with
// Cauchy-Schwarz: |sum g - sum e| <= 2.02 beta sqrt(M S) + M beta^2 + 12 u (1 + ..) S over M evaluations.  S~ is formed in
// float from non-negative terms, so every addition on the way costs a relative u: S~ = (sum g)(1 + d), |d| <= A u for A
// additions on the longest path.  The tree is now: per lane two accumulators, two additions each per sub-block (the head block
// included where it is evaluated here); one addition across the two; six across the lanes (wave_sum_to_lane63); one that adds
// the screen's head sum, itself seven additions deep (ransac_screen_kernel) -- A <= 2 nsub + 9, one or two more than the walk
// from zero had for the same m (2 nsub' + 7 with nsub' = ceil(m / 256) >= nsub).  The relative term 2^-18 = 64 u of the error
// bound covers 12 u (1 + ..) + A u up to A = 51, i.e. 21 sub-blocks; for longer walks (more than about 5500 matches) the term
// is (13 + A) u instead (cnt_sum_rel): stated here because the constant alone did not cover them before either.  The sum
// rule uses the same expression over the `seen` evaluations so far, with the screen's head sum as their first part, and
// does not fire for a hypothesis whose head is not certified.
//
// Mapping of the count kernel: a workgroup = 128 hypotheses of a pair; those the screen has not already ruled out are
// handed to its 8 waves one at a time; a wave walks the ranked matches behind the head 256 at a time (4 per lane,
// coordinates staged in LDS as four arrays so that a lane's two neighbouring matches are the halves of a packed operand; the
// arrays are padded so that whole sub-blocks exist from ranked match 0 and from ranked match 128: cnt_pad); the hypothesis'
// record (F twice, lo, hi) is a broadcast read from LDS, and so is what the screen found for it; v_cmp writes lane masks
// to SGPRs, counting is s_bcnt1 on the scalar unit (north_star: ballot / popcount).
constexpr int kCntHyps = 128;
constexpr int kCntWaves = 8;
constexpr int kCntQueue = 320;          // words per wave: the 256 evaluations of one sub-block + 63 carried over
constexpr int kCntLdsMatches = 4096;    // ranked coordinates are staged in LDS up to this many matches (64 KiB); read from memory beyond
constexpr int kScreenMatches = 128;
constexpr int kScreenHyps = 128;        // per workgroup: 4 waves x 32
constexpr int kRankThreads = 512;
constexpr int kPilotHyps = kRankThreads / 64;
constexpr int kCandMax = 8;
constexpr float kCntTinyDD = 0x1p-120f;
// __builtin_amdgcn_fcmpf takes LLVM's FCmpInst::Predicate numbering: 2 = ogt, 4 = olt, 9 = ueq, 12 = ult.  The
// tiny-denominator guards below need ult (true for dd < 2^-120 and for NaN).  Builds from c89bef8 (round 2,
// "counts first") up to cce43df (round 3, where the fix rode along in the bench-parity commit) passed 9 there, so the guard fired only on NaN or dd == 2^-120 exactly, and zero / denormal
// a0^2 were certified through v_rcp_f32 instead of taking the exact path (test_tiny_denominators_take_the_exact_path).
constexpr int kFcmpOGT = 2, kFcmpOLT = 4, kFcmpULT = 12;
// A hypothesis as the counting loop reads it from LDS: F, lo, hi (+ 1 pad): kCntRec floats per hypothesis.  (Storing every
// element of F twice spares the loop nine v_movs per hypothesis — the (f, f) operands of the packed instructions — but
// costs 4 KiB per workgroup, which is the difference between two and three workgroups per CU.)
constexpr int kCntRec = 12;
// a wave's queue: volatile (lanes read what other lanes wrote) and typed as LDS so that the accesses are ds_ instructions
typedef __attribute__((address_space(3))) volatile uint32_t cnt_queue_t;
static_assert(VSLAM_MAX_KP <= 65536, "queue words keep the match index in 16 bits");

// Slots per ranked coordinate array for n matches: whole 256-match sub-blocks from ranked match 0.  The count kernel's walk
// starts at ranked match kScreenMatches, so its last sub-block can reach up to 128 slots further: those lanes read the array's
// last four slots instead (a real match or its copy, masked like every lane beyond m) -- 128 more slots per array would be
// 2 KiB of LDS per workgroup, and at 2000 keypoints that is the difference between two and three workgroups per CU.
__host__ __device__ constexpr int cnt_pad(int n) { return (n + 255) & ~255; }
// The word the screen hands on per hypothesis beside pot0: the head's certain inliers (g < lo), kHeadUncertified where
// nothing of the head is certified, and the sum of the head's cheap values.
constexpr int kHeadUncertified = kVsHeadUncertified;
// relative error of a cheap sum against the sum of its terms: 12 u per term (g against e, see ransac_ties_kernel) and u per
// float addition on the longest path to the total (`adds`).  2^-18 = 64 u covers 51 additions, i.e. 21 sub-blocks (about
// 5500 matches); beyond that the term grows with the walk instead of being assumed.
__device__ __forceinline__ float cnt_sum_rel(int adds) { return fmaxf(0x1p-18f, (float)(13 + adds) * 0x1p-24f); }

struct CntBand {
    float lo, hi;
    double beta;
    bool ok;
};
// the certified band of one hypothesis (see above); C1 / C2 = the pair's largest |coordinate| in frame 1 / 2
__device__ __forceinline__ CntBand cnt_band(const float *f, float C1, float C2, float threshold) {
    CntBand B;
    bool ok = threshold >= 0x1p-20f && threshold <= 0x1p20f && C1 <= 0x1p20f && C2 <= 0x1p20f;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && fabsf(f[k]) <= 1024.f;   // false for NaN
    const double S = ((double)fabsf(f[0]) + (double)fabsf(f[3]) + (double)fabsf(f[1]) + (double)fabsf(f[4])) * (double)C2 +
                     (double)fabsf(f[6]) + (double)fabsf(f[7]);
    const double beta = 4.04 * 0x1p-24 * S + 1e-30;
    const double sq = sqrt((double)threshold);
    const double lo_r = sq * (1.0 - 0x1p-20) - 1.01 * beta;
    const double hi_r = sq * (1.0 + 0x1p-20) + 2.5 * beta;
    B.lo = lo_r > 0 ? (float)(lo_r * lo_r * (1.0 - 0x1p-22)) : -1.f;
    B.hi = (float)(hi_r * hi_r * (1.0 + 0x1p-20) * (1.0 + 0x1p-22));
    if (!ok) {
        B.lo = -1.f;       // g >= 0 or NaN: never below lo
        B.hi = INFINITY;   // never above hi: every evaluation takes the exact sequence
    }
    B.beta = beta;
    B.ok = ok;
    return B;
}
__device__ __forceinline__ void cnt_store_record(float *d, const float *f, const CntBand &B) {
#pragma unroll
    for (int k = 0; k < 9; k++) d[k] = f[k];
    d[9] = B.lo;
    d[10] = B.hi;
    d[11] = B.ok ? (float)(B.beta * (1.0 + 0x1p-20)) : -1.f;   // beta rounded up (the sum rule's error term); < 0: nothing is certified
}

struct CntRec {
    float f[9];   // the packed instructions take (f, f) operands: a splat of one register is an operand modifier (op_sel_hi)
    float lo, hi;
    float beta;   // >= the band's beta; < 0 when the cheap values of this hypothesis are not certified
};
__device__ __forceinline__ void cnt_load_record(CntRec &R, const float *s_rec, int hh) {
    const float4 *r4 = reinterpret_cast<const float4 *>(s_rec + hh * kCntRec);
    const float4 v0 = r4[0], v1 = r4[1], v2 = r4[2];
    const float f[9] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x};
#pragma unroll
    for (int k = 0; k < 9; k++) R.f[k] = f[k];
    R.lo = v2.y;
    R.hi = v2.z;
    R.beta = v2.w;
}

// the cheap value g for two matches per lane; dd returned for the caller's denormal check
__device__ __forceinline__ v2f cnt_splat(float f) {
    v2f r;
    r.x = f;
    r.y = f;
    return r;
}
__device__ __forceinline__ v2f cnt_cheap(const CntRec &R, const v2f X1, const v2f Y1, const v2f X2, const v2f Y2, v2f &dd) {
    const v2f f0 = cnt_splat(R.f[0]), f1 = cnt_splat(R.f[1]), f2 = cnt_splat(R.f[2]), f3 = cnt_splat(R.f[3]), f4 = cnt_splat(R.f[4]),
              f5 = cnt_splat(R.f[5]), f6 = cnt_splat(R.f[6]), f7 = cnt_splat(R.f[7]), f8 = cnt_splat(R.f[8]);
    const v2f a0 = (f0 * X1 + f1 * Y1) + f2;
    const v2f a1 = (f3 * X1 + f4 * Y1) + f5;
    const v2f a2 = (f6 * X1 + f7 * Y1) + f8;
    const v2f n = (X2 * a0 + Y2 * a1) + a2;
    const v2f nn = n * n;
    dd = a0 * a0;
    v2f r;
    r.x = __builtin_amdgcn_rcpf(dd.x);
    r.y = __builtin_amdgcn_rcpf(dd.y);
    v2f g = __builtin_elementwise_fma(a1, a1, nn * r);
    const v2f t0 = __builtin_elementwise_fma(f3, Y2, __builtin_elementwise_fma(f0, X2, f6));
    const v2f t1 = __builtin_elementwise_fma(f4, Y2, __builtin_elementwise_fma(f1, X2, f7));
    g = __builtin_elementwise_fma(t0, t0, g);
    g = __builtin_elementwise_fma(t1, t1, g);
    return g;
}

// exact evaluation of up to 64 queued (hypothesis, ranked match) words, one per lane
__device__ __forceinline__ void cnt_drain(const cnt_queue_t *q, int from, int count, int lane, const float *s_rec,
                                          int *s_cnt, const float *cx1, const float *cy1, const float *cx2, const float *cy2,
                                          float threshold) {
    if (lane < count) {
        const uint32_t en = q[from + lane];
        const int hh = (int)(en >> 16), i = (int)(en & 0xFFFFu);
        ResidualF R;
#pragma unroll
        for (int k = 0; k < 9; k++) R.f[k] = s_rec[hh * kCntRec + k];
        residual_prepare(R);
        const float x2 = cx2[i], y2 = cy2[i];
        const float e = residual_e(R, make_float4(cx1[i], cy1[i], x2, y2), (double)x2, (double)y2);
        if (e <= threshold) atomicAdd(&s_cnt[hh], 1);
    }
}

// append the lanes of mask U (evaluation `idx` of hypothesis hh, idx per lane) to the wave's queue
__device__ __forceinline__ void cnt_push(cnt_queue_t *q, int &qn, unsigned long long U, int hh, int idx, int lane) {
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(U >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)U, 0u));
    if ((U >> lane) & 1ull) q[qn + rank] = ((uint32_t)hh << 16) | (uint32_t)idx;
    qn += __popcll(U);
}

// two matches per lane (ranked positions ix, ix + 1) under one hypothesis: count of the certain inliers and masks of
// the undecided lanes
template <bool PARTIAL>
__device__ __forceinline__ void cnt_eval_pair(const CntRec &R, const v2f X1, const v2f Y1, const v2f X2, const v2f Y2, int ix,
                                              int m, int &cnt, unsigned long long &ua, unsigned long long &ub,
                                              float &ddmin, v2f &acc) {
    v2f dd;
    v2f g = cnt_cheap(R, X1, Y1, X2, Y2, dd);
    ddmin = fminf(ddmin, fminf(dd.x, dd.y));
    // v_cmp straight into a lane mask (llvm::CmpInst predicates: 4 = ordered <, 2 = ordered >)
    unsigned long long ia = __builtin_amdgcn_fcmpf(g.x, R.lo, kFcmpOLT), oa = __builtin_amdgcn_fcmpf(g.x, R.hi, kFcmpOGT);
    unsigned long long ib = __builtin_amdgcn_fcmpf(g.y, R.lo, kFcmpOLT), ob = __builtin_amdgcn_fcmpf(g.y, R.hi, kFcmpOGT);
    if (PARTIAL) {
        const bool in_a = ix < m, in_b = ix + 1 < m;
        const unsigned long long va = __ballot(in_a), vb = __ballot(in_b);
        ia &= va;
        ib &= vb;
        ua = va & ~(ia | oa);
        ub = vb & ~(ib | ob);
        g.x = in_a ? g.x : 0.f;
        g.y = in_b ? g.y : 0.f;
    } else {
        ua = ~(ia | oa);
        ub = ~(ib | ob);
    }
    cnt += __popcll(ia) + __popcll(ib);
    acc += g;   // running sum of the cheap values: ransac_ties_kernel prunes the tie list with it
}

// sum over the 64 lanes, in a fixed order, left in lane 63 (row butterflies, then row_bcast 15 / 31)
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
    const int z = 0;
    v += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(v), 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(v), 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(v), 0x141, 0xF, 0xF, false));   // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(v), 0x140, 0xF, 0xF, false));   // row_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(v), 0x142, 0xA, 0xF, false));   // row_bcast:15 -> rows 1, 3
    v += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(v), 0x143, 0xC, 0xF, false));   // row_bcast:31 -> rows 2, 3
    return v;
}

// one 256-match sub-block (the lane's ranked matches ix .. ix + 3) of hypothesis hh: certified count into cnt, the rest queued
template <bool PARTIAL>
__device__ __forceinline__ void cnt_sub_block(const CntRec &R, const float4 X1, const float4 Y1, const float4 X2, const float4 Y2,
                                              int ix, int hh, int lane, int m, int &cnt, cnt_queue_t *q, int &qn, v2f &acc,
                                              int *s_unk, int &pot, bool &unk) {
    unsigned long long u0, u1, u2, u3;
    int c = 0;
    float ddmin = INFINITY;
    v2f x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b;
    x1a.x = X1.x; x1a.y = X1.y; x1b.x = X1.z; x1b.y = X1.w;
    y1a.x = Y1.x; y1a.y = Y1.y; y1b.x = Y1.z; y1b.y = Y1.w;
    x2a.x = X2.x; x2a.y = X2.y; x2b.x = X2.z; x2b.y = X2.w;
    y2a.x = Y2.x; y2a.y = Y2.y; y2b.x = Y2.z; y2b.y = Y2.w;
    cnt_eval_pair<PARTIAL>(R, x1a, y1a, x2a, y2a, ix, m, c, u0, u1, ddmin, acc);
    cnt_eval_pair<PARTIAL>(R, x1b, y1b, x2b, y2b, ix + 2, m, c, u2, u3, ddmin, acc);
    if (__builtin_amdgcn_fcmpf(ddmin, kCntTinyDD, kFcmpULT) != 0ull) {   // unordered or <: some dd is zero / denormal (or NaN)
        // nothing of this sub-block is certified: all of it is queued, and the hypothesis' cheap sum means nothing
        if (lane == 0) s_unk[hh] = 1;
        unk = true;   // wave-uniform
        c = 0;
        u0 = __builtin_amdgcn_sicmp(ix, m, 40);   // 40 = signed <
        u1 = __builtin_amdgcn_sicmp(ix + 1, m, 40);
        u2 = __builtin_amdgcn_sicmp(ix + 2, m, 40);
        u3 = __builtin_amdgcn_sicmp(ix + 3, m, 40);
    }
    cnt += c;
    pot += c;   // inliers this sub-block can still turn out to have: the certain ones plus the undecided ones
    if ((u0 | u1 | u2 | u3) != 0ull) {
        pot += __popcll(u0) + __popcll(u1) + __popcll(u2) + __popcll(u3);
        if (u0) cnt_push(q, qn, u0, hh, ix, lane);
        if (u1) cnt_push(q, qn, u1, hh, ix + 1, lane);
        if (u2) cnt_push(q, qn, u2, hh, ix + 2, lane);
        if (u3) cnt_push(q, qn, u3, hh, ix + 3, lane);
    }
}

// exact inlier count of one hypothesis over the ranked coordinate arrays (one wave, lanes over the matches)
// (sum_out: the sum of every e as well, lanes' partial sums in double -- not the reference's sequential order: a value within
// m 2^-53 of it, for a bound)
__device__ __forceinline__ int cnt_exact_ranked(const float *F9, const float *r, int kp_pad, int m, float threshold, int lane,
                                                double *sum_out = nullptr) {
    ResidualF R;
#pragma unroll
    for (int j = 0; j < 9; j++) R.f[j] = F9[j];
    residual_prepare(R);
    int count = 0;
    double esum = 0;
    for (int i0 = 0; i0 < m; i0 += 256) {   // the arrays are padded to a multiple of 256
        float4 c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * 64 + lane;
            c[u] = make_float4(r[i], r[kp_pad + i], r[2 * kp_pad + i], r[3 * kp_pad + i]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const float e = residual_e(R, c[u], (double)c[u].z, (double)c[u].w);
            count += __popcll(__ballot(i0 + u * 64 + lane < m && e <= threshold));
            if (sum_out && i0 + u * 64 + lane < m) esum += (double)e;
        }
    }
    if (sum_out) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off, 64);
        *sum_out = esum;
    }
    return count;
}

// One workgroup per pair.  Wave w counts pilot hypothesis w exactly (lanes over the matches) and leaves its inlier mask in
// LDS; cbound[pair] = the best of those counts (stored, not accumulated: nothing has to clear it): a first lower bound on the pair's maximum count (any count of any
// hypothesis is a valid bound; a better one only prunes more).  Then the matches are ordered by the number of pilots that
// miss them, most-missed first, original order among equals (a counting sort over 9 keys), and written as four arrays
// rk[pair][0..3][kp_pad] = x1, y1, x2, y2, padded with a real match up to the next multiple of 256.
// cmax[pair] = the largest |coordinate| per frame (the error bands need it).
__global__ __launch_bounds__(kRankThreads) void ransac_rank_kernel(
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int kp_pad, int hyp, float threshold,
    const float *__restrict__ hypF, int32_t *__restrict__ cbound, float *__restrict__ rk, float *__restrict__ cmax,
    unsigned long long *__restrict__ sfloor) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = min(m_arr[b], kp_stride);
    if (m < min_m) return;
    __shared__ double s_psum[kPilotHyps];   // the pilots' residual sums (lanes' partial sums: for the sum floor, a bound)
    __shared__ unsigned long long s_bits[kPilotHyps][VSLAM_MAX_KP / 64];
    __shared__ int s_hist[kPilotHyps][kPilotHyps + 1], s_off[kPilotHyps][kPilotHyps + 1], s_pcount[kPilotHyps];
    const float2 *P1 = reinterpret_cast<const float2 *>(xy1) + (size_t)b * kp_stride;
    const float2 *P2 = reinterpret_cast<const float2 *>(xy2) + (size_t)b * kp_stride;
    const int2 *PR = reinterpret_cast<const int2 *>(pairs) + (size_t)b * kp_stride;
    const int npil = min(kPilotHyps, hyp);
    const int G = (m + 63) >> 6;

    if (wave < npil) {
        const int h = (int)(((long long)hyp * wave) / npil);
        ResidualF R;
        const float *src = hypF + ((size_t)b * hyp + h) * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) R.f[j] = src[j];
        residual_prepare(R);
        int count = 0;
        double esum = 0;
        float c1 = 0.f, c2 = 0.f;
        for (int g0 = 0; g0 < G; g0 += 4) {   // four matches per lane and round: their gathers are in flight together
            int2 pr[4];
            float2 a[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) pr[u] = PR[min((g0 + u) * 64 + lane, m - 1)];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                a[u] = P1[pr[u].x];
                c[u] = P2[pr[u].y];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float e = residual_e(R, make_float4(a[u].x, a[u].y, c[u].x, c[u].y), (double)c[u].x, (double)c[u].y);
                const unsigned long long in = __ballot((g0 + u) * 64 + lane < m && e <= threshold);
                count += __popcll(in);
                if ((g0 + u) * 64 + lane < m) esum += (double)e;
                if (lane == 0 && g0 + u < G) s_bits[wave][g0 + u] = in;
                c1 = fmaxf(c1, fmaxf(fabsf(a[u].x), fabsf(a[u].y)));
                c2 = fmaxf(c2, fmaxf(fabsf(c[u].x), fabsf(c[u].y)));
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off, 64);
        if (lane == 0) {
            s_pcount[wave] = count;
            s_psum[wave] = esum;
        }
        if (wave == 0) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                c1 = fmaxf(c1, __shfl_xor(c1, off, 64));
                c2 = fmaxf(c2, __shfl_xor(c2, off, 64));
            }
            if (lane == 0) {
                cmax[2 * b] = c1;
                cmax[2 * b + 1] = c2;
            }
        }
    }
    __syncthreads();

    // this wave's share of the 64-match groups; key of a match = number of pilots that miss it
    const int gpw = (G + kPilotHyps - 1) / kPilotHyps;
    const int g_lo = min(G, wave * gpw), g_hi = min(G, g_lo + gpw);
    int hist[kPilotHyps + 1];
#pragma unroll
    for (int v = 0; v <= kPilotHyps; v++) hist[v] = 0;
    for (int g = g_lo; g < g_hi; g++) {
        const bool valid = g * 64 + lane < m;
        int key = 0;
        for (int w = 0; w < npil; w++) key += (int)((~s_bits[w][g] >> lane) & 1ull);
#pragma unroll
        for (int v = 0; v <= kPilotHyps; v++) hist[v] += __popcll(__ballot(valid && key == v));
    }
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v <= kPilotHyps; v++) s_hist[wave][v] = hist[v];
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;   // the first word written to cbound[pair] in a call: a plain store, nothing to clear beforehand
        for (int w = 0; w < npil; w++) best = max(best, s_pcount[w]);
        cbound[b] = best;
        if (sfloor) {   // the first sum floor of the pair (see ransac_cand_kernel): the best-counting pilots' largest sum
            double fl = -INFINITY;
            bool any_nan = false;
            for (int w = 0; w < npil; w++)
                if (s_pcount[w] == best) {
                    any_nan = any_nan || !(s_psum[w] == s_psum[w]);
                    if (s_psum[w] > fl) fl = s_psum[w];
                }
            const bool valid = best > 0 && !any_nan && fl > 0 && fl < 0x1p120;
            sfloor[b] = valid ? ((unsigned long long)(uint32_t)best << 32) | (unsigned long long)__float_as_uint((float)(fl * (1.0 - 0x1p-20))) : 0ull;
        }
        int run = 0;
        for (int v = kPilotHyps; v >= 0; v--)
            for (int w = 0; w < kPilotHyps; w++) {
                s_off[w][v] = run;
                run += s_hist[w][v];
            }
    }
    __syncthreads();
    int off[kPilotHyps + 1];
#pragma unroll
    for (int v = 0; v <= kPilotHyps; v++) off[v] = s_off[wave][v];
    float *r = rk + (size_t)b * 4 * kp_pad;
    for (int g = g_lo; g < g_hi; g++) {
        const int i = g * 64 + lane;
        const bool valid = i < m;
        int key = 0;
        for (int w = 0; w < npil; w++) key += (int)((~s_bits[w][g] >> lane) & 1ull);
        int pos = 0;
#pragma unroll
        for (int v = 0; v <= kPilotHyps; v++) {
            const unsigned long long bal = __ballot(valid && key == v);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (key == v) pos = off[v] + rank;
            off[v] += __popcll(bal);
        }
        if (valid) {
            const int2 pr = PR[i];
            const float2 a = P1[pr.x], c = P2[pr.y];
            r[pos] = a.x;
            r[kp_pad + pos] = a.y;
            r[2 * kp_pad + pos] = c.x;
            r[3 * kp_pad + pos] = c.y;
        }
    }
    const int mpad = cnt_pad(m);
    if (m + tid < mpad) {   // at most 255 slots: lanes beyond m in the last sub-block read a real match (and are masked)
        const int2 pr = PR[m - 1];
        const float2 a = P1[pr.x], c = P2[pr.y];
        r[m + tid] = a.x;
        r[kp_pad + m + tid] = a.y;
        r[2 * kp_pad + m + tid] = c.x;
        r[3 * kp_pad + m + tid] = c.y;
    }
}

// pot0[pair][h] = how many of the kScreenMatches most-missed matches (the head) hypothesis h can have as inliers (everything
// the cheap evaluation does not certify as an outlier).  head[pair][h] = (how many of them it certainly has: g < lo, or
// kHeadUncertified after a zero / denormal / NaN dd; the sum of the head's cheap values): the count kernel starts behind
// the head with these and evaluates the head again only for a hypothesis that completes with pot0 != certain.
// Workgroup = 128 hypotheses, a wave walks 32 of them with two of the ranked matches per lane.  grid = (ceil(hyp / 128), batch).
// route_out (experiments build only): per pair, 1 = the certificate, 0 = the cheap evaluation, -1 = fewer than min_m matches.
#ifdef VSLAM_EXPERIMENTS
#define VS_SCREEN_ROUTE_PARAM , int32_t *__restrict__ route_out
#else
#define VS_SCREEN_ROUTE_PARAM
#endif
// kRows (experiments build only, VSLAM_RANSAC_PRUNE_ROWS): the head path in the row-per-hypothesis form it had before.
template <bool kRows>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7))) void ransac_screen_kernel(
    const float *__restrict__ rk, int kp_pad, const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp,
    float threshold, const float *__restrict__ hypF, const float *__restrict__ cmax, const int32_t *__restrict__ cbound,
    int32_t *__restrict__ pot0, int2 *__restrict__ head, float splus, int route VS_SCREEN_ROUTE_PARAM) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hbase = blockIdx.x * kScreenHyps;
    const int m = min(m_arr[b], kp_stride);
    const int bound_pilots = cbound[b];   // ransac_rank_kernel's: a count some hypothesis of the pair reaches (read beside m)
#ifdef VSLAM_EXPERIMENTS
    if (route_out && blockIdx.x == 0 && tid == 0)
        route_out[b] = m < min_m ? -1 : (vs_head_on_certificate(m, bound_pilots, min(m, kScreenMatches), route) ? 1 : 0);
#endif
    if (m < min_m) return;
    // The pair's head on the prune certificate instead (workgroup-uniform; the same 4 waves x 32 hypotheses).  One kernel with
    // this branch, not a launch of its own: a launch whose 8192 workgroups all return costs 0.006 to 0.012 ms
    // (profiles/r09_matrix_pipe_ab.txt section 3).  amdgpu_waves_per_eu(7, 7) above holds the two paths together to 72 vector
    // registers without a spill; left to itself the compiler takes 79 (six waves per SIMD) with the head counted in the lanes
    // (profiles/r10_prune_lanes_ab.txt section 1), and took 108 with the row-per-hypothesis head of round 9.
    if (vs_head_on_certificate(m, bound_pilots, min(m, kScreenMatches), route)) {
        static_assert(kScreenHyps == vs_prune::kPruneWaves * vs_prune::kPruneHyps && kScreenMatches <= vs_prune::kHeadTiles * vs_prune::kPruneTile,
                      "a wave of the screen is a wave of the prune tile");
        if (hbase + wave * 32 < hyp) {   // wave-uniform
#ifdef VSLAM_EXPERIMENTS
            if constexpr (kRows)
                vs_prune::head_on_certificate_rows(rk, kp_pad, b, m, min(m, kScreenMatches), hbase + wave * 32, hyp, threshold, splus, hypF, cmax, pot0, head);
            else
#endif
                vs_prune::head_on_certificate(rk, kp_pad, b, m, min(m, kScreenMatches), hbase + wave * 32, hyp, threshold, splus, hypF, cmax, pot0, head);
        }
        return;
    }
    __shared__ __align__(16) float s_rec[kScreenHyps * kCntRec];
    if (tid < kScreenHyps) {
        const float *src = hypF + ((size_t)b * hyp + min(hbase + tid, hyp - 1)) * 9;
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; k++) f[k] = src[k];
        const CntBand B = cnt_band(f, cmax[2 * b], cmax[2 * b + 1], threshold);
        cnt_store_record(s_rec + tid * kCntRec, f, B);
    }
    const int n0 = min(m, kScreenMatches);
    const float *r = rk + (size_t)b * 4 * kp_pad;
    const float2 x1 = *reinterpret_cast<const float2 *>(r + 2 * lane);
    const float2 y1 = *reinterpret_cast<const float2 *>(r + kp_pad + 2 * lane);
    const float2 x2 = *reinterpret_cast<const float2 *>(r + 2 * kp_pad + 2 * lane);
    const float2 y2 = *reinterpret_cast<const float2 *>(r + 3 * kp_pad + 2 * lane);
    v2f X1, Y1, X2, Y2;
    X1.x = x1.x; X1.y = x1.y; Y1.x = y1.x; Y1.y = y1.y;
    X2.x = x2.x; X2.y = x2.y; Y2.x = y2.x; Y2.y = y2.y;
    const unsigned long long va = __ballot(2 * lane < n0), vb = __ballot(2 * lane + 1 < n0);
    __syncthreads();
    int mine = 0;         // pot0 | certain << 8 (0xFF: not certified) of the hypothesis this lane reports
    float mine_sum = 0.f;
    const bool odd1 = (lane & 1) != 0, odd2 = (lane & 2) != 0;
    const bool in_a = 2 * lane < n0, in_b = 2 * lane + 1 < n0;
    constexpr int kU = 4;   // hypotheses in flight: the record reads and the dependent chain of one hide behind the others
    static_assert(kU == 4, "the head sums are reduced four hypotheses at a time");
    for (int j = 0; j < 32; j += kU) {
        CntRec R[kU];
        v2f dd[kU], g[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) cnt_load_record(R[u], s_rec, wave * 32 + j + u);
#pragma unroll
        for (int u = 0; u < kU; u++) g[u] = cnt_cheap(R[u], X1, Y1, X2, Y2, dd[u]);
        bool any_alive = false;   // wave-uniform: the counts are scalar
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const unsigned long long oa = __builtin_amdgcn_fcmpf(g[u].x, R[u].hi, kFcmpOGT), ob = __builtin_amdgcn_fcmpf(g[u].y, R[u].hi, kFcmpOGT);
            const unsigned long long ia = __builtin_amdgcn_fcmpf(g[u].x, R[u].lo, kFcmpOLT), ib = __builtin_amdgcn_fcmpf(g[u].y, R[u].lo, kFcmpOLT);
            int p = __popcll(va & ~oa) + __popcll(vb & ~ob);
            int c = __popcll(va & ia) + __popcll(vb & ib);
            // a zero / denormal (or NaN) dd: v_rcp_f32 is not a 1-ulp reciprocal there, nothing is certified
            if (__builtin_amdgcn_fcmpf(fminf(dd[u].x, dd[u].y), kCntTinyDD, kFcmpULT) != 0ull) {   // unordered or <
                p = n0;
                c = 0xFF;
            }
            mine = lane == j + u ? (p | (c << 8)) : mine;
            any_alive = any_alive || p + (m - n0) >= bound_pilots;
        }
        // The four head sums, reduced together in a fixed order: two exchange steps leave lane l with a partial sum of
        // hypothesis j + (l & 3), two row rotations and two cross-row exchanges add the 16 lanes of that class.  Lane j + u
        // is of class u, so it already holds the sum it reports.  Seven additions deep.
        // (Skipped where none of the four can survive: pot0 + the matches behind the head stays below the pilots' bound, and
        // the bound only rises from there, so ransac_count_kernel never reads their word.)
        if (!any_alive) continue;
        float v[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) v[u] = (in_a ? g[u].x : 0.f) + (in_b ? g[u].y : 0.f);
        const int z = 0;
        const float k01 = odd1 ? v[1] : v[0], t01 = odd1 ? v[0] : v[1], k23 = odd1 ? v[3] : v[2], t23 = odd1 ? v[2] : v[3];
        const float r01 = k01 + __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(t01), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
        const float r23 = k23 + __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(t23), 0xB1, 0xF, 0xF, false));
        const float kk = odd2 ? r23 : r01, tt = odd2 ? r01 : r23;
        float r = kk + __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(tt), 0x4E, 0xF, 0xF, false));             // quad_perm [2,3,0,1]
        r += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(r), 0x124, 0xF, 0xF, false));                       // row_ror:4
        r += __int_as_float(__builtin_amdgcn_update_dpp(z, __float_as_int(r), 0x128, 0xF, 0xF, false));                       // row_ror:8
        r += __shfl_xor(r, 16, 64);
        r += __shfl_xor(r, 32, 64);
        mine_sum = (lane >> 2) == (j >> 2) ? r : mine_sum;
    }
    const int h = hbase + wave * 32 + lane;
    if (lane < 32 && h < hyp) {
        const int c = mine >> 8;
        pot0[(size_t)b * hyp + h] = mine & 0xFF;
        head[(size_t)b * hyp + h] = make_int2(c == 0xFF ? kHeadUncertified : c, __float_as_int(mine_sum));
    }
}

// The hypotheses that do best on the screen (largest pot0, then one less, first indices, at most kCandMax) are counted in
// full, exactly: cbound[pair] = max(cbound[pair], those counts).  One workgroup of 8 waves per pair.
__global__ __launch_bounds__(64 * kCandMax) void ransac_cand_kernel(
    const float *__restrict__ rk, int kp_pad, const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp,
    float threshold, const float *__restrict__ hypF, const int32_t *__restrict__ pot0, int by_sum,
    int32_t *__restrict__ cbound, unsigned long long *__restrict__ sfloor) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = min(m_arr[b], kp_stride);
    if (m < min_m) return;
    __shared__ int s_max[kCandMax], s_l0[kCandMax][kCandMax], s_l1[kCandMax][kCandMax], s_n0[kCandMax], s_n1[kCandMax];
    __shared__ int s_cand[kCandMax], s_nc;
    const int32_t *P = pot0 + (size_t)b * hyp;
    int mx = -1;
    for (int i = tid; i < hyp; i += 64 * kCandMax) mx = max(mx, P[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_max[wave] = mx;
    __syncthreads();
    mx = s_max[0];
    for (int w = 1; w < kCandMax; w++) mx = max(mx, s_max[w]);
    // wave w scans its contiguous share in index order
    const int per = (hyp + kCandMax - 1) / kCandMax;
    const int lo = min(hyp, wave * per), hi = min(hyp, lo + per);
    int n0 = 0, n1 = 0;
    // (by_sum: the wave also notes the first 32 best-scoring hypotheses of its share -- a random sample: a hypothesis' index
    // says nothing about it -- and afterwards moves the one with the largest residual sum over the screen's matches to the
    // front.  Those matches are mostly the pair's outliers, whose residuals dominate a residual sum, so that candidate's sum
    // is likely to be near the largest among the hypotheses that tie the maximum count: what makes the sum floor below bite.)
    __shared__ int s_samp[kCandMax][32];
    int nsamp = 0;
    for (int i0 = lo; i0 < hi && ((by_sum && nsamp < 32) || n0 < kCandMax || n1 < kCandMax); i0 += 64) {
        const int i = i0 + lane;
        const int v = i < hi ? P[i] : -2;
        unsigned long long b0 = __ballot(v == mx), b1 = __ballot(v == mx - 1);
        if (by_sum) {
            const int rs = nsamp + __popcll(b0 & ((1ull << lane) - 1ull));
            if (v == mx && rs < 32) s_samp[wave][rs] = i;
            nsamp = min(32, nsamp + (int)__popcll(b0));
        }
        const int r0 = n0 + __popcll(b0 & ((1ull << lane) - 1ull)), r1 = n1 + __popcll(b1 & ((1ull << lane) - 1ull));
        if (v == mx && r0 < kCandMax) s_l0[wave][r0] = i;
        if (v == mx - 1 && r1 < kCandMax) s_l1[wave][r1] = i;
        n0 = min(kCandMax, n0 + __popcll(b0));
        n1 = min(kCandMax, n1 + __popcll(b1));
    }
    if (by_sum && nsamp > 1) {   // the sample's best by sum over the screen's matches to the front of the wave's list
        // (a ranking aid only: nothing is certified with these values; NaN / inf simply rank oddly)
        const int n128 = min(m, kScreenMatches);
        const float *r = rk + (size_t)b * 4 * kp_pad;
        const float2 x1 = *reinterpret_cast<const float2 *>(r + 2 * lane), y1 = *reinterpret_cast<const float2 *>(r + kp_pad + 2 * lane);
        const float2 x2 = *reinterpret_cast<const float2 *>(r + 2 * kp_pad + 2 * lane), y2 = *reinterpret_cast<const float2 *>(r + 3 * kp_pad + 2 * lane);
        v2f X1, Y1, X2, Y2;
        X1.x = x1.x; X1.y = x1.y; Y1.x = y1.x; Y1.y = y1.y;
        X2.x = x2.x; X2.y = x2.y; Y2.x = y2.x; Y2.y = y2.y;
        float fl[9];   // lane l < nsamp: the F of sample l
        {
            const int hs = s_samp[wave][lane < nsamp ? lane : 0];
            const float *src = hypF + ((size_t)b * hyp + hs) * 9;
#pragma unroll
            for (int k = 0; k < 9; k++) fl[k] = src[k];
        }
        float best_s = -INFINITY;
        int best_i = -1;
        for (int j = 0; j < nsamp; j++) {
            CntRec R;
#pragma unroll
            for (int k = 0; k < 9; k++) R.f[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fl[k]), j));
            v2f dd;
            const v2f g = cnt_cheap(R, X1, Y1, X2, Y2, dd);
            const float part = wave_sum_to_lane63((2 * lane < n128 ? g.x : 0.f) + (2 * lane + 1 < n128 ? g.y : 0.f));
            const float tot = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part), 63));
            if (tot > best_s) {   // false for NaN
                best_s = tot;
                best_i = s_samp[wave][j];
            }
        }
        if (lane == 0 && best_i >= 0 && n0 > 0) {
            const int old = s_l0[wave][0];
            for (int k = 1; k < n0; k++)
                if (s_l0[wave][k] == best_i) s_l0[wave][k] = old;
            s_l0[wave][0] = best_i;
        }
    }
    if (lane == 0) {
        s_n0[wave] = n0;
        s_n1[wave] = n1;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int w = 0; w < kCandMax && n < kCandMax; w++)   // every wave's first entry first (with ssum: its best by sum)
            if (s_n0[w] > 0) s_cand[n++] = s_l0[w][0];
        for (int w = 0; w < kCandMax && n < kCandMax; w++)
            for (int k = 1; k < s_n0[w] && n < kCandMax; k++) s_cand[n++] = s_l0[w][k];
        for (int w = 0; w < kCandMax && n < kCandMax; w++)
            for (int k = 0; k < s_n1[w] && n < kCandMax; k++) s_cand[n++] = s_l1[w][k];
        s_nc = n;
    }
    __syncthreads();
    // The sum floor (the counting kernel's second way of dropping a hypothesis): among hypotheses of equal count the accept
    // rule keeps the one with the LARGER residual sum (src/RansacFilter.cpp:59), so a candidate with exact count c and
    // residual sum s rules out every hypothesis that can at best tie c with a sum certainly below s.
    // sfloor[pair] = c << 32 | bits of a lower bound of s (a positive float: its bits order as the number does), so that
    // a 64-bit maximum is "the higher count, then the larger sum": ransac_rank_kernel stores the best pilot's, this kernel
    // keeps the larger of that and its own candidates'.  0 = no floor.
    __shared__ int s_ccount[kCandMax];
    __shared__ double s_csum[kCandMax];
    if (wave < s_nc) {
        const int h = s_cand[wave];
        double esum = 0;
        const int count = cnt_exact_ranked(hypF + ((size_t)b * hyp + h) * 9, rk + (size_t)b * 4 * kp_pad, kp_pad, m, threshold, lane, &esum);
        if (lane == 0) {
            atomicMax(&cbound[b], count);
            s_ccount[wave] = count;
            s_csum[wave] = esum;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int cb = -1;
        for (int k = 0; k < s_nc; k++) cb = max(cb, s_ccount[k]);
        double fl = -INFINITY;
        bool any_nan = false;
        for (int k = 0; k < s_nc; k++)
            if (s_ccount[k] == cb) {
                any_nan = any_nan || !(s_csum[k] == s_csum[k]);
                if (s_csum[k] > fl) fl = s_csum[k];
            }
        // a NaN sum among the best candidates takes part in the accept rule in ways a floor cannot express: no floor from them
        const bool valid = cb > 0 && !any_nan && fl > 0 && fl < 0x1p120;
        const float flf = (float)(fl * (1.0 - 0x1p-20));   // float rounding stays inside the 2^-20
        const unsigned long long mine = valid ? ((unsigned long long)(uint32_t)cb << 32) | (unsigned long long)__float_as_uint(flf) : 0ull;
        const unsigned long long pilots = sfloor[b];   // ransac_rank_kernel's: the higher count, then the larger sum
        sfloor[b] = mine > pilots ? mine : pilots;
    }
}

// grid = (ceil(hyp / 128), batch), block = 512; dynamic LDS = (LDS ? 16 B x cnt_pad(kp_stride) : 0) + 8 queues.
// LDS = false (more than kCntLdsMatches matches per pair): the ranked coordinates are read from memory instead.
// ZERO (experiments build only, VSLAM_RANSAC_COUNT_FROM_ZERO): the walk of before the head start -- every survivor begins
// at ranked match 0 with nothing seen and takes nothing but its survival from the screen.  For A/B timing and the identity test.
// exit_payload (a parameter of the experiments build only, VSLAM_RANSAC_COUNT_EXIT_PAYLOAD): the NaN in hyp_sum of an abandoned
// hypothesis carries the number of matches it had seen -- the histogram of tools/count_exit_hist.py.
#ifdef VSLAM_EXPERIMENTS
#define VS_CNT_PAYLOAD_PARAM , int exit_payload
#define VS_CNT_PAYLOAD_ARG , exit_payload
#else
#define VS_CNT_PAYLOAD_PARAM
#define VS_CNT_PAYLOAD_ARG
#endif
template <bool LDS, bool ZERO>
__global__ __launch_bounds__(64 * kCntWaves) __attribute__((amdgpu_waves_per_eu(6, 6))) void ransac_count_kernel(
    const float *__restrict__ rk, int kp_pad, const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, float threshold,
    const float *__restrict__ hypF, const int32_t *__restrict__ pot0, const int2 *__restrict__ head,
    const float *__restrict__ cmax, int32_t *__restrict__ hyp_count, float *__restrict__ hyp_sum, float *__restrict__ approx,
    int32_t *__restrict__ cbound, const unsigned long long *__restrict__ sfloor VS_CNT_PAYLOAD_PARAM) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform, and the compiler may know it
    const int hbase = blockIdx.x * kCntHyps;
    const int nh = min(kCntHyps, hyp - hbase);
    const int m = min(m_arr[b], kp_stride);
    if (m < min_m) return;   // uniform per workgroup

    __shared__ __align__(16) float s_rec[kCntHyps * kCntRec];
    __shared__ int s_cnt[kCntHyps];      // exact count: starts as the head's certain inliers where the screen's word is taken over
    __shared__ float s_part[kCntHyps];   // sum of the cheap values: starts as the screen's sum over the head (0 where not certified)
    // s_state also carries, from bit 2 up, what the screen found: pot0 | kHeadMine (the head has to be evaluated here if the walk
    // completes) | kHeadNoSum -- a fifth array of 512 B would, at 2000 keypoints, cost the third workgroup per CU
    constexpr int kHeadMine = 0x10000, kHeadNoSum = 0x20000;
    __shared__ int s_unk[kCntHyps];      // hypothesis whose cheap sum is not certified
    __shared__ int s_state[kCntHyps];    // 0 = ruled out by the screen, 1 = counted in full, 2 = abandoned on the way
    __shared__ int s_list[kCntHyps];     // survivors of the screen: [64 w, 64 w + s_nlist[w]) found by wave w
    constexpr int kListWaves = kCntHyps / 64;
    static_assert(kCntHyps % 64 == 0 && kListWaves <= kCntWaves, "whole waves find the survivors");
    __shared__ int s_nlist[kListWaves], s_next, s_bound;
    extern __shared__ __align__(16) uint32_t s_dyn[];

    const int n0 = min(m, kScreenMatches);
    const int bound0 = cbound[b];   // a count some hypothesis of this pair is known to reach (never above the true maximum)
    if (tid < kCntHyps) {           // whole waves
        const int p0 = tid < nh ? pot0[(size_t)b * hyp + hbase + tid] : 0;
        const bool alive = tid < nh && p0 + (m - n0) >= bound0;
        int certain = 0, word = p0;
        float hsum = 0.f;
        if (!ZERO && alive) {
            // certain == pot0: every evaluation of the head was decided, and decided with a certified band (an
            // uncertified head reads kHeadUncertified, which no pot0 equals): the head's count is `certain`
            const int2 hd = head[(size_t)b * hyp + hbase + tid];
            if (hd.x == p0) certain = hd.x;
            else word |= kHeadMine;
            if (hd.x != kHeadUncertified) hsum = __int_as_float(hd.y);
            else word |= kHeadNoSum;
        }
        s_cnt[tid] = certain;
        s_unk[tid] = 0;
        s_part[tid] = hsum;
        s_state[tid] = (alive ? 1 : 0) | (ZERO ? 0 : word << 2);
        const unsigned long long bal = __ballot(alive);
        if (alive) s_list[wave * 64 + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
        if (lane == 0) s_nlist[wave] = __popcll(bal);
    }
    if (tid == 0) {
        s_next = 0;
        s_bound = bound0;
    }
    __syncthreads();
    int n_alive = 0;
#pragma unroll
    for (int w = 0; w < kListWaves; w++) n_alive += s_nlist[w];
    const size_t out = (size_t)b * hyp + hbase + tid;
    if (n_alive == 0) {   // the usual case on a pair whose maximum only a few hypotheses reach
        if (tid < nh) {
            hyp_count[out] = -1;
            hyp_sum[out] = __int_as_float(0x7FC00000);
            reinterpret_cast<float2 *>(approx)[out] = make_float2(0.f, INFINITY);
        }
        return;
    }

    double my_beta = 0;     // thread t < 128 keeps hypothesis t's beta for the bound on its cheap sum
    bool my_ok = false;
    if (tid < kCntHyps && (s_state[tid] & 3)) {   // the survivors' records: F, lo, hi
        const float *src = hypF + ((size_t)b * hyp + hbase + tid) * 9;
        float f[9];
#pragma unroll
        for (int k = 0; k < 9; k++) f[k] = src[k];
        const CntBand B = cnt_band(f, cmax[2 * b], cmax[2 * b + 1], threshold);
        my_beta = B.beta;
        my_ok = B.ok;
        cnt_store_record(s_rec + tid * kCntRec, f, B);
    }
    const int mpad = cnt_pad(m);
    const float *rg = rk + (size_t)b * 4 * kp_pad;
    float *s_co = reinterpret_cast<float *>(s_dyn);
    if (LDS) {
        for (int k = tid * 4; k < mpad; k += 64 * kCntWaves * 4) {
#pragma unroll
            for (int a = 0; a < 4; a++)
                *reinterpret_cast<float4 *>(s_co + a * mpad + k) = *reinterpret_cast<const float4 *>(rg + (size_t)a * kp_pad + k);
        }
    }
    __syncthreads();
    const int cstride = LDS ? mpad : kp_pad;
    const float *cx1 = LDS ? s_co : rg;
    const float *cy1 = cx1 + cstride, *cx2 = cx1 + 2 * cstride, *cy2 = cx1 + 3 * cstride;

    {
        cnt_queue_t *q = (cnt_queue_t *)(s_dyn + (LDS ? 4 * mpad : 0) + wave * kCntQueue);
        int qn = 0;
        int bound = bound0;
        // the sum floor of ransac_cand_kernel: (the count it belongs to, a lower bound of that hypothesis' residual sum); -1: none
        const unsigned long long fkey = sfloor ? sfloor[b] : 0ull;
        const int floor_count = fkey != 0ull ? (int)(fkey >> 32) : -1;
        const float floor_sum = __uint_as_float((uint32_t)fkey);
        // the walk's origin: behind the screen's matches, which every survivor has been evaluated on already
        const int org = ZERO ? 0 : n0;
        const int nsub = (m - org + 255) >> 8;
        const bool part = ((m - org) & 255) != 0;
        // additions on the longest path to a cheap sum: two per sub-block and lane (the head block included where it is
        // evaluated here), one across the pair of accumulators, six across the lanes, one for the screen's head sum
        const float sum_rel = cnt_sum_rel(2 * nsub + 9);
        // the survivors are handed out one at a time: what a hypothesis costs (256 evaluations or all of them) is not known beforehand
        int k = 0;
        if (lane == 0) k = atomicAdd(&s_next, 1);
        k = __builtin_amdgcn_readfirstlane(k);
        while (k < n_alive) {
            int knext = 0;
            if (lane == 0) knext = atomicAdd(&s_next, 1);   // consumed at the bottom: the round trip hides behind the work
            int hh;
            {
                int kk = k, w = 0;
                while (w + 1 < kListWaves && kk >= s_nlist[w]) kk -= s_nlist[w++];
                hh = s_list[w * 64 + kk];
            }
            bound = max(bound, *(__attribute__((address_space(3))) const volatile int *)&s_bound);
            CntRec R;
            cnt_load_record(R, s_rec, hh);
            // what the screen found on the head: the walk goes on from there (ZERO: nothing is taken over)
            // (broadcast reads, waited for where they are first used: behind the first block's evaluation)
            const int word = ZERO ? 0 : s_state[hh] >> 2;
            const int head_cnt = ZERO ? 0 : *(__attribute__((address_space(3))) const volatile int *)&s_cnt[hh];   // nobody has added to it yet
            float head_sum = ZERO ? 0.f : s_part[hh];
            int cnt = 0, pot = word & 0xFFFF, seen = org;
            bool dropped = false, unk = false;
            v2f acc;
            acc.x = 0.f;
            acc.y = 0.f;
            // Where the screen left something of the head open (an evaluation inside the band, a NaN, an uncertified head),
            // the head is one more block behind the last: reached only by a walk that completes, evaluated like any other
            // (the undecided ones queued), its cheap values summed here (the screen's sum is then not added).
            // (the screen's word is looked at only once the walk is through: the first block's reads do not wait for it)
            for (int s = 0;; s++) {
                if (s >= nsub && (ZERO || s > nsub || !(word & kHeadMine))) break;
                // the lane's four matches of this sub-block: straight from LDS (six waves per SIMD hide the round trip;
                // fetching a sub-block ahead cost 16 registers and a copy per value)
                const bool hd = !ZERO && s == nsub;
                const int pot_walk = pot;
                const int ix = (hd ? 0 : org + s * 256) + 4 * lane;
                const int il = min(ix, mpad - 4);   // the arrays end at mpad: lanes beyond it (all beyond m) read its last slots
                const float4 X1 = *reinterpret_cast<const float4 *>(cx1 + il), Y1 = *reinterpret_cast<const float4 *>(cy1 + il);
                const float4 X2 = *reinterpret_cast<const float4 *>(cx2 + il), Y2 = *reinterpret_cast<const float4 *>(cy2 + il);
                if (hd || (s == nsub - 1 && part)) {
                    cnt_sub_block<true>(R, X1, Y1, X2, Y2, ix, hh, lane, hd ? n0 : m, cnt, q, qn, acc, s_unk, pot, unk);
                    seen += hd ? 0 : (m - org) & 255;
                } else {
                    cnt_sub_block<false>(R, X1, Y1, X2, Y2, ix, hh, lane, m, cnt, q, qn, acc, s_unk, pot, unk);
                    seen += 256;
                }
                while (qn >= 64) {   // a sub-block adds at most 256 words to the 63 left over: kCntQueue holds them
                    cnt_drain(q, qn - 64, 64, lane, s_rec, s_cnt, cx1, cy1, cx2, cy2, threshold);
                    qn -= 64;
                }
                if (hd) {
                    head_sum = 0.f;
                    pot = pot_walk;   // the head's potential inliers are in pot0 already
                    break;
                }
                // Bail-out.  Even if every match not looked at yet were an inlier, the hypothesis would stay below a
                // count some hypothesis of this pair is already known to reach: it cannot be a maximum-count hypothesis,
                // which is all the accept rule looks at.  `bound` never exceeds the true maximum, so every hypothesis
                // that reaches the maximum is counted in full.
                if (pot + (m - seen) < bound) {
                    dropped = true;
                    break;
                }
                // The sum rule.  The hypothesis can at best TIE the count the floor belongs to (every match not looked at
                // yet would have to be an inlier, i.e. add at most `threshold` each to its residual sum), and among equal
                // counts the accept rule keeps the larger sum: if an upper bound of its sum -- the cheap values so far,
                // their certified error (the bound ransac_ties uses, over `seen` evaluations), threshold x the rest --
                // lies below the floor by more than float rounding can close, it is neither the winner nor a tie.
                // On data with one dominant motion a third to a half of the hypotheses share the maximum count and used to
                // be counted in full for that; their sums are far from the best one's (outlier residuals dominate them).
                // (The head's share of the cheap sum is the screen's, where the screen certified it.)
                if (seen < m && bound == floor_count && pot + (m - seen) == bound && !unk && R.beta >= 0.f && !(word & kHeadNoSum)) {
                    // in float, every rounding covered by the 1e-4 factors (the terms are all positive)
                    const float S = head_sum + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum_to_lane63(acc.x + acc.y)), 63));
                    const float ns = (float)seen;
                    const float err = (2.02f * R.beta * sqrtf(ns * S) + ns * R.beta * R.beta + sum_rel * S) * 1.0001f;
                    const float upper = ((S + err) + threshold * (float)(m - seen)) * 1.0001f;
                    if (upper < floor_sum * 0.9999f) {   // false for NaN
                        dropped = true;
                        break;
                    }
                }
            }
            if (dropped) {
#ifdef VSLAM_EXPERIMENTS
                if (lane == 0) s_state[hh] = 2 | (seen << 2);
#else
                if (lane == 0) s_state[hh] = 2;
#endif
            } else {
                const float part_sum = head_sum + wave_sum_to_lane63(acc.x + acc.y);
                // The sum rule once more, over the whole walk (nothing is left to assume about matches not seen): a hypothesis
                // that can at best tie the floor's count with a sum certainly below the floor reports -1 like one abandoned on
                // the way.  Along a walk an unseen match is charged `threshold` and a seen potential inlier its own cheap value,
                // so this last use is as a rule the tightest, and which tied hypotheses read -1 then follows from the whole
                // walk's sum, not from where a sub-block happened to end.  That is not a guarantee (an evaluation inside the
                // band is charged up to hi, the error term grows with the matches seen, and the cheap sums round differently
                // in another summation order): a hypothesis within those margins of the floor may read -1 under one block
                // layout and carry its count under another.  Either is correct: it is beaten on the sum.
                bool beaten = false;
                if (bound == floor_count && pot == bound && !unk && R.beta >= 0.f) {
                    const float S = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part_sum), 63));
                    const float ns = (float)m;
                    const float err = (2.02f * R.beta * sqrtf(ns * S) + ns * R.beta * R.beta + sum_rel * S) * 1.0001f;
                    beaten = (S + err) * 1.0001f < floor_sum * 0.9999f;   // false for NaN
                }
                if (lane == 63) s_part[hh] = part_sum;
                const int certain = head_cnt + cnt;
                if (beaten) {
#ifdef VSLAM_EXPERIMENTS
                    if (lane == 0) s_state[hh] = 2 | (seen << 2);
#else
                    if (lane == 0) s_state[hh] = 2;
#endif
                } else if (lane == 0) {
                    if (cnt) atomicAdd(&s_cnt[hh], cnt);
                    if (certain > bound) {   // the certain inliers alone are a count this hypothesis verifiably reaches
                        atomicMax(&s_bound, certain);
                        atomicMax(&cbound[b], certain);   // fire and forget: workgroups of this pair that start later begin with it
                    }
                }
                if (!beaten) bound = max(bound, certain);
            }
            k = __builtin_amdgcn_readfirstlane(knext);
        }
        if (qn > 0) cnt_drain(q, 0, qn, lane, s_rec, s_cnt, cx1, cy1, cx2, cy2, threshold);
    }
    __syncthreads();
    if (tid < nh) {
        const int st = s_state[tid] & 3;
        hyp_count[out] = st == 1 ? s_cnt[tid] : -1;     // ransac_ties keeps the maximal ones
        int nan_bits = 0x7FC00000;                      // defined by ransac_ties / tiesum where it matters
#ifdef VSLAM_EXPERIMENTS
        if (exit_payload && st != 1) nan_bits |= st == 2 ? min(s_state[tid] >> 2, 0x3FFFFF) : 0x3FFFFF;   // all ones: ruled out by the screen
#endif
        hyp_sum[out] = __int_as_float(nan_bits);
        // The cheap values' sum S~ and a bound on |S~ - (exact double sum of the e)|: per evaluation
        // |g - e| <= 12 u max(g, e) + beta (2 sqrt(g) + beta)  (the derivation above), summed with Cauchy-Schwarz
        // (sum sqrt(g_i) <= sqrt(M sum g_i)), plus the relative term
        // (terms and additions: cnt_sum_rel) for the rounding between g and e and the float additions that formed S~.
        const float S = st == 1 ? s_part[tid] : 0.f;
        float err = INFINITY;
        if (st == 1 && my_ok && !s_unk[tid]) {
            const double Sd = (double)S;
            const double rel = (double)cnt_sum_rel(2 * ((m - (ZERO ? 0 : n0) + 255) >> 8) + 9);
            err = (float)((2.02 * my_beta * sqrt((double)m * Sd) + (double)m * my_beta * my_beta + rel * Sd) * (1.0 + 0x1p-20));
        }
        reinterpret_cast<float2 *>(approx)[out] = make_float2(S, err);
    }
}

}  // namespace

int vs_launch_ransac_count(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs, const int32_t *m,
                           const float *hypF, int batch, int kp_stride, int hyp, float threshold, int32_t *hyp_count,
                           float *hyp_sum, float *approx) {
    const int min_m = ctx->ransac_min_matches;
    int rc;
    int32_t *cbound = nullptr, *pot0 = nullptr;
    float *rk = nullptr, *cmax = nullptr;
    const int kp_pad = cnt_pad(kp_stride);
    if ((rc = vs_arena_get(ctx, "ransac.cbound", sizeof(int32_t) * (size_t)batch, (void **)&cbound))) return rc;
    unsigned long long *sfloor = nullptr;
    if ((rc = vs_arena_get(ctx, "ransac.sfloor", sizeof(unsigned long long) * (size_t)batch, (void **)&sfloor))) return rc;
    static const bool no_sum_rule = VS_EXPERIMENT_ENV("VSLAM_RANSAC_NO_SUM_RULE") != nullptr;   // A/B timing: bail out on counts only
    // A/B timing and the identity test: the walk from ranked match 0 (read at every call: a test switches it within a process)
    const bool from_zero = VS_EXPERIMENT_ENV("VSLAM_RANSAC_COUNT_FROM_ZERO") != nullptr;
#ifdef VSLAM_EXPERIMENTS
    const int exit_payload = VS_EXPERIMENT_ENV("VSLAM_RANSAC_COUNT_EXIT_PAYLOAD") != nullptr ? 1 : 0;
#endif
    int2 *head = nullptr;
    if ((rc = vs_arena_get(ctx, "ransac.head", sizeof(int2) * (size_t)batch * hyp, (void **)&head))) return rc;
    const unsigned long long *use_floor = no_sum_rule ? nullptr : sfloor;
    if ((rc = vs_arena_get(ctx, "ransac.pot0", sizeof(int32_t) * (size_t)batch * hyp, (void **)&pot0))) return rc;
    if ((rc = vs_arena_get(ctx, "ransac.rk", sizeof(float) * 4 * (size_t)kp_pad * batch, (void **)&rk))) return rc;
    if ((rc = vs_arena_get(ctx, "ransac.cmax", sizeof(float) * 2 * (size_t)batch, (void **)&cmax))) return rc;
    {
        VsProfScope ps(ctx, "ransac_rank_kernel");
        ransac_rank_kernel<<<batch, kRankThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, min_m, kp_stride, kp_pad, hyp, threshold, hypF,
                                                                    cbound, rk, cmax, sfloor);
    }
    // the head of a pair: by the cheap evaluation (exact counts and sums handed on) or, where the hypotheses have to miss more
    // than the head holds, by the prune certificate on the matrix cores (vs_head_on_certificate)
    int route = -1;
    if (const char *e = VS_EXPERIMENT_ENV("VSLAM_RANSAC_HEAD_ROUTE")) route = atoi(e) ? 1 : 0;   // the tests force either path (read at every call)
#ifdef VSLAM_EXPERIMENTS
    int32_t *route_out = nullptr, *pot0_out = nullptr;   // what vslam_debug_ransac_head (ransac_prune.hip) hands out
    if ((rc = vs_arena_get(ctx, "ransac.head_route", sizeof(int32_t) * (size_t)batch, (void **)&route_out))) return rc;
    if ((rc = vs_arena_get(ctx, "ransac.head_pot0", sizeof(int32_t) * (size_t)batch * hyp, (void **)&pot0_out))) return rc;
#endif
    {
        VsProfScope ps(ctx, "ransac_screen_kernel");
        dim3 grid(vs_div_up(hyp, kScreenHyps), batch);
#ifdef VSLAM_EXPERIMENTS
        if (vs_prune_rows_form())
            ransac_screen_kernel<true><<<grid, 256, 0, ctx->stream>>>(rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, cmax, cbound, pot0, head,
                                                                      pc_splus(threshold), route, route_out);
        else
            ransac_screen_kernel<false><<<grid, 256, 0, ctx->stream>>>(rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, cmax, cbound, pot0, head,
                                                                       pc_splus(threshold), route, route_out);
#else
        ransac_screen_kernel<false><<<grid, 256, 0, ctx->stream>>>(rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, cmax, cbound, pot0, head,
                                                                   pc_splus(threshold), route);
#endif
    }
#ifdef VSLAM_EXPERIMENTS   // pot0 as the screen leaves it, before ransac_prune marks the dead
    VS_HIP(ctx, hipMemcpyAsync(pot0_out, pot0, sizeof(int32_t) * (size_t)batch * hyp, hipMemcpyDeviceToDevice, ctx->stream));
#endif
    {
        VsProfScope ps(ctx, "ransac_cand_kernel");
        ransac_cand_kernel<<<batch, 64 * kCandMax, 0, ctx->stream>>>(rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, pot0,
                                                                     no_sum_rule ? 0 : 1, cbound, sfloor);
    }
    // cbound is final for the small kernels in front: what certainly stays below it is ruled out on the matrix cores
    if ((rc = vs_launch_ransac_prune(ctx, rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, cmax, cbound, pot0, batch, kScreenMatches)))
        return rc;
    if (int arc = vs_aux_job_point(ctx, 4)) return arc;
    {
        VsProfScope ps(ctx, "ransac_count_kernel");
        const bool lds = kp_pad <= kCntLdsMatches;
        const size_t dyn = (lds ? sizeof(float) * 4 * (size_t)kp_pad : 0) + sizeof(uint32_t) * kCntQueue * kCntWaves;
        const size_t dyn_max = sizeof(float) * 4 * kCntLdsMatches + sizeof(uint32_t) * kCntQueue * kCntWaves;
        dim3 grid(vs_div_up(hyp, kCntHyps), batch);
#ifdef VSLAM_EXPERIMENTS
        if (from_zero) {
            if (dyn > 32 * 1024 && (rc = vs_allow_dynamic_lds(ctx, ransac_count_kernel<true, true>, "ransac_count_from_zero", dyn_max)))
                return rc;
            if (lds)
                ransac_count_kernel<true, true><<<grid, 64 * kCntWaves, dyn, ctx->stream>>>(
                    rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, pot0, head, cmax, hyp_count, hyp_sum, approx, cbound,
                    use_floor VS_CNT_PAYLOAD_ARG);
            else
                ransac_count_kernel<false, true><<<grid, 64 * kCntWaves, dyn, ctx->stream>>>(
                    rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, pot0, head, cmax, hyp_count, hyp_sum, approx, cbound,
                    use_floor VS_CNT_PAYLOAD_ARG);
            return VSLAM_OK;
        }
#endif
        (void)from_zero;
        if (dyn > 32 * 1024 &&   // beyond the default static + dynamic LDS limit
            (rc = vs_allow_dynamic_lds(ctx, ransac_count_kernel<true, false>, "ransac_count", dyn_max)))
            return rc;
        if (lds)
            ransac_count_kernel<true, false><<<grid, 64 * kCntWaves, dyn, ctx->stream>>>(
                rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, pot0, head, cmax, hyp_count, hyp_sum, approx, cbound,
                    use_floor VS_CNT_PAYLOAD_ARG);
        else
            ransac_count_kernel<false, false><<<grid, 64 * kCntWaves, dyn, ctx->stream>>>(
                rk, kp_pad, m, min_m, kp_stride, hyp, threshold, hypF, pot0, head, cmax, hyp_count, hyp_sum, approx, cbound,
                    use_floor VS_CNT_PAYLOAD_ARG);
    }
    return VSLAM_OK;
}
