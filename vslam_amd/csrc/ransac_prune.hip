// RANSAC fundamental-matrix loop, between stages 3a (screen, candidates) and 3b (count): hypotheses that certainly cannot
// reach the pair's maximum count are ruled out on the f32 matrix cores before ransac_count_kernel walks them.
//
// Replaces nothing of the reference: it removes work of ransac_count_kernel (ransac_count.hip), whose results it cannot change
// -> ransac_prune_mfma_kernel.
//
// Numerics: one-sided.  The kernel only ever says "this match is certainly not an inlier of this hypothesis"
// (ransac_prune_cert.h: the derivation), counts those per hypothesis, and marks a hypothesis dead when the certified misses
// alone keep it below a count some hypothesis of the pair verifiably reaches.  Inlier decisions, counts and sums stay where
// they were: the cheap evaluation and the exact sequence of ransac_count.hip.
//
// Why.  On data with 40-45 % outliers nearly every hypothesis is garbage, and ransac_count_kernel spends its time certifying
// that each of them misses D = m - bound + 1 matches, at the price of a full cheap evaluation each.  A miss needs far less:
// e >= q = n^2 / a0^2, so |n| > sqrt(thr) |a0| with margins proves it.  n = sum_k F_k phi_k is bilinear in the hypothesis and
// the match's design-matrix row phi = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1), a0 = F_0..2 . (x1, y1, 1): two small
// GEMMs (hypotheses x matches, K = 9 and K = 3) that v_mfma_f32_32x32x2_f32 computes as exact-f32 fma chains on the matrix
// pipe, which is idle in this part of the step.  Per 64 results one v_fma and one v_cmp remain on the vector pipe.
//
// Mapping.  A wave owns 32 hypotheses of a pair: the COLUMNS of a 32 x 32 tile, the B operand (F, K padded to 10 for n and to
// 4 for a0).  It walks the ranked matches behind the head ([n0, m), most-missed first: ransac_rank_kernel), 32 per tile: the
// rows, the A operand, phi formed from the four coordinates.  Operand layout of v_mfma_f32_32x32x2_f32: lane l holds
// A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31]; accumulator register r of lane l holds row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.  So lane l holds hypothesis l & 31, and its sixteen result registers are
// sixteen MATCHES of that one hypothesis (the lane l ^ 32 holds the other sixteen).  Everything per hypothesis is per lane:
// the margin c, the limit, and the count of certified misses -- a v_cmp per register whose carry is added into the lane's own
// counter; X[h] is the counter of lane h plus that of lane h + 32, one cross-lane read at each look.  (The transposed
// tile, a hypothesis per row, computes the same fma chain per element -- products commute, k runs in the same order -- but
// spreads a hypothesis over the lanes: its misses then leave the vector pipe as compare masks for 64 s_bcnt1 and as many
// scalar counters per tile pair, and the scalar unit, shared by a CU's four SIMDs, becomes a third loaded unit.)
//
// A hypothesis h with X[h] certified misses behind the head is dead when pot0[h] + (m - n0) - X[h] < cbound[pair]: pot0 bounds
// its inliers on the head (ransac_screen_kernel, either path), m - n0 - X[h] those behind it.  A dead hypothesis gets
// pot0[h] = -(m - n0) - 1, with which ransac_count_kernel's own `alive` test is false (cbound >= 0), and reports -1.  Nothing
// else is written: survivors keep pot0 and head.  What the accept rule can see is unchanged by construction: a dead hypothesis is
// below the pair's maximum count, and ransac_ties_kernel writes -1 for every such hypothesis whatever the count kernel found.
// That the count kernel ALONE would have reported -1 for it is not guaranteed: a certified miss here need not be a certain
// outlier (g > hi) of the cheap evaluation there, so a below-bound hypothesis may survive that kernel's walk with its exact count
// where this kernel cuts it short.  Both are correct (the same holds of the sum rule, ransac_count.hip); hyp_count after
// ransac_ties is the same either way, which is what tests/test_gpu_prune.py compares.
//
// Work limits (speed only, never results): pairs with m < min_m or m <= n0 are skipped, and so are pairs with D <= n0 (the gate:
// there the screen has ruled the garbage out already); so are hypotheses the screen has ruled out or that lie outside the
// certificate's stated ranges, and a wave returns when it has none left; a wave stops once all its 32 hypotheses are dead,
// and once every live one has missed fewer than half of the matches seen so far -- a plateau of good hypotheses (easy data,
// photographs), of which nothing can be pruned.  Both are looked at every 64 matches.  A wave walks until its slowest
// hypothesis is dead: on the hard data nearly every wave goes 400 matches or more behind the head.
#include "ransac_prune_tile.h"

namespace {
using namespace vs_prune;

constexpr int kPruneStep = 2;     // tiles between two looks at the stop rules
// Chosen by measurement (profiles/r08_prune_ab.txt section 5, HISTORY.md round 8): a wave walks all matches behind the head
// (limits of 256 and 512 were slower), and the plateau rule stops at half of the matches seen (3/4 and no rule: no gain).
// The pair-level gate (in the kernel) can be switched off in the experiments build (VSLAM_RANSAC_PRUNE_GATE=0): the tests
// walk the pairs it skips that way.

#ifdef VSLAM_EXPERIMENTS
#define VS_PRUNE_X_PARAM , int32_t *__restrict__ x_out
#else
#define VS_PRUNE_X_PARAM
#endif

// grid = (ceil(hyp / 128), batch), block = 256: four independent waves, no LDS.  gate: 0 switches the pair-level gate off.
// x_out (experiments build only): X[h] of every hypothesis a wave has walked (zeroed by the launcher).
// amdgpu_waves_per_eu(4): a promise of at most 128 registers, without which the compiler puts the tiles into accumulation
// registers (the launch bounds alone allow a wave 512) and copies every result out with a v_accvgpr_read before the vector
// pipe can compare it: 64 more vector instructions per trip.  The kernel takes 57.
__global__ __launch_bounds__(64 * kPruneWaves) __attribute__((amdgpu_waves_per_eu(4))) void ransac_prune_mfma_kernel(
    const float *__restrict__ rk, int kp_pad, const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, float threshold,
    float splus, const float *__restrict__ hypF, const float *__restrict__ cmax, const int32_t *__restrict__ cbound, int32_t *__restrict__ pot0,
    int n_head, int gate VS_PRUNE_X_PARAM) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, col = lane & 31;
    const bool half = lane >= 32;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = min(m_arr[b], kp_stride);
    const int bound = cbound[b];   // read beside m, not behind it: a pair the gate skips costs one round trip, not two
    if (m < min_m) return;
    const int n0 = min(m, n_head);
    const int hbase = (blockIdx.x * kPruneWaves + wave) * kPruneHyps;
    if (m <= n0 || hbase >= hyp) return;   // wave-uniform
    // The gate.  A hypothesis has to miss D = m - bound + 1 matches to be out.  With D <= n0 the screen has seen enough matches --
    // the most-missed ones -- to rule a garbage hypothesis out by itself, and has: what it left alive misses few of them, a
    // plateau of good hypotheses this kernel cannot prune either (easy data: + 0.05 ms per step for nothing without the gate).
    if (gate && m - bound + 1 <= n0) return;

    // the lane's hypothesis (both halves hold the same 32), and whether anything is left to prove about it
    const int h = hbase + col;
    const size_t hi = (size_t)b * hyp + min(h, hyp - 1);
    const int behind = m - n0;
    const int lim = pot0[hi] + behind - bound;   // certified misses it can take and still reach the bound
    bool live0 = h < hyp && lim >= 0 && lim < behind;   // lim >= behind: not even `behind` misses kill it
    if (__ballot(live0) == 0ull) return;
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = hypF[hi * 9 + k];
    const float c = pc_margin(f, cmax[2 * b], cmax[2 * b + 1], threshold, splus);
    live0 = live0 && c < INFINITY;
    if (__ballot(live0) == 0ull) return;
    const PruneA A = prune_operands(f, half);

    const float *r1 = rk + (size_t)b * 4 * kp_pad, *r2 = r1 + kp_pad, *r3 = r2 + kp_pad, *r4 = r3 + kp_pad;
    const int row4 = half ? 4 : 0;   // the lane's part of prune_row
    int cnt = 0;   // certified misses of the lane's hypothesis among the matches its half has held
    int xv = 0;    // X of hypothesis l & 31 at the last look: cnt of both halves
    const int end = m;
    for (int base = n0; base < end; base += kPruneStep * kPruneTile) {
        float x1[kPruneStep], y1[kPruneStep], x2[kPruneStep], y2[kPruneStep];
#pragma unroll
        for (int t = 0; t < kPruneStep; t++) {
            const int j = min(base + t * kPruneTile + col, m - 1);   // rows beyond m read a real match and are masked
            x1[t] = r1[j];
            y1[t] = r2[j];
            x2[t] = r3[j];
            y2[t] = r4[j];
        }
        if (base + kPruneStep * kPruneTile <= end) {   // wave-uniform: full tiles, one block of code for the scheduler
#pragma unroll
            for (int t = 0; t < kPruneStep; t++) {
                v16f n, a0;
                prune_tile(A, half, x1[t], y1[t], x2[t], y2[t], n, a0);
                cnt = prune_count(n, a0, splus, c, cnt);
            }
        } else {   // only a pair's last trip: rows of a tile at and beyond `end` count nothing
#pragma unroll
            for (int t = 0; t < kPruneStep; t++) {
                v16f n, a0;
                prune_tile(A, half, x1[t], y1[t], x2[t], y2[t], n, a0);
                cnt = prune_count(n, a0, splus, c, cnt, end - (base + t * kPruneTile) - row4);
            }
        }
        // the stop rules, as one ballot: nobody is alive, or no live hypothesis has missed half of the matches seen so far
        // (the second contains the first)
        xv = cnt + __shfl_xor(cnt, 32, 64);
        const int seen = min(base + kPruneStep * kPruneTile, end) - n0;
        const bool alive = live0 && xv <= lim;
        if (__ballot(alive && 2 * xv >= seen) == 0ull) break;
    }
    if (!half && h < hyp) {
        if (live0 && xv > lim) pot0[hi] = -behind - 1;
#ifdef VSLAM_EXPERIMENTS
        if (x_out) x_out[hi] = xv;
#endif
    }
}

#ifdef VSLAM_EXPERIMENTS
// (experiments build only, VSLAM_RANSAC_PRUNE_ROWS=1) The walk this kernel replaced, a hypothesis per tile row
// (prune_tile_rows, ransac_prune_tile.h): the same tiles walked, the same X and the same dead, for the identity test
// (tests/test_gpu_prune_lanes.py) and for A/B timing inside one library.
__global__ __launch_bounds__(64 * kPruneWaves) void ransac_prune_rows_kernel(
    const float *__restrict__ rk, int kp_pad, const int32_t *__restrict__ m_arr, int min_m, int kp_stride, int hyp, float threshold,
    float splus, const float *__restrict__ hypF, const float *__restrict__ cmax, const int32_t *__restrict__ cbound, int32_t *__restrict__ pot0,
    int n_head, int gate, int32_t *__restrict__ x_out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, col = lane & 31;
    const bool half = lane >= 32;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = min(m_arr[b], kp_stride);
    const int bound = cbound[b];   // read beside m, not behind it: a pair the gate skips costs one round trip, not two
    if (m < min_m) return;
    const int n0 = min(m, n_head);
    const int hbase = (blockIdx.x * kPruneWaves + wave) * kPruneHyps;
    if (m <= n0 || hbase >= hyp) return;   // wave-uniform
    // The gate.  A hypothesis has to miss D = m - bound + 1 matches to be out.  With D <= n0 the screen has seen enough matches --
    // the most-missed ones -- to rule a garbage hypothesis out by itself, and has: what it left alive misses few of them, a
    // plateau of good hypotheses this kernel cannot prune either (easy data: + 0.05 ms per step for nothing without the gate).
    if (gate && m - bound + 1 <= n0) return;

    // the lane's hypothesis (both halves hold the same 32), and whether anything is left to prove about it
    const int h = hbase + col;
    const size_t hi = (size_t)b * hyp + min(h, hyp - 1);
    const int behind = m - n0;
    const int lim = pot0[hi] + behind - bound;   // certified misses it can take and still reach the bound
    bool live0 = h < hyp && lim >= 0 && lim < behind;   // lim >= behind: not even `behind` misses kill it
    if (__ballot(live0) == 0ull) return;
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = hypF[hi * 9 + k];
    const float c = pc_margin(f, cmax[2 * b], cmax[2 * b + 1], threshold, splus);
    live0 = live0 && c < INFINITY;
    if (__ballot(live0) == 0ull) return;
    const PruneA A = prune_operands(f, half);
    float cr[16];   // c of the hypothesis each accumulator register holds in this lane
#pragma unroll
    for (int r = 0; r < 16; r++) cr[r] = __shfl(c, half ? prune_row(r, 1) : prune_row(r, 0), 64);

    const float *r1 = rk + (size_t)b * 4 * kp_pad, *r2 = r1 + kp_pad, *r3 = r2 + kp_pad, *r4 = r3 + kp_pad;
    // X and the limits live in scalar registers (every index below is a constant after unrolling): a v_cmp mask and its
    // s_bcnt1 are scalar already, and this compiler has no builtin that writes a scalar into one lane, so a lane-held X would
    // cost a select per register and tile; counters in LDS would cost 32 ds_add per tile from one lane and a read-back at
    // every look.  The price: 64 values for about 100 registers -- the compiler parks 59 of them in vector lanes (no scratch).
    int X[kPruneHyps], L[kPruneHyps];
#pragma unroll
    for (int i = 0; i < kPruneHyps; i++) {
        X[i] = 0;
        L[i] = __builtin_amdgcn_readlane(live0 ? lim : -1, i);   // -1: nothing to prove about it
    }
    const int end = m;
    for (int base = n0; base < end; base += kPruneStep * kPruneTile) {
        float x1[kPruneStep], y1[kPruneStep], x2[kPruneStep], y2[kPruneStep];
#pragma unroll
        for (int t = 0; t < kPruneStep; t++) {
            const int j = min(base + t * kPruneTile + col, m - 1);   // lanes beyond m read a real match and are masked
            x1[t] = r1[j];
            y1[t] = r2[j];
            x2[t] = r3[j];
            y2[t] = r4[j];
        }
#pragma unroll
        for (int t = 0; t < kPruneStep; t++) {
            v16f n, a0;
            prune_tile_rows(A, half, x1[t], y1[t], x2[t], y2[t], n, a0);
            const unsigned long long valid = __ballot(base + t * kPruneTile + col < end);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                // pc_miss (ransac_prune_cert.h) as a lane mask: |n| > fma(s+, |a0|, c), ordered
                const unsigned long long miss =
                    __builtin_amdgcn_fcmpf(fabsf(n[r]), fmaf(splus, fabsf(a0[r]), cr[r]), kPruneOGT) & valid;
                X[prune_row(r, 0)] += __popc((uint32_t)miss);
                X[prune_row(r, 1)] += __popc((uint32_t)(miss >> 32));
            }
        }
        // the stop rules, on the scalar unit: the largest X among the hypotheses still alive (-1: none is)
        int top = -1;
#pragma unroll
        for (int i = 0; i < kPruneHyps; i++) top = max(top, X[i] <= L[i] ? X[i] : -1);
        const int seen = min(base + kPruneStep * kPruneTile, end) - n0;
        if (top < 0 || 2 * top < seen) break;
    }
    int xv = 0;   // lane l: X of hypothesis l & 31
#pragma unroll
    for (int i = 0; i < kPruneHyps; i++) xv = col == i ? X[i] : xv;
    if (!half && h < hyp) {
        if (live0 && xv > lim) pot0[hi] = -behind - 1;
        if (x_out) x_out[hi] = xv;
    }
}
#endif

#ifdef VSLAM_EXPERIMENTS
// (experiments build only) one tile by itself: n and a0 of 32 hypotheses (F: 32 x 9) and 32 matches (xy: x1, y1, x2, y2 as four
// arrays of 32), written as [hypothesis][match] through prune_row -- what the layout test compares with a scalar loop.
__global__ __launch_bounds__(64) void ransac_prune_tile_kernel(const float *__restrict__ F, const float *__restrict__ xy,
                                                               float *__restrict__ n_out, float *__restrict__ a0_out) {
    const int lane = threadIdx.x, col = lane & 31;
    const bool half = lane >= 32;
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = F[col * 9 + k];
    const PruneA A = prune_operands(f, half);
    v16f n, a0;
    prune_tile(A, half, xy[col], xy[32 + col], xy[64 + col], xy[96 + col], n, a0);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = half ? prune_row(r, 1) : prune_row(r, 0);   // the match; the lane's column is the hypothesis
        n_out[col * 32 + row] = n[r];
        a0_out[col * 32 + row] = a0[r];
    }
}
#endif

}  // namespace

int vs_launch_ransac_prune(vslam_ctx *ctx, const float *rk, int kp_pad, const int32_t *m, int min_m, int kp_stride, int hyp,
                           float threshold, const float *hypF, const float *cmax, const int32_t *cbound, int32_t *pot0, int batch,
                           int n_head) {
    // A/B timing and the identity test (read at every call: a test switches it within a process)
    if (VS_EXPERIMENT_ENV("VSLAM_RANSAC_NO_PRUNE") != nullptr) return VSLAM_OK;
    int gate = 1;
    if (const char *e = VS_EXPERIMENT_ENV("VSLAM_RANSAC_PRUNE_GATE")) gate = atoi(e);   // the tests walk every pair with 0
#ifdef VSLAM_EXPERIMENTS
    int32_t *x_out = nullptr;
    if (int rc = vs_arena_get(ctx, "ransac.prune_x", sizeof(int32_t) * (size_t)batch * hyp, (void **)&x_out)) return rc;
    VS_HIP(ctx, hipMemsetAsync(x_out, 0, sizeof(int32_t) * (size_t)batch * hyp, ctx->stream));
#endif
    VsProfScope ps(ctx, "ransac_prune_kernel");
    dim3 grid(vs_div_up(hyp, kPruneWaves * kPruneHyps), batch);
#ifdef VSLAM_EXPERIMENTS
    if (vs_prune_rows_form())   // the identity test and A/B timing (read at every call)
        ransac_prune_rows_kernel<<<grid, 64 * kPruneWaves, 0, ctx->stream>>>(rk, kp_pad, m, min_m, kp_stride, hyp, threshold, pc_splus(threshold), hypF,
                                                                             cmax, cbound, pot0, n_head, gate, x_out);
    else
        ransac_prune_mfma_kernel<<<grid, 64 * kPruneWaves, 0, ctx->stream>>>(rk, kp_pad, m, min_m, kp_stride, hyp, threshold, pc_splus(threshold), hypF,
                                                                             cmax, cbound, pot0, n_head, gate, x_out);
#else
    ransac_prune_mfma_kernel<<<grid, 64 * kPruneWaves, 0, ctx->stream>>>(rk, kp_pad, m, min_m, kp_stride, hyp, threshold, pc_splus(threshold), hypF, cmax,
                                                                         cbound, pot0, n_head, gate);
#endif
    return VSLAM_OK;
}

#ifdef VSLAM_EXPERIMENTS
extern "C" {
// (experiments build only) X[h] of the last vs_launch_ransac_prune of this context: the certified misses per hypothesis behind
// the head, batch x hyp int32 (zero for a hypothesis no wave walked), copied to d_out in stream order
int vslam_debug_ransac_prune_x(vslam_ctx *ctx, int32_t *d_out, int batch, int hyp) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_out && batch > 0 && hyp > 0 && vs_ptr_bits(d_out) % 4 == 0, VSLAM_ERR_INVALID);
    const size_t bytes = sizeof(int32_t) * (size_t)batch * hyp;
    const auto it = ctx->arena.find("ransac.prune_x");
    VS_REQUIRE(ctx, it != ctx->arena.end() && it->second.bytes >= bytes, VSLAM_ERR_INVALID);
    VS_HIP(ctx, hipMemcpyAsync(d_out, it->second.ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return VSLAM_OK;
}
// (experiments build only) of the last RANSAC scoring of this context: pot0 as ransac_screen_kernel's two paths left it
// (batch x hyp int32, before the prune kernel) and the routing word per pair (1 = the head on the certificate, 0 = on the
// cheap evaluation, -1 = fewer than min_m matches), copied in stream order
int vslam_debug_ransac_head(vslam_ctx *ctx, int32_t *d_pot0, int32_t *d_route, int batch, int hyp) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_pot0 && d_route && batch > 0 && hyp > 0 && vs_ptr_bits(d_pot0, d_route) % 4 == 0, VSLAM_ERR_INVALID);
    const size_t bytes = sizeof(int32_t) * (size_t)batch * hyp;
    const auto ip = ctx->arena.find("ransac.head_pot0"), ir = ctx->arena.find("ransac.head_route");
    VS_REQUIRE(ctx, ip != ctx->arena.end() && ip->second.bytes >= bytes, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, ir != ctx->arena.end() && ir->second.bytes >= sizeof(int32_t) * (size_t)batch, VSLAM_ERR_INVALID);
    VS_HIP(ctx, hipMemcpyAsync(d_pot0, ip->second.ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    VS_HIP(ctx, hipMemcpyAsync(d_route, ir->second.ptr, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToDevice, ctx->stream));
    return VSLAM_OK;
}
// (experiments build only) one 32 x 32 tile through the kernel's own operand and accumulator mapping
int vslam_debug_ransac_prune_tile(vslam_ctx *ctx, const float *d_F, const float *d_xy, float *d_n, float *d_a0) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_F && d_xy && d_n && d_a0 && vs_ptr_bits(d_F, d_xy, d_n, d_a0) % 4 == 0, VSLAM_ERR_INVALID);
    ransac_prune_tile_kernel<<<1, 64, 0, ctx->stream>>>(d_F, d_xy, d_n, d_a0);
    return VSLAM_OK;
}
}  // extern "C"
#endif
