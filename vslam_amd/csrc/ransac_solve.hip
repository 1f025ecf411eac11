// RANSAC fundamental-matrix loop, stage 2 of 4: one hypothesis F per set of 8 matches.
//
// Replaces RansacFilter::compute_fundamental (the reference's src/RansacFilter.cpp:69-103):
//   design matrix :75-90, SVDecomp :94, V_t.row(8) :95,
//   SVDecomp of F0 :98, D[2] = 0 :99, U diag(D) V_t :101  -> ransac_solve_kernel<>  (one lane per hypothesis)
//   the same, stopped behind the first SVD + the rest      -> ransac_solve_kernel<true, .> + ransac_close_kernel
//                                                             (experiments build only; measured slower)
//   opt-in approximate solver (VSLAM_OPT_RANSAC_SOLVER 1) -> ransac_condition_kernel + ransac_solve_gram_kernel
//
// Numerics: the default solver is bit-exact with the reference: every hypothesis is the F that OpenCV's Jacobi SVD gives
// on the CPU (ransac_svd.h states how).  The 8 x 9 instance below keeps the matrix in registers; every operation on every
// value is the one the plain restatement in ransac_svd.h would perform, in the same order.  The Gram solver is NOT
// bit-exact and never the default; its section says what it promises instead.
#include "ransac_svd.h"

namespace {
using namespace vs_ransac;

// ------------------------------------------------------------------------------------------
// The 8 x 9 instance as ransac_solve_kernel runs it: the lane's whole matrix in registers during the sweeps.
// ------------------------------------------------------------------------------------------
// 72 floats per lane in LDS held the kernel at 8 waves per CU (2 per SIMD); it is bound by dependent f64 chains on the
// vector pipe, where more waves pay (2 -> 3 per SIMD: 0.96 -> 0.88 ms with three of the rows in registers).  With all
// eight rows in registers (72 VGPRs; every (i, j) step written out, the row indices compile-time) the sweeps touch no
// LDS at all, 128 VGPRs suffice and 4 waves fit.  The part after the sweeps sorts the rows in place, between compile-time
// positions, so it needs no LDS either; the kernel's LDS is the 3 x 3 solve's (18 floats per lane).  Every operation on
// every value is the one jacobi_svd_lanes<9, 8, 9, false> (the plain restatement in ransac_svd.h) would perform, in the
// same order.
// Where the kernel's values live is decided as much by what surrounds the arithmetic as by the arithmetic: c and s of
// jacobi_cs_full coming back through pointers, and the rare closing path as the other side of an if / else, each put
// values of the common path into scratch memory (363 spilled registers, one row element going through memory on every
// rotation).  Both are written below so that nothing of the common path is live across a call.
constexpr int kSolveLdsFloats = 18;

// c, s of a rotation for operands outside the range the short sqrt / division sequences cover (see jacobi_svd_lanes).
// Deliberately a real call: it is reached by a wave-wide vote that practically never passes, and 28 inlined copies of the
// IEEE sqrt and division expansions would double the size of the sweep loop.  (c, s) come back in registers: returned
// through pointers they are two stack objects, and the sweep loop addresses scratch memory around every call site.
__device__ __attribute__((noinline)) float2 jacobi_cs_full(double p, double beta, double g2) {
    float c, s;
    const double gamma = sqrt(g2);   // pinned hypot
    if (beta < 0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)sqrt(delta / gamma);
        c = (float)(p / (gamma * (double)s * 2));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2));
        s = (float)(p / (gamma * (double)c * 2));
    }
    return make_float2(c, s);
}

// one (i, j) step on two rows held in registers.  Returns whether this lane rotated (the rows are then the rotated ones).
// TWOQ (experiments build, VSLAM_RANSAC_SOLVE_QUOTIENT=two): the first quotient's operands selected between the two branches'
// own expressions, the form of round 11, for the bit comparison.
template <bool TWOQ>
__device__ __forceinline__ bool jacobi_pair_9(float (&ai)[9], float (&aj)[9]) {
    double a = 0, p = 0, b = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double di = (double)ai[k], dj = (double)aj[k];
        p = __builtin_fma(di, dj, p);
        a = __builtin_fma(di, di, a);   // W[i]
        b = __builtin_fma(dj, dj, b);   // W[j]
    }
    if (jacobi_converged(p, a, b)) return false;
    p *= 2;
    const double beta = a - b;
    const double g2 = p * p + beta * beta;
    float c, s;
    // see jacobi_svd_lanes for the range argument
    const bool safe = g2 > 0x1p-400 && g2 < 0x1p400 && fabs(p) > 0x1p-300;
    if (!__any(!safe)) {
        // One instruction stream for both signs of beta (lanes of a wave differ in it, so as two branches both would run):
        // the first of (c, s) is a square root of a quotient, the second a quotient by it; which is which is
        // selected.  The first quotient is one expression for both signs, with the bits each branch would give:
        //   beta < 0:   ((gamma - beta) * 0.5) / gamma.  gamma - beta is the IEEE operation gamma + |beta| (x - y = x + (-y), and
        //               -beta = |beta| here), so the numerator is the expression below as written.
        //   beta >= 0:  (gamma + beta) / (gamma * 2), with t = gamma + beta = gamma + |beta| (beta = -0 included: gamma > 0, and
        //               gamma + 0 = gamma under either sign).  t * 0.5 and gamma * 2 are exact: the vote confines g2 to
        //               (2^-400, 2^400), so gamma lies in [2^-200, 2^200] and t in [gamma, 2 gamma + ulp] -- no overflow, nothing
        //               subnormal.  div_inrange(t * 0.5, gamma) and div_inrange(t, gamma * 2) then run the same sequence on
        //               operands that differ by exact powers of two (v_rcp_f64 of 2 y is half that of y, every product and
        //               fma of the corrections scales with it, all far from the exponent range's ends): the same quotient
        //               bits, the rounding of t / (2 gamma) in [1/2, 1].
        // |beta| is a source modifier of the add: this spares a subtraction, a multiplication and two f64 selects (four
        // v_cndmask_b32) per visit, two of them on the dependent chain.  jacobi_cs_full above stays the reference sequence.
        const double gamma = sqrt_inrange(g2);   // pinned hypot
        const bool neg = beta < 0;
        const double num = TWOQ ? (neg ? (gamma - beta) * 0.5 : gamma + beta) : (gamma + fabs(beta)) * 0.5;
        const double den = TWOQ ? (neg ? gamma : gamma * 2) : gamma;
        const float first = (float)sqrt_inrange(div_inrange(num, den));
        const float second = (float)div_inrange(p, gamma * (double)first * 2);
        s = neg ? first : second;
        c = neg ? second : first;
    } else {
        const float2 cs = jacobi_cs_full(p, beta, g2);
        c = cs.x;
        s = cs.y;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const float t0 = c * ai[k] + s * aj[k];
        const float t1 = (-s) * ai[k] + c * aj[k];
        ai[k] = t0;
        aj[k] = t1;
    }
    return true;
}

// One sweep over all pairs in OpenCV's order, all 28 steps written out so that the row indices are compile-time.
// (Round 3 tried the re-rolled form the 60 % "waiting for an instruction" of this kernel seemed to ask for — the seven
// steps of one row written out, the rows themselves shifted one position after each row's turn, 72 register moves, loop
// 13 KB instead of 40 KB: bit-identical, and 0.92 ms instead of 0.75.  The waits are the dependent f64 chains of a
// rotation's parameters — two square roots and two divisions in sequence, about a hundred dependent instructions with
// four waves per SIMD to hide them — not instruction fetch.)
template <bool TWOQ>
__device__ __forceinline__ bool jacobi_sweep_8x9_regs(float (&R)[8][9]) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = i + 1; j < 8; j++) changed |= jacobi_pair_9<TWOQ>(R[i], R[j]);
    return changed;
}

// The rare form of the part after the sweeps: jacobi_finish on a private copy of the rows (see jacobi_null_row_8x9).  A real
// call, like jacobi_cs_full: its loops over run-time rows stay out of the kernel's register allocation.  The result comes
// back in registers, so the caller's f0 is no stack object.
struct NullRow {
    float f[9];
};
__device__ __attribute__((noinline)) NullRow jacobi_null_row_private(float *rows) {
    NullRow out;
    float w8[8];
    jacobi_finish<9, 8, 9, false, 1>(rows, nullptr, w8, out.f);
    return out;
}

// After the sweeps: V_t.row(8) of SVDecomp(A 8x9, FULL_UV) = the row beyond the rank, orthogonalised against the sorted,
// normalised rows (jacobi_finish<9, 8, 9, false, .> with only extra_row kept).  If a row's norm does not exceed FLT_MIN
// OpenCV regenerates that row from its RNG stream first (degenerate samples): a wave with a lane that may be in that
// case goes through jacobi_finish itself on a private copy.  Otherwise a row's normalisation factor is a function of that
// row alone, so the rows are normalised where they are and then sorted: the selection sort's swap of rows i and j becomes
// a conditional swap of row i with each row behind it (28 candidates, 18 selects each, once, and only in a wave where the
// sort has anything to do), after which the orthogonalisation reads registers in static order.
__device__ __forceinline__ void jacobi_null_row_8x9(float (&R)[8][9], float *f0) {
    constexpr int M = 9, N = 8;
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    // A row is tiny when its norm sqrt(sum of squares) <= FLT_MIN = 2^-126.  A row with an element of magnitude 2^-120 or
    // more has a sum of squares of at least 2^-240 and is not tiny, so the vote below passes whenever a row is tiny.  It
    // may pass for rows that are not: jacobi_finish is the general procedure and gives those the same bits.  Voting on the
    // elements, before the norms exist, keeps the norms from being live across the call.
    float small = 0x1p-120f;
#pragma unroll
    for (int i = 0; i < N; i++) {
        float big = fabsf(R[i][0]);
#pragma unroll
        for (int k = 1; k < M; k++) big = fmaxf(big, fabsf(R[i][k]));
        small = fminf(small, big);
    }
    int usual = 1;
    if (__any(small < 0x1p-120f)) {
        float rows[N * M];
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int k = 0; k < M; k++) rows[i * M + k] = R[i][k];
        const NullRow nr = jacobi_null_row_private(rows);
#pragma unroll
        for (int k = 0; k < M; k++) f0[k] = nr.f[k];
        // Not `return`: as the two sides of an if / else the paths are laid out one behind the other, every row counts as
        // live through the call, and the usual path spills too.  As two ifs in sequence, the flag opaque to the compiler
        // and the rows read back (they are never used), nothing is live across the call.
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int k = 0; k < M; k++) R[i][k] = rows[i * M + k];
        usual = 0;
        asm volatile("" : "+s"(usual));
    }
    if (!usual) return;
    double W[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd = __builtin_fma((double)R[i][k], (double)R[i][k], sd);
        W[i] = sqrt(sd);
    }
    // normalise (row *= (float)(1 / W), W = the row's norm)
#pragma unroll
    for (int i = 0; i < N; i++) {
        const float s = (float)(1 / W[i]);
#pragma unroll
        for (int k = 0; k < M; k++) R[i][k] = R[i][k] * s;
    }
    // The descending selection sort.  A rotation leaves the larger norm in the row of the lower index, so the sweeps
    // nearly always end with the rows in order already: the sort moves something exactly when W[i] < W[k] for some i < k
    // (its first such i is where it first swaps), and only a wave with such a lane goes through it.  There the rows travel
    // with W as conditional swaps between compile-time positions.
    bool unsorted = false;
#pragma unroll
    for (int i = 0; i < N - 1; i++)
#pragma unroll
        for (int k = i + 1; k < N; k++) unsorted = unsorted || W[i] < W[k];
    if (__any(unsorted)) {
#pragma unroll
        for (int i = 0; i < N - 1; i++) {
            int j = i;
            double wj = W[i];
#pragma unroll
            for (int k = i + 1; k < N; k++)
                if (wj < W[k]) {
                    j = k;
                    wj = W[k];
                }
#pragma unroll
            for (int jj = i + 1; jj < N; jj++) {
                const bool hit = jj == j;
                W[jj] = hit ? W[i] : W[jj];
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float x = R[i][k], y = R[jj][k];
                    R[i][k] = hit ? y : x;
                    R[jj][k] = hit ? x : y;
                }
            }
            W[i] = wj;
        }
    }
    // the row beyond the rank: jacobi_finish's N1 > N block, rows visited in sorted order
    uint64_t rng = 0x12345678ull;
    float v[M];
    double sd = 0;
    for (int ii = 0; ii < 100 && sd <= minval; ii++) {
        const float val0 = (float)(1. / M);
#pragma unroll
        for (int k = 0; k < M; k++) v[k] = (cvrng_next(rng) & 256) != 0 ? val0 : -val0;
        for (int iter = 0; iter < 2; iter++) {
#pragma unroll
            for (int jj = 0; jj < N; jj++) {
                float vj[M];
                sd = 0;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    vj[k] = R[jj][k];
                    sd += (double)(v[k] * vj[k]);   // float product, double running sum
                }
                float asum = 0;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float t = (float)((double)v[k] - sd * (double)vj[k]);
                    v[k] = t;
                    asum += fabsf(t);
                }
                asum = asum > eps * 100 ? 1 / asum : 0;
#pragma unroll
                for (int k = 0; k < M; k++) v[k] = v[k] * asum;
            }
        }
        sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd = __builtin_fma((double)v[k], (double)v[k], sd);
        sd = sqrt(sd);
    }
    const float s = (float)(sd > minval ? 1 / sd : 0.);
#pragma unroll
    for (int k = 0; k < M; k++) f0[k] = v[k] * s;
}

// The part of compute_fundamental behind the first SVD (src/RansacFilter.cpp:98-101): the 3 x 3 SVD of F0 (working rows =
// its columns), D[2] = 0, F = U diag(D) Vt.  sA / sV: this wave's 9 + 9 float columns in LDS; `tid` = the lane.
__device__ __forceinline__ void fundamental_rank2(const float (&f0)[9], float *sA, float *sV, int tid, float (&F)[9]) {
    {
        constexpr int M = 3;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) VS_A(i, k) = f0[3 * k + i];
    }
    float d3[3];
    jacobi_svd_lanes<3, 3, 3, true>(sA, sV, tid, d3, nullptr);
    d3[2] = 0.f;   // :99

    float U[9], Vt[9];
    {
        constexpr int M = 3, N = 3;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                U[r * 3 + c] = VS_A(c, r);   // u = transpose(temp_u)
                Vt[r * 3 + c] = VS_V(r, c);
            }
    }
    // temp_F = U * diag(D) * V_t (:101) through OpenCV's 3x3 float fast path (a0*b0 + a1*b1 + a2*b2)
    const float Dg[9] = {d3[0], 0.f, 0.f, 0.f, d3[1], 0.f, 0.f, 0.f, d3[2]};
    float UD[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            UD[i * 3 + j] = U[i * 3 + 0] * Dg[0 * 3 + j] + U[i * 3 + 1] * Dg[1 * 3 + j] + U[i * 3 + 2] * Dg[2 * 3 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            F[i * 3 + j] = UD[i * 3 + 0] * Vt[0 * 3 + j] + UD[i * 3 + 1] * Vt[1 * 3 + j] + UD[i * 3 + 2] * Vt[2 * 3 + j];
}

// One lane per hypothesis, one wave per workgroup.  grid = (ceil(hyp / 64), batch).
// SPLIT (round 5, VSLAM_RANSAC_SOLVE_SPLIT): the kernel stops behind the first SVD and leaves F0 = V_t.row(8) in hypF;
// ransac_close_kernel turns it into F in place.  WPE: waves per SIMD the register budget is cut for.
template <bool SPLIT, int WPE, bool TWOQ = false>
__global__ __launch_bounds__(kSolveThreads) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void ransac_solve_kernel(
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, int min_m, const int32_t *__restrict__ sets, int kp_stride, int hyp,
    float *__restrict__ hypF) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int h = blockIdx.x * kSolveThreads + tid;
    if (m_arr[b] < min_m) return;   // uniform per workgroup (8 unless RansacFilter::min_items is smaller)

    __shared__ float sA[kSolveLdsFloats * kSolveThreads];   // fundamental_rank2's 9 + 9 columns per lane

    const bool live = h < hyp;
    const int hc = live ? h : hyp - 1;   // idle lanes redo the last hypothesis; no divergence in barriers
    const float2 *P1 = reinterpret_cast<const float2 *>(xy1) + (size_t)b * kp_stride;
    const float2 *P2 = reinterpret_cast<const float2 *>(xy2) + (size_t)b * kp_stride;
    const int2 *PR = reinterpret_cast<const int2 *>(pairs) + (size_t)b * kp_stride;
    const int32_t *S = sets + ((size_t)b * hyp + hc) * VSLAM_SET_SIZE;

    float R[8][9];
#pragma unroll
    for (int r = 0; r < 8; r++) {   // design matrix, RansacFilter.cpp:75-90
        const int2 pr = PR[S[r]];
        const float2 a = P1[pr.x], c = P2[pr.y];
        const float u1 = a.x, v1 = a.y, u2 = c.x, v2 = c.y;
        R[r][0] = u2 * u1;
        R[r][1] = u2 * v1;
        R[r][2] = u2;
        R[r][3] = v2 * u1;
        R[r][4] = v2 * v1;
        R[r][5] = v2;
        R[r][6] = u1;
        R[r][7] = v1;
        R[r][8] = 1.f;
    }

    float f0[9];
    {   // SVDecomp(A 8x9), :94; f0 = V_t.row(8), :95
        constexpr int max_iter = 30;
        for (int iter = 0; iter < max_iter; iter++)
            if (!jacobi_sweep_8x9_regs<TWOQ>(R)) break;
        jacobi_null_row_8x9(R, f0);
    }

    float F[9];
    if (SPLIT) {
#pragma unroll
        for (int k = 0; k < 9; k++) F[k] = f0[k];
    } else {
        fundamental_rank2(f0, sA, sA + 9 * kSolveThreads, tid, F);   // second SVD on the 3x3 (:98) and F = U diag Vt (:101)
    }
    if (live) {
        float *o = hypF + ((size_t)b * hyp + h) * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = F[k];
    }
}

#ifdef VSLAM_EXPERIMENTS
// The closing part of the split form (experiments build; measured slower than the one-kernel solve): four waves per
// workgroup, a lane per hypothesis, F0 in, F out, in place.
constexpr int kCloseThreads = 256;
__global__ __launch_bounds__(kCloseThreads) void ransac_close_kernel(const int32_t *__restrict__ m_arr, int min_m, int hyp,
                                                                     float *__restrict__ hypF) {
    const int b = blockIdx.y;
    if (m_arr[b] < min_m) return;
    __shared__ float s[kCloseThreads / 64][18 * kSolveThreads];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = blockIdx.x * kCloseThreads + threadIdx.x;
    const bool live = h < hyp;
    float *o = hypF + ((size_t)b * hyp + (live ? h : 0)) * 9;
    float f0[9], F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f0[k] = live ? o[k] : (k % 4 == 0 ? 1.f : 0.f);   // lanes past the end work on the identity: no read of a slot a live lane rewrites
    fundamental_rank2(f0, s[wave], s[wave] + 9 * kSolveThreads, lane, F);
    if (live) {
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = F[k];
    }
}
#endif   // VSLAM_EXPERIMENTS

// ------------------------------------------------------------------------------------------
// compute_fundamental, opt-in approximate form: the 8-point system as a dense contraction on the matrix cores
// (BASELINE.json configs[4]; VSLAM_OPT_RANSAC_SOLVER = 1).  NOT bit-exact with the reference and never the default:
// the parity bar pins the default solver to OpenCV's sequential Jacobi sweeps (ransac_solve_kernel above).
//   1. Hartley-style conditioning with ONE similarity per frame of the pair (centroid and mean distance of the
//      pair's matched points; ransac_condition_kernel), so the 9x9 normal matrix is formed from O(1) numbers;
//   2. G = A^T A (9 x 9, A the 8 x 9 design matrix) on v_mfma_f32_16x16x4_f32: the A operand and the B operand of the
//      instruction are the same register (lane l holds design[row 4 step + (l >> 4)][column l & 15]), two
//      instructions per hypothesis, results through LDS to the lane that owns the hypothesis;
//   3. the null vector of A = the eigenvector of G's smallest eigenvalue, by inverse iteration on G + mu I
//      (Cholesky + 4 solves in f64, one lane per hypothesis);
//   4. back to pixel coordinates (F0 = T2^T F^ T1), unit Frobenius norm like V_t.row(8), then the SAME rank-2 step as
//      the exact kernel (jacobi_svd_lanes<3,3,3,true>, RansacFilter.cpp:98-101).
// F agrees with the exact solver up to sign and rounding (tests/test_gpu_ransac.py states the tolerance and measures the
// inlier-mask agreement); on degenerate samples (rank < 8) the two pick different vectors of the null space.
typedef float v4f __attribute__((ext_vector_type(4)));

// the pair's two similarities: cond[b] = (cx1, cy1, s1, cx2, cy2, s2); one workgroup per pair
__global__ __launch_bounds__(256) void ransac_condition_kernel(const float *__restrict__ xy1, const float *__restrict__ xy2,
                                                               const int32_t *__restrict__ pairs, const int32_t *__restrict__ m_arr,
                                                               int kp_stride, float *__restrict__ cond) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = min(m_arr[b], kp_stride);
    if (m < VSLAM_SET_SIZE) return;
    const float2 *P1 = reinterpret_cast<const float2 *>(xy1) + (size_t)b * kp_stride;
    const float2 *P2 = reinterpret_cast<const float2 *>(xy2) + (size_t)b * kp_stride;
    const int2 *PR = reinterpret_cast<const int2 *>(pairs) + (size_t)b * kp_stride;
    __shared__ double red[4][4];
    __shared__ float cen[4];
    auto block_sum4 = [&](double v0, double v1, double v2, double v3, double out[4]) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            v0 += __shfl_xor(v0, off, 64); v1 += __shfl_xor(v1, off, 64);
            v2 += __shfl_xor(v2, off, 64); v3 += __shfl_xor(v3, off, 64);
        }
        __syncthreads();
        if ((tid & 63) == 0) {
            red[tid >> 6][0] = v0; red[tid >> 6][1] = v1; red[tid >> 6][2] = v2; red[tid >> 6][3] = v3;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) out[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    };
    double s[4] = {0, 0, 0, 0}, tot[4];
    for (int i = tid; i < m; i += 256) {
        const int2 pr = PR[i];
        const float2 a = P1[pr.x], c = P2[pr.y];
        s[0] += a.x; s[1] += a.y; s[2] += c.x; s[3] += c.y;
    }
    block_sum4(s[0], s[1], s[2], s[3], tot);
    if (tid < 4) cen[tid] = (float)(tot[tid] / m);
    __syncthreads();
    const float cx1 = cen[0], cy1 = cen[1], cx2 = cen[2], cy2 = cen[3];
    double d1 = 0, d2 = 0;
    for (int i = tid; i < m; i += 256) {
        const int2 pr = PR[i];
        const float2 a = P1[pr.x], c = P2[pr.y];
        d1 += sqrtf((a.x - cx1) * (a.x - cx1) + (a.y - cy1) * (a.y - cy1));
        d2 += sqrtf((c.x - cx2) * (c.x - cx2) + (c.y - cy2) * (c.y - cy2));
    }
    block_sum4(d1, d2, 0, 0, tot);
    if (tid == 0) {
        float *o = cond + (size_t)b * 6;
        o[0] = cx1; o[1] = cy1; o[2] = tot[0] > 0 ? (float)(1.4142135623730951 * m / tot[0]) : 1.f;
        o[3] = cx2; o[4] = cy2; o[5] = tot[1] > 0 ? (float)(1.4142135623730951 * m / tot[1]) : 1.f;
    }
}

__global__ __launch_bounds__(kSolveThreads) void ransac_solve_gram_kernel(
    const float *__restrict__ xy1, const float *__restrict__ xy2, const int32_t *__restrict__ pairs,
    const int32_t *__restrict__ m_arr, const int32_t *__restrict__ sets, const float *__restrict__ cond, int kp_stride, int hyp,
    float *__restrict__ hypF) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int h = blockIdx.x * kSolveThreads + tid;
    const int m = min(m_arr[b], kp_stride);
    if (m < VSLAM_SET_SIZE) return;   // uniform per workgroup

    __shared__ float4 s_pts[kSolveThreads * 8];          // conditioned (u1, v1, u2, v2) of the 8 points of each hypothesis
    __shared__ float s_G[kSolveThreads * 45];            // lower triangle of G per hypothesis; the 3x3 solver's scratch afterwards
    const float2 *P1 = reinterpret_cast<const float2 *>(xy1) + (size_t)b * kp_stride;
    const float2 *P2 = reinterpret_cast<const float2 *>(xy2) + (size_t)b * kp_stride;
    const int2 *PR = reinterpret_cast<const int2 *>(pairs) + (size_t)b * kp_stride;
    const float cx1 = cond[b * 6 + 0], cy1 = cond[b * 6 + 1], sc1 = cond[b * 6 + 2];
    const float cx2 = cond[b * 6 + 3], cy2 = cond[b * 6 + 4], sc2 = cond[b * 6 + 5];

    // ---- conditioned sample points of this lane's hypothesis
    const bool live = h < hyp;
    const int hc = live ? h : hyp - 1;
    const int32_t *S = sets + ((size_t)b * hyp + hc) * VSLAM_SET_SIZE;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int2 pr = PR[S[r]];
        const float2 a = P1[pr.x], c = P2[pr.y];
        s_pts[tid * 8 + r] = make_float4((a.x - cx1) * sc1, (a.y - cy1) * sc1, (c.x - cx2) * sc2, (c.y - cy2) * sc2);
    }
    __syncthreads();

    // ---- 2. G = A^T A on the matrix cores, one hypothesis per pair of instructions
    const int col = tid & 15, grp = tid >> 4;
    for (int hh = 0; hh < kSolveThreads; hh++) {
        v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int step = 0; step < 2; step++) {
            const float4 q = s_pts[hh * 8 + 4 * step + grp];   // (u1, v1, u2, v2) of design row 4 step + grp
            // column `col` of the row [u2u1, u2v1, u2, v2u1, v2v1, v2, u1, v1, 1] (RansacFilter.cpp:81-89); 0 beyond 8
            const float left = col < 3 ? q.z : (col < 6 ? q.w : (col < 9 ? 1.f : 0.f));
            const int c3 = col - 3 * (col / 3);
            const float right = c3 == 0 ? q.x : (c3 == 1 ? q.y : 1.f);
            const float e = left * right;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(e, e, acc, 0, 0, 0);   // D[i][j] += sum_k design[k][i] design[k][j]
        }
        // D: column = lane & 15, row = 4 (lane >> 4) + register; G is symmetric, the lower triangle is kept
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int row = 4 * grp + v;
            if (row < 9 && col <= row) s_G[hh * 45 + row * (row + 1) / 2 + col] = acc[v];
        }
    }
    __syncthreads();

    // ---- 3. smallest eigenvector of G by inverse iteration on G + mu I (f64, this lane's hypothesis)
    double L[45];   // lower triangle, row-major: L[i(i+1)/2 + j]
    double tr = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) tr += (double)s_G[tid * 45 + i * (i + 1) / 2 + i];
    const double mu = tr * 1e-7 + 1e-30;
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double v = (double)s_G[tid * 45 + i * (i + 1) / 2 + j] + (i == j ? mu : 0.0);
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = i == j ? sqrt(v) : v / L[j * (j + 1) / 2 + j];
        }
    double x[9];
#pragma unroll
    for (int i = 0; i < 9; i++) x[i] = (i & 1) ? -1.0 / 3.0 : 1.0 / 3.0;
#pragma unroll 1
    for (int it = 0; it < 4; it++) {
#pragma unroll
        for (int i = 0; i < 9; i++) {   // L y = x
            double v = x[i];
#pragma unroll
            for (int k = 0; k < i; k++) v -= L[i * (i + 1) / 2 + k] * x[k];
            x[i] = v / L[i * (i + 1) / 2 + i];
        }
#pragma unroll
        for (int i = 8; i >= 0; i--) {   // L^T z = y
            double v = x[i];
#pragma unroll
            for (int k = i + 1; k < 9; k++) v -= L[k * (k + 1) / 2 + i] * x[k];
            x[i] = v / L[i * (i + 1) / 2 + i];
        }
        double nn = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) nn += x[i] * x[i];
        const double inv = 1.0 / sqrt(nn);
#pragma unroll
        for (int i = 0; i < 9; i++) x[i] *= inv;
    }

    // ---- 4. F0 = T2^T F^ T1 with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], then unit norm
    double f0[9];
    {
        const double s1 = sc1, s2 = sc2, tx1 = -(double)sc1 * cx1, ty1 = -(double)sc1 * cy1, tx2 = -(double)sc2 * cx2, ty2 = -(double)sc2 * cy2;
        double Mx[9];   // F^ T1
#pragma unroll
        for (int r = 0; r < 3; r++) {
            Mx[r * 3 + 0] = x[r * 3 + 0] * s1;
            Mx[r * 3 + 1] = x[r * 3 + 1] * s1;
            Mx[r * 3 + 2] = x[r * 3 + 0] * tx1 + x[r * 3 + 1] * ty1 + x[r * 3 + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {   // T2^T (F^ T1)
            f0[0 * 3 + c] = s2 * Mx[0 * 3 + c];
            f0[1 * 3 + c] = s2 * Mx[1 * 3 + c];
            f0[2 * 3 + c] = tx2 * Mx[0 * 3 + c] + ty2 * Mx[1 * 3 + c] + Mx[2 * 3 + c];
        }
        double nn = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) nn += f0[i] * f0[i];
        const double inv = 1.0 / sqrt(nn);
#pragma unroll
        for (int i = 0; i < 9; i++) f0[i] *= inv;
    }
    __syncthreads();   // every lane is done with its G: the buffer becomes the 3x3 solver's scratch

    // the rank-2 step of the exact kernel (RansacFilter.cpp:98-101)
    float *sA = s_G;
    float *sV = s_G + 9 * kSolveThreads;
    {
        constexpr int M = 3;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) VS_A(i, k) = (float)f0[3 * k + i];
    }
    float d3[3];
    jacobi_svd_lanes<3, 3, 3, true>(sA, sV, tid, d3, nullptr);
    d3[2] = 0.f;
    float U[9], Vt[9];
    {
        constexpr int M = 3, N = 3;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                U[r * 3 + c] = VS_A(c, r);
                Vt[r * 3 + c] = VS_V(r, c);
            }
    }
    const float Dg[9] = {d3[0], 0.f, 0.f, 0.f, d3[1], 0.f, 0.f, 0.f, d3[2]};
    float UD[9], F[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            UD[i * 3 + j] = U[i * 3 + 0] * Dg[0 * 3 + j] + U[i * 3 + 1] * Dg[1 * 3 + j] + U[i * 3 + 2] * Dg[2 * 3 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            F[i * 3 + j] = UD[i * 3 + 0] * Vt[0 * 3 + j] + UD[i * 3 + 1] * Vt[1 * 3 + j] + UD[i * 3 + 2] * Vt[2 * 3 + j];
    if (live) {
        float *o = hypF + ((size_t)b * hyp + h) * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = F[k];
    }
}
#undef VS_A
#undef VS_V

}  // namespace

int vs_launch_ransac_solve(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs,
                           const int32_t *m, const int32_t *sets, int batch, int kp_stride, int hyp,
                           float *hypF) {
    VS_REQUIRE(ctx, xy1 && xy2 && pairs && m && sets && hypF, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && kp_stride > 0 && hyp > 0, VSLAM_ERR_INVALID);
    dim3 grid(vs_div_up(hyp, kSolveThreads), batch);
    if (ctx->ransac_solver == 1) {   // opt-in, not bit-exact (VSLAM_OPT_RANSAC_SOLVER)
        float *cond = nullptr;
        int rc = vs_arena_get(ctx, "ransac.cond", sizeof(float) * 6 * (size_t)batch, (void **)&cond);
        if (rc) return rc;
        VsProfScope ps(ctx, "ransac_solve_gram_kernel");
        ransac_condition_kernel<<<batch, 256, 0, ctx->stream>>>(xy1, xy2, pairs, m, kp_stride, cond);
        ransac_solve_gram_kernel<<<grid, kSolveThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, sets, cond, kp_stride, hyp, hypF);
        VS_HIP(ctx, hipGetLastError());
        return VSLAM_OK;
    }
    // VSLAM_RANSAC_SOLVE_SPLIT: 0 one kernel (rounds 2-4); 4 / 5: sweeps + null-space row at 4 / 5 waves per SIMD, then
    // ransac_close_kernel (the 3 x 3 SVD and U diag Vt, a launch of its own at full occupancy).  Same bits either way.
    VsProfScope ps(ctx, "ransac_solve_kernel");
#ifndef VSLAM_EXPERIMENTS
    ransac_solve_kernel<false, 4><<<grid, kSolveThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, ctx->ransac_min_matches, sets, kp_stride, hyp, hypF);
#else
    const int split = ctx->solve_split;
    // VSLAM_RANSAC_SOLVE_QUOTIENT=two (read at every call: a test switches it within a process): jacobi_pair_9<true>
    const char *const q_env = VS_EXPERIMENT_ENV("VSLAM_RANSAC_SOLVE_QUOTIENT");
    if (split == 0 && q_env && q_env[0] == 't') {
        ransac_solve_kernel<false, 4, true><<<grid, kSolveThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, ctx->ransac_min_matches, sets, kp_stride, hyp, hypF);
    } else if (split == 0) {
        ransac_solve_kernel<false, 4><<<grid, kSolveThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, ctx->ransac_min_matches, sets, kp_stride, hyp, hypF);
    } else {
        if (split == 5)
            ransac_solve_kernel<true, 5><<<grid, kSolveThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, ctx->ransac_min_matches, sets, kp_stride, hyp, hypF);
        else
            ransac_solve_kernel<true, 4><<<grid, kSolveThreads, 0, ctx->stream>>>(xy1, xy2, pairs, m, ctx->ransac_min_matches, sets, kp_stride, hyp, hypF);
        ransac_close_kernel<<<dim3(vs_div_up(hyp, kCloseThreads), batch), kCloseThreads, 0, ctx->stream>>>(m, ctx->ransac_min_matches, hyp, hypF);
    }
#endif
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}
