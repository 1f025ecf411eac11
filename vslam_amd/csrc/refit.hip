// Refit of the RANSAC winner over its whole consensus set (vslam_refit_fundamental, include/vslam_amd.h): the step
// find_fundamental leaves undone (src/RansacFilter.cpp:36-67 returns the winner as fitted to its 8 sampled, un-normalised
// points; `//TODO: normalize` at :40).  One workgroup per pair, everything in f64, no floating-point atomics: every sum is a
// per-lane strided partial sum closed by block_reduce.h, so a pair's bits depend on the pair alone -- not on the batch, the slot
// or the run.
#include "ctx.h"
#include "block_reduce.h"
#include "lm_math.h"

namespace {
constexpr int kRT = 256;        // lanes per pair
constexpr int kRW = kRT / 64;   // waves per pair

// e^2 / (Fx1_0^2 + Fx1_1^2 + Ftx2_0^2 + Ftx2_1^2), the true Sampson distance of one correspondence
__device__ __forceinline__ double refit_sampson(const double (&F)[9], double u1, double v1, double u2, double v2) {
    const double a0 = (F[0] * u1 + F[1] * v1) + F[2], a1 = (F[3] * u1 + F[4] * v1) + F[5], a2 = (F[6] * u1 + F[7] * v1) + F[8];
    const double b0 = (F[0] * u2 + F[3] * v2) + F[6], b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const double e = (u2 * a0 + v2 * a1) + a2;
    return (e * e) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1);
}

__global__ __launch_bounds__(kRT) void refit_fundamental_kernel(const float *__restrict__ xy1, const float *__restrict__ xy2,
                                                                const int32_t *__restrict__ matches,
                                                                const int32_t *__restrict__ best, int kp_stride,
                                                                const float *F_in, float *F_out, double *__restrict__ stats) {
    __shared__ double red[kRW * 45];
    __shared__ double sM[81], sV[81];
    const VsBlockReduce rd{red};
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *p1 = xy1 + (size_t)b * kp_stride * 2, *p2 = xy2 + (size_t)b * kp_stride * 2;
    const int32_t *mt = matches + (size_t)b * kp_stride * 2;
    // F_in is read by every lane before the first barrier and F_out is written behind the last one: they may be one array
    float fin32[9];
    double fin[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        fin32[k] = F_in[(size_t)b * 9 + k];
        fin[k] = (double)fin32[k];
    }
    const int winner = best[b * 4 + 0];
    int n = best[b * 4 + 3];
    n = n < 0 ? 0 : (n > kp_stride ? kp_stride : n);

    // what a lane's correspondence i is: false for an index outside the keypoint slots (skipped, not counted)
    auto load = [&](int i, double &u1, double &v1, double &u2, double &v2) -> bool {
        const int a = mt[2 * i], c = mt[2 * i + 1];
        if (a < 0 || a >= kp_stride || c < 0 || c >= kp_stride) return false;
        u1 = (double)p1[2 * a]; v1 = (double)p1[2 * a + 1];
        u2 = (double)p2[2 * c]; v2 = (double)p2[2 * c + 1];
        return true;
    };

    // 1. count and centroids
    double s5[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += kRT) {
        double u1, v1, u2, v2;
        if (!load(i, u1, v1, u2, v2)) continue;
        s5[0] += 1.0; s5[1] += u1; s5[2] += v1; s5[3] += u2; s5[4] += v2;
    }
    rd.sum(s5);
    const double cnt = s5[0];
    const double cx1 = s5[1] / cnt, cy1 = s5[2] / cnt, cx2 = s5[3] / cnt, cy2 = s5[4] / cnt;

    // mean distance to the centroid
    double s2[2] = {0, 0};
    for (int i = tid; i < n; i += kRT) {
        double u1, v1, u2, v2;
        if (!load(i, u1, v1, u2, v2)) continue;
        const double dx1 = u1 - cx1, dy1 = v1 - cy1, dx2 = u2 - cx2, dy2 = v2 - cy2;
        s2[0] += sqrt(dx1 * dx1 + dy1 * dy1);
        s2[1] += sqrt(dx2 * dx2 + dy2 * dy2);
    }
    rd.sum(s2);
    const double d1 = s2[0] / cnt, d2 = s2[1] / cnt;

    const double qnan = __builtin_nan("");
    // left alone: no winner, fewer than 8 correspondences, all points of an image on one spot (d > 0 is false for NaN too)
    if (winner < 0 || cnt < 8.0 || !(d1 > 0.0) || !(d2 > 0.0)) {   // the same in every lane
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) F_out[(size_t)b * 9 + k] = fin32[k];
            if (stats) {
                stats[(size_t)b * 4 + 0] = cnt;
                stats[(size_t)b * 4 + 1] = stats[(size_t)b * 4 + 2] = stats[(size_t)b * 4 + 3] = qnan;
            }
        }
        return;
    }
    const double sc1 = sqrt(2.0) / d1, sc2 = sqrt(2.0) / d2;

    // 2. M = A^t A over the normalised correspondences, rows u2u1, u2v1, u2, v2u1, v2v1, v2, u1, v1, 1 (src/RansacFilter.cpp:81-89)
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += kRT) {
        double u1, v1, u2, v2;
        if (!load(i, u1, v1, u2, v2)) continue;
        u1 = sc1 * u1 - sc1 * cx1; v1 = sc1 * v1 - sc1 * cy1;   // T x, as the matrix product forms it
        u2 = sc2 * u2 - sc2 * cx2; v2 = sc2 * v2 - sc2 * cy2;
        const double r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0};
#pragma unroll
        for (int p = 0; p < 9; p++) {
#pragma unroll
            for (int q = p; q < 9; q++) acc[vs_lm::lm_tri<9>(p, q)] += r[p] * r[q];
        }
    }
    rd.sum(acc);
    // acc is indexed with constants only (it lives in registers): each lane picks its element through a chain of selects
    if (tid < 81) {
        const int i = tid / 9, j = tid % 9, lo = i < j ? i : j, hi = i < j ? j : i;
        double m = 0.0;
#pragma unroll
        for (int p = 0; p < 9; p++) {
#pragma unroll
            for (int q = p; q < 9; q++) m = (p == lo && q == hi) ? acc[vs_lm::lm_tri<9>(p, q)] : m;
        }
        sM[tid] = m;
        sV[tid] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();

    // 3. cyclic Jacobi on M (in LDS; lane k < 9 owns row and column k of a rotation, every lane walks the same control flow)
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0, tr = 0.0;
        for (int i = 0; i < 9; i++) {
            tr += sM[i * 9 + i];
            for (int j = i + 1; j < 9; j++) off += sM[i * 9 + j] * sM[i * 9 + j];
        }
        if (sqrt(2.0 * off) <= 0x1p-52 * tr) break;
        for (int p = 0; p < 8; p++) {
            for (int q = p + 1; q < 9; q++) {
                const double app = sM[p * 9 + p], aqq = sM[q * 9 + q], apq = sM[p * 9 + q];
                double akp = 0, akq = 0, vkp = 0, vkq = 0;
                if (tid < 9) {
                    akp = sM[tid * 9 + p]; akq = sM[tid * 9 + q];
                    vkp = sV[tid * 9 + p]; vkq = sV[tid * 9 + q];
                }
                __syncthreads();   // everything of this rotation has been read
                if (apq != 0.0 && tid < 9) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    if (tid == p) {
                        sM[p * 9 + p] = app - t * apq;
                        sM[p * 9 + q] = 0.0;
                    } else if (tid == q) {
                        sM[q * 9 + q] = aqq + t * apq;
                        sM[q * 9 + p] = 0.0;
                    } else {
                        const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
                        sM[tid * 9 + p] = nkp; sM[p * 9 + tid] = nkp;
                        sM[tid * 9 + q] = nkq; sM[q * 9 + tid] = nkq;
                    }
                    sV[tid * 9 + p] = c * vkp - s * vkq;
                    sV[tid * 9 + q] = s * vkp + c * vkq;
                }
                __syncthreads();
            }
        }
    }
    // the two smallest eigenvalues (the first of equal ones)
    int i9 = 0;
    for (int i = 1; i < 9; i++)
        if (sM[i * 9 + i] < sM[i9 * 9 + i9]) i9 = i;
    int i8 = i9 == 0 ? 1 : 0;
    for (int i = 0; i < 9; i++)
        if (i != i9 && sM[i * 9 + i] < sM[i8 * 9 + i8]) i8 = i;
    const double lam9 = sM[i9 * 9 + i9], lam8 = sM[i8 * 9 + i8];

    // 4. rank 2: one-sided Jacobi on the 3 x 3 (G = Fh W with orthogonal columns: Fh = G W^t, the column norms of G are the
    // singular values), the column of the smallest norm dropped from the product
    double g[3][3], w[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            g[r][c] = sV[(3 * r + c) * 9 + i9];
            w[r][c] = r == c ? 1.0 : 0.0;
        }
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int pr = 0; pr < 3; pr++) {
            const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
            const double al = (g[0][i] * g[0][i] + g[1][i] * g[1][i]) + g[2][i] * g[2][i];
            const double be = (g[0][j] * g[0][j] + g[1][j] * g[1][j]) + g[2][j] * g[2][j];
            const double ga = (g[0][i] * g[0][j] + g[1][i] * g[1][j]) + g[2][i] * g[2][j];
            if (!(fabs(ga) > 0x1p-51 * sqrt(al * be))) continue;
            rotated = true;
            const double zeta = (be - al) / (2.0 * ga);
            const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double gi = g[r][i], gj = g[r][j], wi = w[r][i], wj = w[r][j];
                g[r][i] = c * gi - s * gj; g[r][j] = s * gi + c * gj;
                w[r][i] = c * wi - s * wj; w[r][j] = s * wi + c * wj;
            }
        }
        if (!rotated) break;
    }
    double nrm[3];
#pragma unroll
    for (int c = 0; c < 3; c++) nrm[c] = (g[0][c] * g[0][c] + g[1][c] * g[1][c]) + g[2][c] * g[2][c];
    const int cmin = (nrm[1] < nrm[0]) ? (nrm[2] < nrm[1] ? 2 : 1) : (nrm[2] < nrm[0] ? 2 : 0);
    double fh[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            double acc3 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; c++) acc3 += (c == cmin) ? 0.0 : g[r][c] * w[k][c];
            fh[r][k] = acc3;
        }
    }

    // 5. F = T2^t Fh T1, over its Frobenius norm;  6. the sign of F_in
    const double tx1 = -(sc1 * cx1), ty1 = -(sc1 * cy1), tx2 = -(sc2 * cx2), ty2 = -(sc2 * cy2);
    double a[3][3], F[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        a[r][0] = fh[r][0] * sc1;
        a[r][1] = fh[r][1] * sc1;
        a[r][2] = (fh[r][0] * tx1 + fh[r][1] * ty1) + fh[r][2];
    }
    double fro = 0.0, dot = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        F[0 + c] = sc2 * a[0][c];
        F[3 + c] = sc2 * a[1][c];
        F[6 + c] = (tx2 * a[0][c] + ty2 * a[1][c]) + a[2][c];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) fro += F[k] * F[k];
    fro = sqrt(fro);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        F[k] = F[k] / fro;
        dot += F[k] * fin[k];
    }
    // 7. one rounding to f32
    float fout32[9];
    double fout[9];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        fout32[k] = (float)(dot < 0.0 ? -F[k] : F[k]);
        fout[k] = (double)fout32[k];
        finite = finite && isfinite(fout32[k]);
    }

    double ss[2] = {0, 0};
    if (stats && finite) {   // the same in every lane
        for (int i = tid; i < n; i += kRT) {
            double u1, v1, u2, v2;
            if (!load(i, u1, v1, u2, v2)) continue;
            ss[0] += refit_sampson(fin, u1, v1, u2, v2);
            ss[1] += refit_sampson(fout, u1, v1, u2, v2);
        }
        rd.sum(ss);
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) F_out[(size_t)b * 9 + k] = finite ? fout32[k] : fin32[k];
        if (stats) {
            stats[(size_t)b * 4 + 0] = cnt;
            stats[(size_t)b * 4 + 1] = finite ? ss[0] / cnt : qnan;
            stats[(size_t)b * 4 + 2] = finite ? ss[1] / cnt : qnan;
            stats[(size_t)b * 4 + 3] = finite ? lam9 / lam8 : qnan;
        }
    }
}
}  // namespace

int vs_launch_refit(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *matches, const int32_t *best, int batch,
                    int kp_stride, const float *F_in, float *F_out, double *stats) {
    VS_REQUIRE(ctx, xy1 && xy2 && matches && best && F_in && F_out, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && kp_stride > 0, VSLAM_ERR_INVALID);
    VsProfScope ps(ctx, "refit_fundamental_kernel");
    refit_fundamental_kernel<<<batch, kRT, 0, ctx->stream>>>(xy1, xy2, matches, best, kp_stride, F_in, F_out, stats);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

extern "C" int vslam_refit_fundamental(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const int32_t *d_matches,
                                       const int32_t *d_best, int batch, int kp_stride, const float *d_F_in, float *d_F_out,
                                       double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_ALIGNED(ctx, d_xy1, 8);
    VS_ALIGNED(ctx, d_xy2, 8);
    VS_ALIGNED(ctx, d_matches, 8);
    VS_ALIGNED(ctx, d_stats, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_best, d_F_in, d_F_out) % 4 == 0, VSLAM_ERR_INVALID);
    return vs_launch_refit(ctx, d_xy1, d_xy2, d_matches, d_best, batch, kp_stride, d_F_in, d_F_out, d_stats);
}
