// The arithmetic of the window adjustment (vslam_adjust_windows, include/vslam_adjust.h) that does not know about lanes: one
// observation's blocks, the entries of the reduced system, its Cholesky solve, and the rounds of the iteration written over one
// policy (Ex) that says who walks which points, entries and rows and how a sum over the points is closed.  adjust.hip runs it
// with 256 lanes per item; tests/native/adjust_serial.cpp compiles the same text for the host, walks everything one after the
// other and is held to tests/ref_adjust.py without a GPU.  The camera, its start and candidate, the Jacobian's pieces and a
// point's damped 3 x 3 solve are lm_math.h's.  All f64, never fused (compile host code with -ffp-contract=off).
#pragma once

#include <cstdint>

#include "lm_math.h"

namespace vs_adjust {
using namespace vs_lm;

constexpr int kAdMaxCams = 8;                 // VSLAM_ADJUST_MAX_CAMS
constexpr int kAdMaxSlots = kAdMaxCams - 1;   // n_fixed >= 1
constexpr int kAdMaxN = 6 * kAdMaxSlots;      // unknowns of the reduced system
constexpr int kAdLd = kAdMaxN + 1;            // row pitch of S: odd, so that a column walk changes bank
// what a point keeps per slot between the passes: W [6][3] at 0, Y [6][3] at 18, U (upper 21) at 36, gc [6] at 57
constexpr int kAdW = 0, kAdY = 18, kAdU = 36, kAdG = 57, kAdStage = 63;
constexpr int kAdActive = 1 << 8;             // in a point's mask: it takes part; bits 0 .. 6: the slots it has observations in

struct AdParams {
    int max_iterations, rounds, min_obs, n_fixed;
    double huber, gate;
};

struct AdItem {   // the caller's arrays of one item
    int C, N, cam_stride, pt_stride, obs_stride;
    const double *R, *T, *X;
    const int32_t *off, *cam;
    const float *xy;
};

struct AdWork {   // per point and per observation, between the passes
    double *Xa, *Xb;    // [N][3] the points and their candidate (the two change places when a step is accepted)
    double *z;          // [N][3]
    double *stage;      // [N][kAdMaxSlots][kAdStage]
    int32_t *mask;      // [N]
    uint8_t *fa, *fb;   // [observations] participation of the round and of the round being decided
};

struct AdShared {   // one per item (LDS on the device)
    double S[kAdMaxN * kAdLd];   // lower triangle: S, then L below the diagonal
    double Ld[kAdMaxN], Ud[kAdMaxN], rhs[kAdMaxN], dc[kAdMaxN];
    LmCam start[kAdMaxCams], cur[kAdMaxCams], cand[kAdMaxCams];
    int slot[kAdMaxCams];
    int flag;
};

struct AdResult {
    const double *X;        // [N][3] the points of the result
    const uint8_t *flags;   // the participants of the last round that ran
    int ever_free;     // bit c: camera c was free in some round
};

LM_FN double ad_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// one observation's blocks at (c, X): V (upper 6: 00 01 02 11 12 22), gx, and -- for a free camera -- st[kAdW], st[kAdU], st[kAdG]
LM_FN void ad_blocks(const double (&K)[9], const LmCam &c, double delta, const double (&X)[3], const double (&x)[2], bool free_cam,
                     double (&V)[6], double (&gx)[3], double (&st)[kAdStage]) {
    LmPoint o;
    lm_point(K, c, X, x, o);
    double A[2][3], Jx[2][3], Jc[2][6];
    lm_dproj(K, o.u, o.v, o.q2, A);
    lm_jac_point(A, c.R, Jx);
    lm_jac_rotation(A, o.RX, Jc);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        Jc[r][3] = A[r][0];
        Jc[r][4] = A[r][1];
        Jc[r][5] = A[r][2];
    }
    const double w = lm_weight(o.e, delta);
    int t = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = i; j < 3; j++) V[t++] = w * (Jx[0][i] * Jx[0][j] + Jx[1][i] * Jx[1][j]);
        gx[i] = w * (Jx[0][i] * o.r[0] + Jx[1][i] * o.r[1]);
    }
    if (!free_cam) return;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) st[kAdW + 3 * i + j] = w * (Jc[0][i] * Jx[0][j] + Jc[1][i] * Jx[1][j]);
#pragma unroll
        for (int j = i; j < 6; j++) st[kAdU + lm_tri<6>(i, j)] = w * (Jc[0][i] * Jc[0][j] + Jc[1][i] * Jc[1][j]);
        st[kAdG + i] = w * (Jc[0][i] * o.r[0] + Jc[1][i] * o.r[1]);
    }
}

// entry e of the reduced system over the points in ascending order: e < n is rhs[e]; the others walk the upper triangle row by
// row, (I, J) with I <= J, stored at S[J][I]
LM_FN void ad_entry(int e, int n, int N, const AdWork &w, AdShared &sh) {
    if (e < n) {
        const int a = e / 6, j = e % 6;
        double acc = 0.0;
        for (int i = 0; i < N; i++) {
            if (!((w.mask[i] >> a) & 1)) continue;
            const double *row = w.stage + ((size_t)i * kAdMaxSlots + a) * kAdStage;
            acc += row[kAdG + j] - ad_dot(row + kAdW + 3 * j, w.z + 3 * (size_t)i);
        }
        sh.rhs[e] = acc;
        return;
    }
    int t = e - n, I = 0;
    while (t >= n - I) {
        t -= n - I;
        I++;
    }
    const int J = I + t, a = I / 6, j = I % 6, b = J / 6, l = J % 6;
    double acc = 0.0, accu = 0.0;
    if (a == b) {
        const int u = kAdU + lm_tri<6>(j, l);
        for (int i = 0; i < N; i++) {
            if (!((w.mask[i] >> a) & 1)) continue;
            const double *row = w.stage + ((size_t)i * kAdMaxSlots + a) * kAdStage;
            acc += row[u] - ad_dot(row + kAdY + 3 * j, row + kAdW + 3 * l);
            accu += row[u];
        }
        if (j == l) sh.Ud[I] = accu;
    } else {
        for (int i = 0; i < N; i++) {
            const int m = w.mask[i];
            if (!((m >> a) & (m >> b) & 1)) continue;
            const double *ra = w.stage + ((size_t)i * kAdMaxSlots + a) * kAdStage;
            const double *rb = w.stage + ((size_t)i * kAdMaxSlots + b) * kAdStage;
            acc += -ad_dot(ra + kAdY + 3 * j, rb + kAdW + 3 * l);
        }
    }
    sh.S[J * kAdLd + I] = acc;
}

// row i's part of column j of the factor: the pivot p_j (every row forms it alike) and L_ij
LM_FN void ad_chol_column(int i, int j, double lambda, AdShared &sh) {
    if (i < j) return;
    double p = sh.S[j * kAdLd + j] + lambda * fmax(sh.Ud[j], kDiagFloor);
    for (int k = 0; k < j; k++) p = p - sh.S[j * kAdLd + k] * sh.S[j * kAdLd + k];
    if (i == j) {
        if (!(p > 0.0)) sh.flag = 1;
        sh.Ld[j] = sqrt(p);
        return;
    }
    double s = sh.S[i * kAdLd + j];
    for (int k = 0; k < j; k++) s = s - sh.S[i * kAdLd + k] * sh.S[j * kAdLd + k];
    sh.S[i * kAdLd + j] = s / sqrt(p);
}

// L L^t d = rhs, dc = -d; raises the flag for a dc that is not finite
LM_FN void ad_substitute(int n, AdShared &sh) {
    double *f = sh.dc;
    for (int i = 0; i < n; i++) {
        double s = sh.rhs[i];
        for (int k = 0; k < i; k++) s = s - sh.S[i * kAdLd + k] * f[k];
        f[i] = s / sh.Ld[i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = f[i];
        for (int k = n - 1; k > i; k--) s = s - sh.S[k * kAdLd + i] * f[k];
        f[i] = s / sh.Ld[i];
    }
    for (int i = 0; i < n; i++) {
        f[i] = -f[i];
        if (!std::isfinite(f[i])) sh.flag = 1;
    }
}

// whether point i has a participant among its observations
LM_FN bool ad_took_part(const int32_t *off, const uint8_t *flags, int i) {
    bool any = false;
    for (int k = off[i]; k < off[i + 1]; k++) any = any || flags[k] != 0;
    return any;
}

LM_FN bool ad_finite3(const double (&v)[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// The rounds of the adjustment.  Ex::points(N, f) calls f(i) for the points this caller owns (all of them on the host; l, l + 256,
// ... for lane l), Ex::entries(n, f) and Ex::rows(n, f) likewise for the entries of the reduced system (strided) and for rows
// (row i is lane i's), Ex::one(f) for one caller; Ex::sum closes partial sums over all callers and Ex::any a flag, the same value
// everywhere afterwards; Ex::sync() makes what the callers wrote visible to one another.  Every decision is taken alike by every
// caller.  Returns true with the cameras in sh.cur and the points in res.X when the item moved.
template <class Ex>
LM_FN bool ad_run(const double (&K)[9], const AdItem &it, const AdParams &p, const AdWork &w, AdShared &sh, Ex &ex, AdResult &res,
                  double (&stats)[4]) {
    const double qnan = __builtin_nan("");
    stats[0] = 0.0;
    stats[1] = stats[2] = stats[3] = qnan;
    const int C = it.C, N = it.N;
    if (C < 1 || C > it.cam_stride || C > kAdMaxCams || N < 0 || N > it.pt_stride) return false;
    bool bad = false;
    ex.points(N, [&](int i) {
        const int a = it.off[i], b = it.off[i + 1];
        bad = bad || a < 0 || b < a || b > it.obs_stride;
    });
#pragma unroll
    for (int k = 0; k < 9; k++) bad = bad || !std::isfinite(K[k]);
    ex.rows(C, [&](int c) {
        LmCam in;
#pragma unroll
        for (int k = 0; k < 9; k++) in.R[k] = it.R[9 * c + k];
#pragma unroll
        for (int k = 0; k < 3; k++) in.T[k] = it.T[3 * c + k];
        bad = bad || !lm_finite(in);
        LmCam st = in;
        if (c >= p.n_fixed) lm_cam_start(in, st);
        sh.start[c] = st;
        sh.cur[c] = st;
    });
    if (ex.any(bad)) return false;
    ex.points(N, [&](int i) {
#pragma unroll
        for (int k = 0; k < 3; k++) w.Xa[3 * (size_t)i + k] = it.X[3 * (size_t)i + k];
    });
    ex.sync();

    double *Xc = w.Xa, *Xn = w.Xb;
    uint8_t *fl = w.fa, *fn = w.fb;
    int accepted = 0, nslot = 0;
    bool ran = false;
    res.ever_free = 0;

    // sum of rho over the participants (flags fl) under (cams, Xp), and whether one of them is not in front of its camera
    auto objective = [&](const LmCam *cams, const double *Xp, double &obj, bool &behind) {
        double so[1] = {0.0};
        bool bh = false;
        ex.points(N, [&](int i) {
            const double X[3] = {Xp[3 * (size_t)i], Xp[3 * (size_t)i + 1], Xp[3 * (size_t)i + 2]};
            for (int k = it.off[i]; k < it.off[i + 1]; k++) {
                if (!fl[k]) continue;
                const float ox = it.xy[2 * (size_t)k], oy = it.xy[2 * (size_t)k + 1];
                const double x[2] = {(double)ox, (double)oy};
                LmPoint o;
                lm_point(K, cams[it.cam[k]], X, x, o);
                so[0] += lm_rho(o.e, p.huber);
                bh = bh || !(o.Y[2] > 0.0);
            }
        });
        ex.sum(so);
        behind = ex.any(bh);
        obj = so[0];
    };

    for (int round = 0; round < p.rounds; round++) {
        // who takes part, decided under the current iterate into fn
        double cnt[kAdMaxCams + 1];
#pragma unroll
        for (int c = 0; c <= kAdMaxCams; c++) cnt[c] = 0.0;
        ex.points(N, [&](int i) {
            const double X[3] = {Xc[3 * (size_t)i], Xc[3 * (size_t)i + 1], Xc[3 * (size_t)i + 2]};
            const bool xfin = ad_finite3(X);
            int cams = 0;
            for (int k = it.off[i]; k < it.off[i + 1]; k++) {
                const int c = it.cam[k];
                const float ox = it.xy[2 * (size_t)k], oy = it.xy[2 * (size_t)k + 1];
                bool take = false;
                if (xfin && c >= 0 && c < C && std::isfinite(ox) && std::isfinite(oy)) {
                    const double x[2] = {(double)ox, (double)oy};
                    LmPoint o;
                    lm_point(K, sh.cur[c], X, x, o);
                    take = o.Y[2] > 0.0 && (round == 0 || o.e <= p.gate);
                }
                fn[k] = take ? 1 : 0;
                if (take) cams |= 1 << c;
            }
            const bool active = (cams & (cams - 1)) != 0;   // two distinct cameras
            for (int k = it.off[i]; k < it.off[i + 1]; k++) {
                if (!fn[k]) continue;
                if (!active) {
                    fn[k] = 0;
                    continue;
                }
                const int c = it.cam[k];
#pragma unroll
                for (int q = 0; q < kAdMaxCams; q++) cnt[q] += c == q ? 1.0 : 0.0;
                cnt[kAdMaxCams] += 1.0;
            }
        });
        ex.sum(cnt);   // counts: exact in any order
        int slots[kAdMaxCams], ns = 0, free_mask = 0;
#pragma unroll
        for (int c = 0; c < kAdMaxCams; c++) {
            const bool fr = c < C && c >= p.n_fixed && cnt[c] >= (double)p.min_obs;
            slots[c] = fr ? ns : -1;
            ns += fr ? 1 : 0;
            free_mask |= fr ? 1 << c : 0;
        }
        if (ns == 0) {
            if (round == 0) stats[0] = cnt[kAdMaxCams];
            break;   // the previous round's result stands
        }
        nslot = ns;
        ran = true;
        res.ever_free |= free_mask;
        stats[0] = cnt[kAdMaxCams];
        {
            uint8_t *t = fl;
            fl = fn;
            fn = t;
        }
        ex.rows(kAdMaxCams, [&](int c) {
            int s = -1;
#pragma unroll
            for (int q = 0; q < kAdMaxCams; q++) s = c == q ? slots[q] : s;
            sh.slot[c] = s;
        });
        ex.sync();
        const int n = 6 * nslot;

        double obj, lambda = kLambda0;
        bool behind0;
        objective(sh.cur, Xc, obj, behind0);
        for (int iter = 0; iter < p.max_iterations; iter++) {
            // 1. per point: the blocks of its observations, V* = L L^t, z and Y
            bool refuse = false;
            ex.one([&]() { sh.flag = 0; });
            ex.points(N, [&](int i) {
                const double X[3] = {Xc[3 * (size_t)i], Xc[3 * (size_t)i + 1], Xc[3 * (size_t)i + 2]};
                double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gx[3] = {0.0, 0.0, 0.0};
                int m = 0;
                bool any = false;
                for (int k = it.off[i]; k < it.off[i + 1]; k++) {
                    if (!fl[k]) continue;
                    any = true;
                    const int c = it.cam[k], s = sh.slot[c];
                    const float ox = it.xy[2 * (size_t)k], oy = it.xy[2 * (size_t)k + 1];
                    const double x[2] = {(double)ox, (double)oy};
                    double Vo[6], go[3], st[kAdStage];
                    ad_blocks(K, sh.cur[c], p.huber, X, x, s >= 0, Vo, go, st);
#pragma unroll
                    for (int q = 0; q < 6; q++) V[q] += Vo[q];
#pragma unroll
                    for (int q = 0; q < 3; q++) gx[q] += go[q];
                    if (s < 0) continue;
                    double *row = w.stage + ((size_t)i * kAdMaxSlots + s) * kAdStage;
                    if ((m >> s) & 1) {   // the camera's second observation of the point
#pragma unroll
                        for (int q = 0; q < kAdStage; q++) {
                            if (q < kAdY || q >= kAdU) row[q] = row[q] + st[q];
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < kAdStage; q++) {
                            if (q < kAdY || q >= kAdU) row[q] = st[q];
                        }
                        m |= 1 << s;
                    }
                }
                if (!any) {
                    w.mask[i] = 0;
                    return;
                }
                const LmChol3 ch = lm_chol3(V, lambda);
                refuse = refuse || !ch.ok;
                double z[3];
                ch.solve(gx, z);
#pragma unroll
                for (int q = 0; q < 3; q++) w.z[3 * (size_t)i + q] = z[q];
                for (int s = 0; s < kAdMaxSlots; s++) {
                    if (!((m >> s) & 1)) continue;
                    double *row = w.stage + ((size_t)i * kAdMaxSlots + s) * kAdStage;
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        const double b[3] = {row[kAdW + 3 * j], row[kAdW + 3 * j + 1], row[kAdW + 3 * j + 2]};
                        double y[3];
                        ch.solve(b, y);
                        row[kAdY + 3 * j] = y[0];
                        row[kAdY + 3 * j + 1] = y[1];
                        row[kAdY + 3 * j + 2] = y[2];
                    }
                }
                w.mask[i] = m | kAdActive;
            });
            refuse = ex.any(refuse);
            ex.sync();
            bool accept = false;
            double obj_new = 0.0;
            if (!refuse) {
                // 2. the reduced system and its solve
                ex.entries(n + n * (n + 1) / 2, [&](int e) { ad_entry(e, n, N, w, sh); });
                ex.sync();
                for (int j = 0; j < n; j++) {
                    ex.rows(n, [&](int i) { ad_chol_column(i, j, lambda, sh); });
                    ex.sync();
                }
                ex.one([&]() { ad_substitute(n, sh); });
                ex.sync();
                // 3. the candidate
                bool badx = false;
                ex.rows(C, [&](int c) {
                    const int s = sh.slot[c];
                    if (s < 0) {
                        sh.cand[c] = sh.cur[c];
                        return;
                    }
                    double d[6];
#pragma unroll
                    for (int q = 0; q < 6; q++) d[q] = sh.dc[6 * s + q];
                    lm_cam_step(sh.cur[c], d, sh.cand[c]);
                    badx = badx || !lm_finite(sh.cand[c]);
                });
                ex.points(N, [&](int i) {
                    const int m = w.mask[i];
                    double Xo[3] = {Xc[3 * (size_t)i], Xc[3 * (size_t)i + 1], Xc[3 * (size_t)i + 2]};
                    if (m & kAdActive) {
                        double acc[3] = {w.z[3 * (size_t)i], w.z[3 * (size_t)i + 1], w.z[3 * (size_t)i + 2]};
                        for (int s = 0; s < kAdMaxSlots; s++) {
                            if (!((m >> s) & 1)) continue;
                            const double *Y = w.stage + ((size_t)i * kAdMaxSlots + s) * kAdStage + kAdY;
#pragma unroll
                            for (int q = 0; q < 3; q++) {
                                double yd = Y[q] * sh.dc[6 * s];
#pragma unroll
                                for (int j = 1; j < 6; j++) yd = yd + Y[3 * j + q] * sh.dc[6 * s + j];
                                acc[q] = acc[q] + yd;
                            }
                        }
#pragma unroll
                        for (int q = 0; q < 3; q++) Xo[q] = Xo[q] + (-acc[q]);
                        badx = badx || !ad_finite3(Xo);
                    }
#pragma unroll
                    for (int q = 0; q < 3; q++) Xn[3 * (size_t)i + q] = Xo[q];
                });
                badx = ex.any(badx);
                ex.sync();
                const bool flagged = sh.flag != 0;
                bool behind;
                objective(sh.cand, Xn, obj_new, behind);
                accept = !flagged && !badx && !behind && obj_new < obj;   // false for a NaN objective
            }
            if (accept) {
                const double rel = (obj - obj_new) / obj;
                ex.sync();   // the candidate has been read by everyone
                ex.rows(C, [&](int c) { sh.cur[c] = sh.cand[c]; });
                {
                    double *t = Xc;
                    Xc = Xn;
                    Xn = t;
                }
                ex.sync();
                obj = obj_new;
                accepted++;
                lambda = fmax(lambda / 10.0, kLambdaMin);
                if (rel < kRelStop) break;
            } else {
                lambda = lambda * 10.0;
                if (lambda > kLambdaMax) break;
            }
        }
    }
    if (!ran || accepted == 0) return false;
    bool fin = true;
    for (int c = 0; c < C; c++) fin = fin && lm_finite(sh.cur[c]);
    double s0, s1;
    bool b0, b1;
    objective(sh.start, it.X, s0, b0);
    objective(sh.cur, Xc, s1, b1);
    const double m0 = s0 / stats[0], m1 = s1 / stats[0];
    if (!(fin && std::isfinite(m0) && std::isfinite(m1))) return false;
    stats[1] = m0;
    stats[2] = m1;
    stats[3] = (double)accepted;
    res.X = Xc;
    res.flags = fl;
    return true;
}
}  // namespace vs_adjust
