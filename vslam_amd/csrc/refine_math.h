// The arithmetic of the two-view bundle adjustment (vslam_refine_pairs, include/vslam_amd.h) that does not know about lanes:
// one point's blocks, the reduced 5 x 5 solve, the candidate camera, and the whole refinement (ba_run) written over one policy
// (Ex) that says whose the correspondences are, where their observations, points and f64 state live, and how a sum over them is
// closed.  refine.hip runs it with 256 lanes per pair; tests/native/refine_serial.cpp compiles the same text for the host, walks
// the correspondences one after the other and is held to tests/ref_refine.py without a GPU.  What it shares with the other
// optimizers is lm_math.h.  All f64, never fused (compile host code with -ffp-contract=off).
#pragma once

#include <cstdint>

#include "lm_math.h"

namespace vs_refine {
using namespace vs_lm;

// squared reprojection errors of one point in the two images
LM_FN void ba_errors(const double (&K)[9], const LmCam &c, const double (&X)[3], const double (&o)[4], double &e1,
                                          double &e2, double &depth2) {
    double u, v, q2, RX[3], Y[3];
    lm_project(K, X, u, v, q2);
    double du = u - o[0], dv = v - o[1];
    e1 = du * du + dv * dv;
    lm_transform(c.R, c.T, X, RX, Y);
    lm_project(K, Y, u, v, q2);
    du = u - o[2];
    dv = v - o[3];
    e2 = du * du + dv * dv;
    depth2 = Y[2];
}

// One point's blocks at (c, X), damped by lambda: Yv = V*^-1 W^t (3 x 5), z = V*^-1 g_x, and what the point adds to the reduced
// system (acc[0..15): U - W Yv with U's diagonal times (1 + lambda); acc[15..20): g_c - W z).  false when V* has a pivot that is
// not > 0 (the step is then refused).
LM_FN bool ba_point_blocks(const double (&K)[9], const LmCam &c, const double (&b1)[3], const double (&b2)[3],
                                                double lambda, const double (&X)[3], const double (&o)[4], double (&Yv)[3][5],
                                                double (&z)[3], double (&acc)[20]) {
    double u1, v1, q, u2, v2, RX[3], Y[3], A1[2][3], A2[2][3];
    lm_project(K, X, u1, v1, q);
    lm_dproj(K, u1, v1, q, A1);
    lm_transform(c.R, c.T, X, RX, Y);
    lm_project(K, Y, u2, v2, q);
    lm_dproj(K, u2, v2, q, A2);
    const double r1[2] = {u1 - o[0], v1 - o[1]}, r2[2] = {u2 - o[2], v2 - o[3]};
    // J2x = A2 R; Jc = A2 [-[RX]x | b1 | b2]
    double J2x[2][3], Jc[2][5];
    lm_jac_point(A2, c.R, J2x);
    lm_jac_rotation(A2, RX, Jc);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        Jc[r][3] = (A2[r][0] * b1[0] + A2[r][1] * b1[1]) + A2[r][2] * b1[2];
        Jc[r][4] = (A2[r][0] * b2[0] + A2[r][1] * b2[1]) + A2[r][2] * b2[2];
    }
    double V[6], gx[3], W[5][3], gc[5];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = i; j < 3; j++)
            V[lm_tri<3>(i, j)] = ((A1[0][i] * A1[0][j] + A1[1][i] * A1[1][j]) + J2x[0][i] * J2x[0][j]) + J2x[1][i] * J2x[1][j];
        gx[i] = ((A1[0][i] * r1[0] + A1[1][i] * r1[1]) + J2x[0][i] * r2[0]) + J2x[1][i] * r2[1];
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int j = 0; j < 3; j++) W[k][j] = Jc[0][k] * J2x[0][j] + Jc[1][k] * J2x[1][j];
        gc[k] = Jc[0][k] * r2[0] + Jc[1][k] * r2[1];
    }
    const LmChol3 ch = lm_chol3(V, lambda);
#pragma unroll
    for (int k = 0; k < 5; k++) {
        double y[3];
        ch.solve(W[k], y);
        Yv[0][k] = y[0];
        Yv[1][k] = y[1];
        Yv[2][k] = y[2];
    }
    ch.solve(gx, z);
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int l = k; l < 5; l++) {
            double uu = Jc[0][k] * Jc[0][l] + Jc[1][k] * Jc[1][l];
            if (k == l) uu = uu + lambda * uu;
            acc[lm_tri<5>(k, l)] = uu - ((W[k][0] * Yv[0][l] + W[k][1] * Yv[1][l]) + W[k][2] * Yv[2][l]);
        }
        acc[15 + k] = gc[k] - ((W[k][0] * z[0] + W[k][1] * z[1]) + W[k][2] * z[2]);
    }
    return ch.ok;
}

// b1 = normalize(t x e_k), k the axis of the smallest |t_k| (the lowest on a tie); b2 = t x b1
LM_FN void ba_tangent(const double (&t)[3], double (&b1)[3], double (&b2)[3]) {
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    const int k = (a1 < a0) ? (a2 < a1 ? 2 : 1) : (a2 < a0 ? 2 : 0);
    double c[3];
    if (k == 0) { c[0] = 0.0; c[1] = t[2]; c[2] = -t[1]; }
    else if (k == 1) { c[0] = -t[2]; c[1] = 0.0; c[2] = t[0]; }
    else { c[0] = t[1]; c[1] = -t[0]; c[2] = 0.0; }
    const double nrm = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) b1[i] = c[i] / nrm;
    b2[0] = t[1] * b1[2] - t[2] * b1[1];
    b2[1] = t[2] * b1[0] - t[0] * b1[2];
    b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// the candidate camera of a step dc: R' = exp([w]x) R, t' = normalize(t + dc[3] b1 + dc[4] b2)
LM_FN void ba_candidate(const LmCam &cur, const double (&b1)[3], const double (&b2)[3], const double (&dc)[5], LmCam &cand) {
    const double w[3] = {dc[0], dc[1], dc[2]};
    lm_rotate(w, cur.R, cand.R);
    double tt[3];
#pragma unroll
    for (int k = 0; k < 3; k++) tt[k] = (cur.T[k] + dc[3] * b1[k]) + dc[4] * b2[k];
    const double nn = sqrt((tt[0] * tt[0] + tt[1] * tt[1]) + tt[2] * tt[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) cand.T[k] = tt[k] / nn;
}

// a point's step from its blocks: X' = X - (z + Yv dc)
LM_FN void ba_point_step(const double (&X)[3], const double (&Yv)[3][5], const double (&z)[3], const double (&dc)[5], double (&Xn)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double yd = (((Yv[k][0] * dc[0] + Yv[k][1] * dc[1]) + Yv[k][2] * dc[2]) + Yv[k][3] * dc[3]) + Yv[k][4] * dc[4];
        Xn[k] = X[k] - (z[k] + yd);
    }
}

// c2 = K [R | t] in f64, products summed left to right, one rounding
LM_FN void ba_camera(const double (&K)[9], const LmCam &c, float (&c2)[12]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) c2[4 * r + k] = (float)((K[3 * r] * c.R[k] + K[3 * r + 1] * c.R[3 + k]) + K[3 * r + 2] * c.R[6 + k]);
        c2[4 * r + 3] = (float)((K[3 * r] * c.T[0] + K[3 * r + 1] * c.T[1]) + K[3 * r + 2] * c.T[2]);
    }
}

struct BaResult {
    LmCam cam;                          // the result before its rounding
    float R32[9], t32[3], c2[12];       // what the caller writes: the result's one rounding to f32, and K [R | t] of cam
    int buf;                            // the half of the state that holds the accepted points (f64)
    double objective;                   // the objective at cam and those points
};

// The refinement of one pair over its correspondences 0 .. n.  Ex::each(n, f) calls f(i) for the correspondences this caller owns
// (all of them on the host; l, l + 256, ... for lane l); Ex::observed(i, o) reads correspondence i's two keypoints, false when it
// has none; Ex::input(i, X) its input point; Ex::state(buf, k, i) is coordinate k of its accepted or candidate point and
// Ex::flag(i) its participation byte, both kept from pass to pass; Ex::sum closes partial sums over all callers and Ex::any a
// flag, the same value everywhere afterwards, so every decision below is taken alike by every caller.  Returns true with the
// result in `res` when the pair moved, false when it is left alone; stats as include/vslam_amd.h states them.
template <class Ex>
LM_FN bool ba_run(const double (&K)[9], const LmCam &in, int winner, int n, double gate_sq, int max_iterations, Ex &ex, BaResult &res,
                  double (&stats)[4]) {
    stats[1] = stats[2] = stats[3] = __builtin_nan("");
    // 1. the participating correspondences, fixed here; their count and objective under the inputs
    double s2[2] = {0, 0};
    ex.each(n, [&](int i) {
        double o[4], X[3], e1, e2, dz;
        bool part = ex.observed(i, o);
        if (part) {
            ex.input(i, X);
            ba_errors(K, in, X, o, e1, e2, dz);
            // every test is evaluated (& on bools, not &&): a lazy chain would put each keypoint's load behind the test before it
            part = std::isfinite(X[0]) & std::isfinite(X[1]) & std::isfinite(X[2]) & (X[2] > 0.0) & (dz > 0.0) & (e1 <= gate_sq) & (e2 <= gate_sq);
        }
        ex.flag(i) = part ? 1 : 0;
        if (part) {
#pragma unroll
            for (int k = 0; k < 3; k++) ex.state(0, k, i) = X[k];
            s2[0] += 1.0;
            s2[1] += e1 + e2;
        }
    });
    ex.sum(s2);
    const double cnt = s2[0];
    stats[0] = cnt;
    const double tn = sqrt((in.T[0] * in.T[0] + in.T[1] * in.T[1]) + in.T[2] * in.T[2]);
    const bool t_ok = std::isfinite(in.T[0]) && std::isfinite(in.T[1]) && std::isfinite(in.T[2]) && tn > 0.0;
    if (winner < 0 || cnt < 8.0 || !t_ok) return false;   // the same everywhere
    const double mean_in = s2[1] / (2.0 * cnt);

    // 2. the start: R one Newton step of the polar iteration closer to a rotation; t / |t|
    LmCam cur;
    lm_polar_step(in.R, cur.R);
#pragma unroll
    for (int k = 0; k < 3; k++) cur.T[k] = in.T[k] / tn;
    int acc_buf = 0;   // which half of the state holds the accepted points

    double s1[1] = {0};
    ex.each(n, [&](int i) {
        if (!ex.flag(i)) return;
        double o[4], e1, e2, dz;
        ex.observed(i, o);
        const double X[3] = {ex.state(0, 0, i), ex.state(0, 1, i), ex.state(0, 2, i)};
        ba_errors(K, cur, X, o, e1, e2, dz);
        s1[0] += e1 + e2;
    });
    ex.sum(s1);
    double obj = s1[0], lambda = kLambda0;
    int accepted = 0;

    // 3. Levenberg-Marquardt
    for (int it = 0; it < max_iterations; it++) {
        double b1[3], b2[3];
        ba_tangent(cur.T, b1, b2);
        double acc[20];
#pragma unroll
        for (int k = 0; k < 20; k++) acc[k] = 0.0;
        bool bad = false;
        ex.each(n, [&](int i) {
            if (!ex.flag(i)) return;
            double o[4], Yv[3][5], z[3], a[20];
            ex.observed(i, o);
            const double X[3] = {ex.state(acc_buf, 0, i), ex.state(acc_buf, 1, i), ex.state(acc_buf, 2, i)};
            if (!ba_point_blocks(K, cur, b1, b2, lambda, X, o, Yv, z, a)) bad = true;
#pragma unroll
            for (int k = 0; k < 20; k++) acc[k] += a[k];
        });
        ex.sum(acc);
        bad = ex.any(bad);
        // the reduced system by Cholesky, in every caller: its diagonal is damped already
        double dc[5], diag[5];
#pragma unroll
        for (int k = 0; k < 5; k++) diag[k] = acc[lm_tri<5>(k, k)];
        const bool ok = !bad && lm_chol_solve<5>(acc, diag, dc);
        bool accept = false;
        double obj_new = 0.0;
        LmCam cand;
        if (ok) {   // the same everywhere
            ba_candidate(cur, b1, b2, dc, cand);
            double so[1] = {0};
            bool behind = false;
            ex.each(n, [&](int i) {
                if (!ex.flag(i)) return;
                double o[4], Yv[3][5], z[3], a[20], Xn[3], e1, e2, dz;
                ex.observed(i, o);
                const double X[3] = {ex.state(acc_buf, 0, i), ex.state(acc_buf, 1, i), ex.state(acc_buf, 2, i)};
                ba_point_blocks(K, cur, b1, b2, lambda, X, o, Yv, z, a);
                ba_point_step(X, Yv, z, dc, Xn);
#pragma unroll
                for (int k = 0; k < 3; k++) ex.state(acc_buf ^ 1, k, i) = Xn[k];
                ba_errors(K, cand, Xn, o, e1, e2, dz);
                so[0] += e1 + e2;
                if (!(Xn[2] > 0.0) || !(dz > 0.0)) behind = true;
            });
            ex.sum(so);
            behind = ex.any(behind);
            obj_new = so[0];
            accept = !behind && obj_new < obj;   // false for a NaN objective
        }
        if (accept) {
            const double rel = (obj - obj_new) / obj;
            cur = cand;
            obj = obj_new;
            acc_buf ^= 1;
            accepted++;
            lambda = fmax(lambda / 10.0, kLambdaMin);
            if (rel < kRelStop) break;
        } else {
            lambda = lambda * 10.0;
            if (lambda > kLambdaMax) break;
        }
    }
    if (accepted == 0) return false;

    // 4. one rounding to f32; anything not finite leaves the pair alone
    LmCam outc;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        res.R32[k] = (float)cur.R[k];
        outc.R[k] = (double)res.R32[k];
        finite = finite && std::isfinite(res.R32[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        res.t32[k] = (float)cur.T[k];
        outc.T[k] = (double)res.t32[k];
        finite = finite && std::isfinite(res.t32[k]);
    }
    ba_camera(K, cur, res.c2);
#pragma unroll
    for (int k = 0; k < 12; k++) finite = finite && std::isfinite(res.c2[k]);
    bool nonfinite = !finite;
    double sf[1] = {0};
    ex.each(n, [&](int i) {
        if (!ex.flag(i)) return;
        double o[4], Xf[3], e1, e2, dz;
        ex.observed(i, o);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float x32 = (float)ex.state(acc_buf, k, i);
            if (!std::isfinite(x32)) nonfinite = true;
            Xf[k] = (double)x32;
        }
        ba_errors(K, outc, Xf, o, e1, e2, dz);
        sf[0] += e1 + e2;
    });
    ex.sum(sf);
    if (ex.any(nonfinite)) return false;
    res.cam = cur;
    res.buf = acc_buf;
    res.objective = obj;
    stats[1] = mean_in;
    stats[2] = sf[0] / (2.0 * cnt);
    stats[3] = (double)accepted;
    return true;
}
}  // namespace vs_refine
