// The arithmetic of the two-view bundle adjustment (vslam_refine_pairs, include/vslam_amd.h) that does not know about lanes:
// one point's blocks, the reduced 5 x 5 solve, the candidate camera.  refine.hip runs it on the device; tests/native/refine_serial.cpp
// compiles the same text for the host and walks the points one after the other, which holds the formulas to tests/ref_refine.py
// without a GPU.  All f64, never fused (compile host code with -ffp-contract=off).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define BA_FN __host__ __device__ __forceinline__
#pragma clang fp contract(off)
#else
#define BA_FN inline
#endif

namespace vs_refine {
constexpr double kLambda0 = 1e-3, kLambdaMin = 1e-15, kLambdaMax = 1e12, kRelStop = 0x1p-40, kDiagFloor = 0x1p-40;

struct BaCam {
    double R[9], t[3];
};

// index of (i, j), i <= j, among the 15 unique entries of a symmetric 5 x 5
BA_FN constexpr int ba_tri(int i, int j) { return i * 5 - i * (i - 1) / 2 + (j - i); }

BA_FN void ba_transform(const double (&R)[9], const double (&t)[3], const double (&X)[3], double (&RX)[3],
                                             double (&Y)[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        RX[r] = (R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2];
        Y[r] = RX[r] + t[r];
    }
}

// (u, v) = (q0 / q2, q1 / q2), q = K Y row by row
BA_FN void ba_project(const double (&K)[9], const double (&Y)[3], double &u, double &v, double &q2) {
    const double q0 = (K[0] * Y[0] + K[1] * Y[1]) + K[2] * Y[2];
    const double q1 = (K[3] * Y[0] + K[4] * Y[1]) + K[5] * Y[2];
    q2 = (K[6] * Y[0] + K[7] * Y[1]) + K[8] * Y[2];
    u = q0 / q2;
    v = q1 / q2;
}

// squared reprojection errors of one point in the two images
BA_FN void ba_errors(const double (&K)[9], const BaCam &c, const double (&X)[3], const double (&o)[4], double &e1,
                                          double &e2, double &depth2) {
    double u, v, q2, RX[3], Y[3];
    ba_project(K, X, u, v, q2);
    double du = u - o[0], dv = v - o[1];
    e1 = du * du + dv * dv;
    ba_transform(c.R, c.t, X, RX, Y);
    ba_project(K, Y, u, v, q2);
    du = u - o[2];
    dv = v - o[3];
    e2 = du * du + dv * dv;
    depth2 = Y[2];
}

// A = d (u, v) / d Y = (K_row0 - u K_row2, K_row1 - v K_row2) / q2
BA_FN void ba_dproj(const double (&K)[9], double u, double v, double q2, double (&A)[2][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        A[0][k] = (K[k] - u * K[6 + k]) / q2;
        A[1][k] = (K[3 + k] - v * K[6 + k]) / q2;
    }
}

// One point's blocks at (c, X), damped by lambda: Yv = V*^-1 W^t (3 x 5), z = V*^-1 g_x, and what the point adds to the reduced
// system (acc[0..15): U - W Yv with U's diagonal times (1 + lambda); acc[15..20): g_c - W z).  false when V* has a pivot that is
// not > 0 (the step is then refused).
BA_FN bool ba_point_blocks(const double (&K)[9], const BaCam &c, const double (&b1)[3], const double (&b2)[3],
                                                double lambda, const double (&X)[3], const double (&o)[4], double (&Yv)[3][5],
                                                double (&z)[3], double (&acc)[20]) {
    double u1, v1, q, u2, v2, RX[3], Y[3], A1[2][3], A2[2][3];
    ba_project(K, X, u1, v1, q);
    ba_dproj(K, u1, v1, q, A1);
    ba_transform(c.R, c.t, X, RX, Y);
    ba_project(K, Y, u2, v2, q);
    ba_dproj(K, u2, v2, q, A2);
    const double r1[2] = {u1 - o[0], v1 - o[1]}, r2[2] = {u2 - o[2], v2 - o[3]};
    // J2x = A2 R; Jc = A2 [-[RX]x | b1 | b2]
    double J2x[2][3], Jc[2][5];
#pragma unroll
    for (int r = 0; r < 2; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) J2x[r][k] = (A2[r][0] * c.R[k] + A2[r][1] * c.R[3 + k]) + A2[r][2] * c.R[6 + k];
        Jc[r][0] = A2[r][2] * RX[1] - A2[r][1] * RX[2];
        Jc[r][1] = A2[r][0] * RX[2] - A2[r][2] * RX[0];
        Jc[r][2] = A2[r][1] * RX[0] - A2[r][0] * RX[1];
        Jc[r][3] = (A2[r][0] * b1[0] + A2[r][1] * b1[1]) + A2[r][2] * b1[2];
        Jc[r][4] = (A2[r][0] * b2[0] + A2[r][1] * b2[1]) + A2[r][2] * b2[2];
    }
    double V[3][3], gx[3], W[5][3], gc[5];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = i; j < 3; j++)
            V[i][j] = ((A1[0][i] * A1[0][j] + A1[1][i] * A1[1][j]) + J2x[0][i] * J2x[0][j]) + J2x[1][i] * J2x[1][j];
        gx[i] = ((A1[0][i] * r1[0] + A1[1][i] * r1[1]) + J2x[0][i] * r2[0]) + J2x[1][i] * r2[1];
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int j = 0; j < 3; j++) W[k][j] = Jc[0][k] * J2x[0][j] + Jc[1][k] * J2x[1][j];
        gc[k] = Jc[0][k] * r2[0] + Jc[1][k] * r2[1];
    }
    // Cholesky of V* = V + lambda max(diag V, floor)
    double L[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) V[i][i] = V[i][i] + lambda * fmax(V[i][i], kDiagFloor);
    bool ok = true;
    ok = ok && V[0][0] > 0.0;
    L[0][0] = sqrt(V[0][0]);
    L[1][0] = V[0][1] / L[0][0];
    L[2][0] = V[0][2] / L[0][0];
    const double d1 = V[1][1] - L[1][0] * L[1][0];
    ok = ok && d1 > 0.0;
    L[1][1] = sqrt(d1);
    L[2][1] = (V[1][2] - L[2][0] * L[1][0]) / L[1][1];
    const double d2 = (V[2][2] - L[2][0] * L[2][0]) - L[2][1] * L[2][1];
    ok = ok && d2 > 0.0;
    L[2][2] = sqrt(d2);
    auto solve = [&](double x0, double x1, double x2, double &y0, double &y1, double &y2) {
        const double f0 = x0 / L[0][0];
        const double f1 = (x1 - L[1][0] * f0) / L[1][1];
        const double f2 = ((x2 - L[2][0] * f0) - L[2][1] * f1) / L[2][2];
        y2 = f2 / L[2][2];
        y1 = (f1 - L[2][1] * y2) / L[1][1];
        y0 = ((f0 - L[1][0] * y1) - L[2][0] * y2) / L[0][0];
    };
#pragma unroll
    for (int k = 0; k < 5; k++) solve(W[k][0], W[k][1], W[k][2], Yv[0][k], Yv[1][k], Yv[2][k]);
    solve(gx[0], gx[1], gx[2], z[0], z[1], z[2]);
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int l = k; l < 5; l++) {
            double uu = Jc[0][k] * Jc[0][l] + Jc[1][k] * Jc[1][l];
            if (k == l) uu = uu + lambda * uu;
            acc[ba_tri(k, l)] = uu - ((W[k][0] * Yv[0][l] + W[k][1] * Yv[1][l]) + W[k][2] * Yv[2][l]);
        }
        acc[15 + k] = gc[k] - ((W[k][0] * z[0] + W[k][1] * z[1]) + W[k][2] * z[2]);
    }
    return ok;
}

// b1 = normalize(t x e_k), k the axis of the smallest |t_k| (the lowest on a tie); b2 = t x b1
BA_FN void ba_tangent(const double (&t)[3], double (&b1)[3], double (&b2)[3]) {
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

// out = exp([w]x) R
BA_FN void ba_rotate(const double (&w)[3], const double (&R)[9], double (&out)[9]) {
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    double a, b;
    if (th2 < 0x1p-26) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2), s = sin(0.5 * th);
        a = sin(th) / th;
        b = ((2.0 * s) * s) / th2;
    }
    // E = I + a [w]x + b [w]x^2, [w]x^2 = w w^t - th2 I
    double E[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) E[3 * i + j] = b * (w[i] * w[j] - (i == j ? th2 : 0.0)) + (i == j ? 1.0 : 0.0);
    }
    E[1] = E[1] - a * w[2]; E[2] = E[2] + a * w[1];
    E[3] = E[3] + a * w[2]; E[5] = E[5] - a * w[0];
    E[6] = E[6] - a * w[1]; E[7] = E[7] + a * w[0];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
    }
}

// S dc = -rhs by Cholesky from the 15 + 5 sums; false for a pivot that is not > 0 or a dc that is not finite
BA_FN bool ba_reduced_solve(const double (&acc)[20], double (&dc)[5]) {
    double Lc[5][5];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double d = acc[ba_tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) d = d - Lc[j][k] * Lc[j][k];
        ok = ok && d > 0.0;
        Lc[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 5; i++) {
            double s = acc[ba_tri(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - Lc[i][k] * Lc[j][k];
            Lc[i][j] = s / Lc[j][j];
        }
    }
    double f[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        double s = acc[15 + i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - Lc[i][k] * f[k];
        f[i] = s / Lc[i][i];
    }
#pragma unroll
    for (int i = 4; i >= 0; i--) {
        double s = f[i];
#pragma unroll
        for (int k = 4; k > i; k--) s = s - Lc[k][i] * dc[k];
        dc[i] = s / Lc[i][i];
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        dc[i] = -dc[i];
        ok = ok && std::isfinite(dc[i]);
    }
    return ok;
}

// the candidate camera of a step dc: R' = exp([w]x) R, t' = normalize(t + dc[3] b1 + dc[4] b2)
BA_FN void ba_candidate(const BaCam &cur, const double (&b1)[3], const double (&b2)[3], const double (&dc)[5], BaCam &cand) {
    const double w[3] = {dc[0], dc[1], dc[2]};
    ba_rotate(w, cur.R, cand.R);
    double tt[3];
#pragma unroll
    for (int k = 0; k < 3; k++) tt[k] = (cur.t[k] + dc[3] * b1[k]) + dc[4] * b2[k];
    const double nn = sqrt((tt[0] * tt[0] + tt[1] * tt[1]) + tt[2] * tt[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) cand.t[k] = tt[k] / nn;
}

// a point's step from its blocks: X' = X - (z + Yv dc)
BA_FN void ba_point_step(const double (&X)[3], const double (&Yv)[3][5], const double (&z)[3], const double (&dc)[5], double (&Xn)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double yd = (((Yv[k][0] * dc[0] + Yv[k][1] * dc[1]) + Yv[k][2] * dc[2]) + Yv[k][3] * dc[3]) + Yv[k][4] * dc[4];
        Xn[k] = X[k] - (z[k] + yd);
    }
}

// the start of the iteration: R (3 I - R^t R) / 2, one Newton step of the polar iteration; t / |t|
BA_FN void ba_start(const BaCam &in, double tn, BaCam &cur) {
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            G[3 * i + j] = (i == j ? 3.0 : 0.0) - ((in.R[i] * in.R[j] + in.R[3 + i] * in.R[3 + j]) + in.R[6 + i] * in.R[6 + j]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            cur.R[3 * i + j] = 0.5 * ((in.R[3 * i] * G[j] + in.R[3 * i + 1] * G[3 + j]) + in.R[3 * i + 2] * G[6 + j]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) cur.t[k] = in.t[k] / tn;
}
}  // namespace vs_refine
