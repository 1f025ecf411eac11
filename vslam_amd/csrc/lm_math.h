// What the Levenberg-Marquardt optimizers share (refine_math.h, resect_math.h, adjust_math.h) and that does not know about lanes:
// the schedule's constants, the camera, projection and its derivative, the rotation update and start, the Jacobian's columns,
// the Huber loss, the packed triangle and the two Cholesky solves.  Compiled for the device by the kernels and for the host by
// the serial drivers of tests/native.  All f64, never fused (compile host code with -ffp-contract=off): every expression's
// operand order and parentheses are part of the contract, since the results are compared bit for bit.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define LM_FN __host__ __device__ __forceinline__
#pragma clang fp contract(off)
#else
#define LM_FN inline
#endif

namespace vs_lm {
constexpr double kLambda0 = 1e-3, kLambdaMin = 1e-15, kLambdaMax = 1e12, kRelStop = 0x1p-40, kDiagFloor = 0x1p-40;

struct LmCam {   // Y = R X + T
    double R[9], T[3];
};

// index of (i, j), i <= j, among the N (N + 1) / 2 unique entries of a symmetric N x N, row by row
template <int N>
LM_FN constexpr int lm_tri(int i, int j) {
    return i * N - i * (i - 1) / 2 + (j - i);
}

LM_FN void lm_transform(const double (&R)[9], const double (&t)[3], const double (&X)[3], double (&RX)[3], double (&Y)[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        RX[r] = (R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2];
        Y[r] = RX[r] + t[r];
    }
}

// (u, v) = (q0 / q2, q1 / q2), q = K Y row by row
LM_FN void lm_project(const double (&K)[9], const double (&Y)[3], double &u, double &v, double &q2) {
    const double q0 = (K[0] * Y[0] + K[1] * Y[1]) + K[2] * Y[2];
    const double q1 = (K[3] * Y[0] + K[4] * Y[1]) + K[5] * Y[2];
    q2 = (K[6] * Y[0] + K[7] * Y[1]) + K[8] * Y[2];
    u = q0 / q2;
    v = q1 / q2;
}

// A = d (u, v) / d Y = (K_row0 - u K_row2, K_row1 - v K_row2) / q2
LM_FN void lm_dproj(const double (&K)[9], double u, double v, double q2, double (&A)[2][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        A[0][k] = (K[k] - u * K[6 + k]) / q2;
        A[1][k] = (K[3 + k] - v * K[6 + k]) / q2;
    }
}

// the first three columns of a camera's Jacobian, A (-[RX]x): the rotation update exp([w]x) R at w = 0
template <int M>
LM_FN void lm_jac_rotation(const double (&A)[2][3], const double (&RX)[3], double (&J)[2][M]) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
        J[r][0] = A[r][2] * RX[1] - A[r][1] * RX[2];
        J[r][1] = A[r][0] * RX[2] - A[r][2] * RX[0];
        J[r][2] = A[r][1] * RX[0] - A[r][0] * RX[1];
    }
}

// a point's Jacobian under a camera, A R
LM_FN void lm_jac_point(const double (&A)[2][3], const double (&R)[9], double (&J)[2][3]) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) J[r][k] = (A[r][0] * R[k] + A[r][1] * R[3 + k]) + A[r][2] * R[6 + k];
    }
}

// out = exp([w]x) R
LM_FN void lm_rotate(const double (&w)[3], const double (&R)[9], double (&out)[9]) {
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

// the start of an iteration's R: R (3 I - R^t R) / 2, one Newton step of the polar iteration closer to a rotation
LM_FN void lm_polar_step(const double (&R)[9], double (&out)[9]) {
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) G[3 * i + j] = (i == j ? 3.0 : 0.0) - ((R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[3 * i + j] = 0.5 * ((R[3 * i] * G[j] + R[3 * i + 1] * G[3 + j]) + R[3 * i + 2] * G[6 + j]);
    }
}

LM_FN bool lm_finite(const LmCam &c) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(c.R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(c.T[k]);
    return ok;
}

// Huber: rho(e) = e^2 inside delta, 2 delta e - delta^2 outside; its weight 1 inside and delta / e outside
LM_FN double lm_rho(double e, double delta) { return e <= delta ? e * e : (2.0 * delta) * e - delta * delta; }
LM_FN double lm_weight(double e, double delta) { return e <= delta ? 1.0 : delta / e; }

struct LmPoint {   // one observation (u, v) of a point under one camera
    double RX[3], Y[3], u, v, q2, r[2], e;
};

LM_FN void lm_point(const double (&K)[9], const LmCam &c, const double (&X)[3], const double (&x)[2], LmPoint &o) {
    lm_transform(c.R, c.T, X, o.RX, o.Y);
    lm_project(K, o.Y, o.u, o.v, o.q2);
    o.r[0] = o.u - x[0];
    o.r[1] = o.v - x[1];
    o.e = sqrt(o.r[0] * o.r[0] + o.r[1] * o.r[1]);
}

// A free camera's six unknowns (rotation, translation).  Its start: R a polar step closer to a rotation, t as it is;
// the candidate of a step d: R' = exp([d_0..2]x) R, t' = t + d_3..5
LM_FN void lm_cam_start(const LmCam &in, LmCam &cur) {
    lm_polar_step(in.R, cur.R);
#pragma unroll
    for (int k = 0; k < 3; k++) cur.T[k] = in.T[k];
}

LM_FN void lm_cam_step(const LmCam &cur, const double (&d)[6], LmCam &cand) {
    const double w[3] = {d[0], d[1], d[2]};
    lm_rotate(w, cur.R, cand.R);
#pragma unroll
    for (int k = 0; k < 3; k++) cand.T[k] = cur.T[k] + d[3 + k];
}

// V* = L L^t of a point's 3 x 3 block V (upper 6: 00 01 02 11 12 22), V* = V + lambda max(diag V, floor); ok is false when V*
// has a pivot that is not > 0
struct LmChol3 {
    double l00, l10, l20, l11, l21, l22;
    bool ok;
    LM_FN void solve(const double *b, double *y) const {   // V* y = b
        const double f0 = b[0] / l00;
        const double f1 = (b[1] - l10 * f0) / l11;
        const double f2 = ((b[2] - l20 * f0) - l21 * f1) / l22;
        y[2] = f2 / l22;
        y[1] = (f1 - l21 * y[2]) / l11;
        y[0] = ((f0 - l10 * y[1]) - l20 * y[2]) / l00;
    }
};

LM_FN LmChol3 lm_chol3(const double (&V)[6], double lambda) {
    LmChol3 c;
    const double v00 = V[0] + lambda * fmax(V[0], kDiagFloor), v11 = V[3] + lambda * fmax(V[3], kDiagFloor),
                 v22 = V[5] + lambda * fmax(V[5], kDiagFloor);
    c.ok = v00 > 0.0;
    c.l00 = sqrt(v00);
    c.l10 = V[1] / c.l00;
    c.l20 = V[2] / c.l00;
    const double d1 = v11 - c.l10 * c.l10;
    c.ok = c.ok && d1 > 0.0;
    c.l11 = sqrt(d1);
    c.l21 = (V[4] - c.l20 * c.l10) / c.l11;
    const double d2 = (v22 - c.l20 * c.l20) - c.l21 * c.l21;
    c.ok = c.ok && d2 > 0.0;
    c.l22 = sqrt(d2);
    return c;
}

// H d = -g by Cholesky, H symmetric N x N: acc holds its upper triangle by lm_tri<N> and then g; diag is the diagonal the
// factorisation starts from (the caller's damping: H's own, or H's plus lambda times something).  false for a pivot that is
// not > 0 or a d that is not finite.
template <int N>
LM_FN bool lm_chol_solve(const double (&acc)[N * (N + 1) / 2 + N], const double (&diag)[N], double (&d)[N]) {
    double L[N][N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double p = diag[j];
#pragma unroll
        for (int k = 0; k < j; k++) p = p - L[j][k] * L[j][k];
        ok = ok && p > 0.0;
        L[j][j] = sqrt(p);
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double s = acc[lm_tri<N>(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    double f[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = acc[N * (N + 1) / 2 + i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[i][k] * f[k];
        f[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = f[i];
#pragma unroll
        for (int k = N - 1; k > i; k--) s = s - L[k][i] * d[k];
        d[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        d[i] = -d[i];
        ok = ok && std::isfinite(d[i]);
    }
    return ok;
}
}  // namespace vs_lm
