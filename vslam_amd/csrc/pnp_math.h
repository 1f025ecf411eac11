// The arithmetic of the pose without a prior (vslam_pnp_ransac, include/vslam_pnp.h) that does not know about lanes: the integer
// sampler, the minimal solver (P3P: a quartic in a ratio of two distances, closed by Ferrari's method on a cubic root found by a
// capped Newton iteration, then an absolute orientation from two orthonormal frames), the inlier test and the winner's key.
// pnp.hip compiles it for the device; tests/native/pnp_serial.cpp compiles the same text for the host, walks hypotheses and
// correspondences one after the other and is held to tests/ref_pnp.py without a GPU.  All f64, never fused (compile host code
// with -ffp-contract=off), only + - * / sqrt: every expression's operand order and parentheses are part of the contract, since
// the counts are compared bit for bit.
#pragma once

#include <cstdint>

#include "lm_math.h"

namespace vs_pnp {
using namespace vs_lm;

constexpr int kPnDraws = 16;           // draws per hypothesis
constexpr int kPnNewton = 64;          // cap of the Newton iteration on the resolvent cubic
constexpr int kPnRootSteps = 6;        // Newton steps on the quartic itself behind Ferrari's closed form
constexpr double kPnRotTol = 1e-9;     // max |R^t R - I| of a solution that is kept
constexpr int kPnMaxPoses = 4096;      // 4 x the largest hypotheses (1024): the key's low 12 bits

LM_FN uint32_t pn_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

// three distinct indices below n for hypothesis h, or false: draw c is mix(mix(seed ^ (0x9e3779b9 (h + 1))) + c), its index
// ((u64) r n) >> 32; a draw that repeats an index is skipped; at most kPnDraws draws
LM_FN bool pn_sample(uint32_t seed, int h, int n, int &i0, int &i1, int &i2) {
    i0 = i1 = i2 = -1;
    if (n < 3) return false;
    const uint32_t base = pn_mix(seed ^ (0x9e3779b9u * (uint32_t)(h + 1)));
    int got = 0;
    for (int c = 0; c < kPnDraws && got < 3; c++) {
        const uint32_t r = pn_mix(base + (uint32_t)c);
        const int i = (int)(((uint64_t)r * (uint64_t)(uint32_t)n) >> 32);
        if (i == i0 || i == i1) continue;
        if (got == 0) i0 = i;
        else if (got == 1) i1 = i;
        else i2 = i;
        got++;
    }
    return got == 3;
}

// K^-1 by the adjugate; non-finite for a singular K, which leaves every hypothesis without a pose
LM_FN void pn_kinv(const double (&K)[9], double (&inv)[9]) {
    double a[9];
    a[0] = K[4] * K[8] - K[5] * K[7];
    a[1] = K[2] * K[7] - K[1] * K[8];
    a[2] = K[1] * K[5] - K[2] * K[4];
    a[3] = K[5] * K[6] - K[3] * K[8];
    a[4] = K[0] * K[8] - K[2] * K[6];
    a[5] = K[2] * K[3] - K[0] * K[5];
    a[6] = K[3] * K[7] - K[4] * K[6];
    a[7] = K[1] * K[6] - K[0] * K[7];
    a[8] = K[0] * K[4] - K[1] * K[3];
    const double det = (K[0] * a[0] + K[1] * a[3]) + K[2] * a[6];
#pragma unroll
    for (int k = 0; k < 9; k++) inv[k] = a[k] / det;
}

// the unit bearing of pixel x: K^-1 (x, y, 1), normalised
LM_FN void pn_bearing(const double (&inv)[9], const double (&x)[2], double (&f)[3]) {
    double m[3];
#pragma unroll
    for (int r = 0; r < 3; r++) m[r] = (inv[3 * r] * x[0] + inv[3 * r + 1] * x[1]) + inv[3 * r + 2];
    const double nrm = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) f[r] = m[r] / nrm;
}

LM_FN double pn_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

LM_FN double pn_dist2(const double (&a)[3], const double (&b)[3]) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// The real roots of c[4] v^4 + c[3] v^3 + c[2] v^2 + c[1] v + c[0] in four fixed slots.  Monic and depressed (v = y - B / 4:
// y^4 + p y^2 + q y + r); m = a real root >= 0 of the resolvent m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8, which is <= 0 at 0 and
// > 0 at Cauchy's bound: Newton from the bound, kept inside the bracket [lo, hi] of the sign change (a step that leaves it is
// replaced by the midpoint), ended when a step no longer moves m and after kPnNewton steps at the latest; with s = sqrt(2 m), t =
// q / (2 s), h = p / 2 + m the quartic is (y^2 - s y + h + t)(y^2 + s y + h - t): slots 0, 1 the first factor's roots (smaller
// first), slots 2, 3 the second's.  A quartic whose m is not > 0 (q = 0), or with c[4] = 0, has no root here.
LM_FN void pn_quartic(const double (&c)[5], double (&v)[4], bool (&has)[4]) {
    const double B = c[3] / c[4], C = c[2] / c[4], D = c[1] / c[4], E = c[0] / c[4];
    const double B2 = B * B;
    const double p = C - (3.0 * B2) / 8.0;
    const double q = (D - (B * C) / 2.0) + (B2 * B) / 8.0;
    const double r = ((E - (B * D) / 4.0) + (B2 * C) / 16.0) - (3.0 * (B2 * B2)) / 256.0;
    const double k2 = p, k1 = (p * p) / 4.0 - r, k0 = -((q * q) / 8.0);
    double lo = 0.0, hi = 1.0 + fmax(fmax(fabs(k2), fabs(k1)), fabs(k0)), m = hi;
    for (int it = 0; it < kPnNewton; it++) {
        const double f = ((m + k2) * m + k1) * m + k0;
        const double fp = (3.0 * m + 2.0 * k2) * m + k1;
        if (f > 0.0) hi = m;
        else lo = m;
        double mn = m - f / fp;
        if (!(mn > lo && mn < hi)) mn = 0.5 * (lo + hi);
        if (mn == m) break;
        m = mn;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        has[k] = false;
        v[k] = 0.0;
    }
    if (!(m > 0.0) || !std::isfinite(m)) return;
    const double s = sqrt(2.0 * m), t = q / (2.0 * s), h = p / 2.0 + m, shift = B / 4.0;
    const double disc1 = s * s - 4.0 * (h + t), disc2 = s * s - 4.0 * (h - t);
    if (disc1 >= 0.0) {
        const double w = sqrt(disc1);
        v[0] = (s - w) / 2.0 - shift;
        v[1] = (s + w) / 2.0 - shift;
        has[0] = has[1] = true;
    }
    if (disc2 >= 0.0) {
        const double w = sqrt(disc2);
        v[2] = (-s - w) / 2.0 - shift;
        v[3] = (-s + w) / 2.0 - shift;
        has[2] = has[3] = true;
    }
    // the closed form loses digits where s - w or h +- t cancel: kPnRootSteps Newton steps on the quartic itself; a step that is
    // not finite is not taken
#pragma unroll
    for (int k = 0; k < 4; k++) {
        for (int it = 0; it < kPnRootSteps; it++) {
            const double x = v[k];
            const double f = (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0];
            const double fp = ((4.0 * c[4] * x + 3.0 * c[3]) * x + 2.0 * c[2]) * x + c[1];
            const double xn = x - f / fp;
            if (std::isfinite(xn)) v[k] = xn;
        }
    }
}

// the orthonormal frame of three points as columns e1 e2 e3: e1 along B - A, e3 along e1 x (C - A), e2 = e3 x e1
LM_FN void pn_frame(const double (&A)[3], const double (&B)[3], const double (&C)[3], double (&e)[3][3]) {
    double ab[3], ac[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ab[k] = B[k] - A[k];
        ac[k] = C[k] - A[k];
    }
    const double n1 = sqrt(pn_dot(ab, ab));
#pragma unroll
    for (int k = 0; k < 3; k++) e[0][k] = ab[k] / n1;
    double w[3];
    w[0] = e[0][1] * ac[2] - e[0][2] * ac[1];
    w[1] = e[0][2] * ac[0] - e[0][0] * ac[2];
    w[2] = e[0][0] * ac[1] - e[0][1] * ac[0];
    const double n3 = sqrt(pn_dot(w, w));
#pragma unroll
    for (int k = 0; k < 3; k++) e[2][k] = w[k] / n3;
    e[1][0] = e[2][1] * e[0][2] - e[2][2] * e[0][1];
    e[1][1] = e[2][2] * e[0][0] - e[2][0] * e[0][2];
    e[1][2] = e[2][0] * e[0][1] - e[2][1] * e[0][0];
}

// P3P.  Points P[0..2], unit bearings f[0..2]; distances s_i along the bearings with |s_i f_i - s_j f_j| = |P_i - P_j|.  With
// s_1 = u s_0, s_2 = v s_0, A = |P1 - P2|^2 / |P0 - P2|^2, C = |P0 - P1|^2 / |P0 - P2|^2, ca = f1.f2, cb = f0.f2, cg = f0.f1 the
// two law-of-cosines ratios are quadratics in u,
//     u^2 + p1 u + p0 = 0,   p1 = -2 ca v,   p0 = (1 - A) v^2 + 2 A cb v - A
//     u^2 + q1 u + q0 = 0,   q1 = -2 cg,     q0 = -C v^2 + 2 C cb v + (1 - C)
// whose resultant (q0 - p0)^2 - (q1 - p1)(p1 q0 - p0 q1) is the quartic in v, and u = -(q0 - p0) / (q1 - p1).  s_0 =
// sqrt(|P0 - P2|^2 / ((1 + v v) - (2 v) cb)).  A solution is kept iff u, v and the three distances are finite and > 0, the pose
// is finite and max |R^t R - I| <= kPnRotTol.  The pose: R = Ec Ew^t from the frames of (s_i f_i) and (P_i), T = s_0 f_0 - R P_0.
// Collinear or repeated points divide by zero in a frame, so they have no solution.  Solution slot k is the quartic's slot k.
LM_FN void pn_p3p(const double (&P)[3][3], const double (&f)[3][3], LmCam (&cam)[4], bool (&ok)[4]) {
    const double A2 = pn_dist2(P[1], P[2]), B2 = pn_dist2(P[0], P[2]), C2 = pn_dist2(P[0], P[1]);
    const double ca = pn_dot(f[1], f[2]), cb = pn_dot(f[0], f[2]), cg = pn_dot(f[0], f[1]);
    const double A = A2 / B2, C = C2 / B2;
    const double p02 = 1.0 - A, p01 = (2.0 * A) * cb, p00 = -A;
    const double q02 = -C, q01 = (2.0 * C) * cb, q00 = 1.0 - C;
    const double d2 = q02 - p02, d1 = q01 - p01, d0 = q00 - p00;
    const double e1 = 2.0 * ca, e0 = -(2.0 * cg);
    const double g3 = -(e1 * q02);
    const double g2 = (2.0 * cg) * p02 - e1 * q01;
    const double g1 = (2.0 * cg) * p01 - e1 * q00;
    const double g0 = (2.0 * cg) * p00;
    double c[5];
    c[4] = d2 * d2 - e1 * g3;
    c[3] = (2.0 * d2) * d1 - (e1 * g2 + e0 * g3);
    c[2] = ((2.0 * d2) * d0 + d1 * d1) - (e1 * g1 + e0 * g2);
    c[1] = (2.0 * d1) * d0 - (e1 * g0 + e0 * g1);
    c[0] = d0 * d0 - e0 * g0;
    double v[4];
    bool has[4];
    pn_quartic(c, v, has);
    double Ew[3][3];
    pn_frame(P[0], P[1], P[2], Ew);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double vv = v[k];
        const double u = -(((d2 * vv + d1) * vv + d0) / (e1 * vv + e0));
        const double s0 = sqrt(B2 / ((1.0 + vv * vv) - (2.0 * vv) * cb));
        const double s1 = u * s0, s2 = vv * s0;
        bool good = has[k] && std::isfinite(u) && std::isfinite(vv) && u > 0.0 && vv > 0.0 && std::isfinite(s0) && std::isfinite(s1) &&
                    std::isfinite(s2) && s0 > 0.0 && s1 > 0.0 && s2 > 0.0;
        double Y[3][3], Ec[3][3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Y[0][j] = s0 * f[0][j];
            Y[1][j] = s1 * f[1][j];
            Y[2][j] = s2 * f[2][j];
        }
        pn_frame(Y[0], Y[1], Y[2], Ec);
        LmCam &o = cam[k];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) o.R[3 * i + j] = (Ec[0][i] * Ew[0][j] + Ec[1][i] * Ew[1][j]) + Ec[2][i] * Ew[2][j];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) o.T[i] = Y[0][i] - ((o.R[3 * i] * P[0][0] + o.R[3 * i + 1] * P[0][1]) + o.R[3 * i + 2] * P[0][2]);
        good = good && lm_finite(o);
        double worst = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = i; j < 3; j++) {
                const double gij = (o.R[i] * o.R[j] + o.R[3 + i] * o.R[3 + j]) + o.R[6 + i] * o.R[6 + j];
                worst = fmax(worst, fabs(gij - (i == j ? 1.0 : 0.0)));
            }
        }
        ok[k] = good && worst <= kPnRotTol;
    }
}

// The poses of hypothesis h of an item with n correspondences: at(i, P, x) fetches correspondence i (x widened).  No pose
// without three distinct indices.
template <class At>
LM_FN void pn_hypothesis(const double (&Kinv)[9], uint32_t seed, int h, int n, At at, LmCam (&cam)[4], bool (&ok)[4]) {
    int i0, i1, i2;
#pragma unroll
    for (int k = 0; k < 4; k++) ok[k] = false;
    if (!pn_sample(seed, h, n, i0, i1, i2)) return;
    double P[3][3], x[2], f[3][3];
    at(i0, P[0], x);
    pn_bearing(Kinv, x, f[0]);
    at(i1, P[1], x);
    pn_bearing(Kinv, x, f[1]);
    at(i2, P[2], x);
    pn_bearing(Kinv, x, f[2]);
    pn_p3p(P, f, cam, ok);
}

// correspondence (P, x) is an inlier of the pose: in front of it, a finite projection, inside the closed disc thr2 = px px
LM_FN bool pn_inlier(const double (&K)[9], const LmCam &c, const double (&P)[3], const double (&x)[2], double thr2) {
    double RX[3], Y[3], u, v, q2;
    lm_transform(c.R, c.T, P, RX, Y);
    lm_project(K, Y, u, v, q2);
    const double r0 = u - x[0], r1 = v - x[1];
    return Y[2] > 0.0 && std::isfinite(u) && std::isfinite(v) && r0 * r0 + r1 * r1 <= thr2;
}

LM_FN bool pn_finite_row(const double (&P)[3], const double (&x)[2]) {
    return std::isfinite(P[0]) && std::isfinite(P[1]) && std::isfinite(P[2]) && std::isfinite(x[0]) && std::isfinite(x[1]);
}

// one order-free maximum: the larger count wins, then the smaller pose index 4 h + s; 0 where there is no pose
LM_FN uint32_t pn_key(int count, int pose) { return count < 0 ? 0u : ((uint32_t)count << 12) | (uint32_t)(kPnMaxPoses - 1 - pose); }
LM_FN int pn_key_count(uint32_t key) { return (int)(key >> 12); }
LM_FN int pn_key_pose(uint32_t key) { return kPnMaxPoses - 1 - (int)(key & (kPnMaxPoses - 1)); }
}  // namespace vs_pnp
