// The arithmetic of the pose-only adjustment (vslam_resect_poses and the resecting world step, include/vslam_resect.h) that does not
// know about lanes: one correspondence's Jacobian, weight and contributions, the damped 6 x 6 solve, the candidate pose, and the
// rounds of the iteration written over two policies -- where the correspondences come from (Src) and how a sum over them is
// closed (Red).  resect.hip runs it with lane-strided sources and the refit's reduction; tests/native/resect_serial.cpp compiles
// the same text for the host, walks the correspondences one after the other and is held to tests/ref_resect.py without a GPU.
// All f64, never fused (compile host code with -ffp-contract=off).
#pragma once

#include "refine_math.h"

namespace vs_resect {
using vs_refine::kDiagFloor;
using vs_refine::kLambda0;
using vs_refine::kLambdaMax;
using vs_refine::kLambdaMin;
using vs_refine::kRelStop;

struct RsParams {
    int max_iterations, rounds, min_links;
    double huber, gate;
};

struct RsCam {
    double R[9], T[3];
};

// index of (i, j), i <= j, among the 21 unique entries of a symmetric 6 x 6
BA_FN constexpr int rs_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

struct RsPoint {   // one correspondence under one pose
    double RP[3], Y[3], u, v, q2, r[2], e;
};

BA_FN void rs_point(const double (&K)[9], const RsCam &c, const double (&P)[3], const double (&x)[2], RsPoint &o) {
    vs_refine::ba_transform(c.R, c.T, P, o.RP, o.Y);
    vs_refine::ba_project(K, o.Y, o.u, o.v, o.q2);
    o.r[0] = o.u - x[0];
    o.r[1] = o.v - x[1];
    o.e = sqrt(o.r[0] * o.r[0] + o.r[1] * o.r[1]);
}

// rho(e) = e^2 inside delta, 2 delta e - delta^2 outside
BA_FN double rs_rho(double e, double delta) { return e <= delta ? e * e : (2.0 * delta) * e - delta * delta; }

// a participant of a gated round: in front of the gating pose and within gate pixels of its keypoint under it
BA_FN bool rs_gate(const double (&K)[9], const RsCam &g, double gate, const double (&P)[3], const double (&x)[2]) {
    RsPoint o;
    rs_point(K, g, P, x, o);
    return o.Y[2] > 0.0 && o.e <= gate;
}

// what one correspondence adds to H (a[0..21), upper triangle by rs_tri) and to g (a[21..27)) at pose c:
// J = A(Y) [ -[RP]x | I ], w = 1 inside delta and delta / e outside
BA_FN void rs_contribution(const double (&K)[9], const RsCam &c, double delta, const double (&P)[3], const double (&x)[2],
                           double (&a)[27]) {
    RsPoint o;
    rs_point(K, c, P, x, o);
    double A[2][3], J[2][6];
    vs_refine::ba_dproj(K, o.u, o.v, o.q2, A);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        J[r][0] = A[r][2] * o.RP[1] - A[r][1] * o.RP[2];
        J[r][1] = A[r][0] * o.RP[2] - A[r][2] * o.RP[0];
        J[r][2] = A[r][1] * o.RP[0] - A[r][0] * o.RP[1];
        J[r][3] = A[r][0];
        J[r][4] = A[r][1];
        J[r][5] = A[r][2];
    }
    const double w = o.e <= delta ? 1.0 : delta / o.e;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = i; j < 6; j++) a[rs_tri(i, j)] = w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
        a[21 + i] = w * (J[0][i] * o.r[0] + J[1][i] * o.r[1]);
    }
}

// (H + lambda max(diag H, floor)) d = -g by Cholesky from the 21 + 6 sums; false for a pivot that is not > 0 or a d that is
// not finite
BA_FN bool rs_solve(const double (&acc)[27], double lambda, double (&d)[6]) {
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double h = acc[rs_tri(j, j)];
        double p = h + lambda * fmax(h, kDiagFloor);
#pragma unroll
        for (int k = 0; k < j; k++) p = p - L[j][k] * L[j][k];
        ok = ok && p > 0.0;
        L[j][j] = sqrt(p);
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = acc[rs_tri(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    double f[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = acc[21 + i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[i][k] * f[k];
        f[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = f[i];
#pragma unroll
        for (int k = 5; k > i; k--) s = s - L[k][i] * d[k];
        d[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        d[i] = -d[i];
        ok = ok && std::isfinite(d[i]);
    }
    return ok;
}

// the candidate of a step d: R' = exp([d_0..2]x) R as the refinement forms it, T' = T + d_3..5
BA_FN void rs_candidate(const RsCam &cur, const double (&d)[6], RsCam &cand) {
    const double w[3] = {d[0], d[1], d[2]};
    vs_refine::ba_rotate(w, cur.R, cand.R);
#pragma unroll
    for (int k = 0; k < 3; k++) cand.T[k] = cur.T[k] + d[3 + k];
}

// the start: R (3 I - R^t R) / 2, the refinement's; T as it is
BA_FN void rs_start(const RsCam &in, RsCam &cur) {
    vs_refine::BaCam a, b;
#pragma unroll
    for (int k = 0; k < 9; k++) a.R[k] = in.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) a.t[k] = in.T[k];
    vs_refine::ba_start(a, 1.0, b);
#pragma unroll
    for (int k = 0; k < 9; k++) cur.R[k] = b.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) cur.T[k] = in.T[k];
}

BA_FN bool rs_finite(const RsCam &c) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(c.R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(c.T[k]);
    return ok;
}

// The rounds of the adjustment.  Src::each(f) calls f(P, x) for the correspondences this caller owns (all of them on the host;
// items l, l + 256, ... for lane l); Red::sum closes N partial sums over all callers and Red::any a flag, the same value everywhere
// afterwards, so every decision below is taken alike by every lane.  Returns true with the result in `out` when the pose moved,
// false when the item is left alone; stats as include/vslam_resect.h states them.
template <class Src, class Red>
BA_FN bool rs_run(const double (&K)[9], const RsCam &in, const RsParams &p, Src &src, Red &red, RsCam &out, double (&stats)[4]) {
    const double qnan = __builtin_nan("");
    stats[1] = stats[2] = stats[3] = qnan;
    double c1[1] = {0.0};
    bool bad = false;
    src.each([&](const double(&P)[3], const double(&x)[2]) {
        c1[0] += 1.0;
        bad = bad || !(std::isfinite(P[0]) && std::isfinite(P[1]) && std::isfinite(P[2]) && std::isfinite(x[0]) && std::isfinite(x[1]));
    });
    red.sum(c1);
    bad = red.any(bad);
    stats[0] = c1[0];
    bool kfin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) kfin = kfin && std::isfinite(K[k]);
    if (c1[0] < (double)p.min_links || bad || !kfin || !rs_finite(in)) return false;

    RsCam start, cur, gcam;
    rs_start(in, start);
    cur = start;
    gcam = start;
    bool gated = false;
    int accepted = 0;
    for (int round = 0; round < p.rounds; round++) {
        // this round's participants and the objective over them at the current pose
        const bool g = round > 0;
        double co[2] = {0.0, 0.0};
        src.each([&](const double(&P)[3], const double(&x)[2]) {
            RsPoint o;
            rs_point(K, cur, P, x, o);
            if (g && !(o.Y[2] > 0.0 && o.e <= p.gate)) return;
            co[0] += 1.0;
            co[1] += rs_rho(o.e, p.huber);
        });
        red.sum(co);
        if (g) {
            if (co[0] < (double)p.min_links) break;   // the previous round's result stands
            gcam = cur;
            gated = true;
        }
        stats[0] = co[0];
        double obj = co[1], lambda = kLambda0;
        for (int it = 0; it < p.max_iterations; it++) {
            double acc[27];
#pragma unroll
            for (int k = 0; k < 27; k++) acc[k] = 0.0;
            src.each([&](const double(&P)[3], const double(&x)[2]) {
                if (gated && !rs_gate(K, gcam, p.gate, P, x)) return;
                double a[27];
                rs_contribution(K, cur, p.huber, P, x, a);
#pragma unroll
                for (int k = 0; k < 27; k++) acc[k] += a[k];
            });
            red.sum(acc);
            double d[6];
            bool accept = false;
            double obj_new = 0.0;
            RsCam cand;
            if (rs_solve(acc, lambda, d)) {   // the same everywhere
                rs_candidate(cur, d, cand);
                double so[1] = {0.0};
                bool behind = false;
                src.each([&](const double(&P)[3], const double(&x)[2]) {
                    if (gated && !rs_gate(K, gcam, p.gate, P, x)) return;
                    RsPoint o;
                    rs_point(K, cand, P, x, o);
                    so[0] += rs_rho(o.e, p.huber);
                    behind = behind || !(o.Y[2] > 0.0);
                });
                red.sum(so);
                behind = red.any(behind);
                obj_new = so[0];
                accept = !behind && obj_new < obj;   // false for a NaN objective
            }
            if (accept) {
                const double rel = (obj - obj_new) / obj;
                cur = cand;
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
    if (accepted == 0 || !rs_finite(cur)) return false;
    // mean rho under the start and under the result over the last round's participants
    double sf[2] = {0.0, 0.0};
    src.each([&](const double(&P)[3], const double(&x)[2]) {
        if (gated && !rs_gate(K, gcam, p.gate, P, x)) return;
        RsPoint o;
        rs_point(K, start, P, x, o);
        sf[0] += rs_rho(o.e, p.huber);
        rs_point(K, cur, P, x, o);
        sf[1] += rs_rho(o.e, p.huber);
    });
    red.sum(sf);
    stats[1] = sf[0] / stats[0];
    stats[2] = sf[1] / stats[0];
    stats[3] = (double)accepted;
    if (!(std::isfinite(stats[1]) && std::isfinite(stats[2]))) {
        stats[1] = stats[2] = stats[3] = qnan;
        return false;
    }
    out = cur;
    return true;
}
}  // namespace vs_resect
