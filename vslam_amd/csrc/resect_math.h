// The arithmetic of the pose-only adjustment (vslam_resect_poses and the resecting world step, include/vslam_resect.h) that does not
// know about lanes: one correspondence's contributions, the damping of the 6 x 6 solve, and the rounds of the iteration written
// over two policies -- where the correspondences come from (Src) and how a sum over them is closed (Red).  The camera, its
// start and candidate, the Jacobian's pieces and the solve itself are lm_math.h's.  resect.hip runs it with lane-strided sources
// and block_reduce.h; tests/native/resect_serial.cpp compiles the same text for the host, walks the correspondences one after the
// other and is held to tests/ref_resect.py without a GPU.  All f64, never fused (compile host code with -ffp-contract=off).
#pragma once

#include "lm_math.h"

namespace vs_resect {
using namespace vs_lm;
using RsCam = LmCam;   // the pose Y = R P + T, under the name the resection's callers have for it

struct RsParams {
    int max_iterations, rounds, min_links;
    double huber, gate;
};

// a participant of a gated round: in front of the gating pose and within gate pixels of its keypoint under it
LM_FN bool rs_gate(const double (&K)[9], const LmCam &g, double gate, const double (&P)[3], const double (&x)[2]) {
    LmPoint o;
    lm_point(K, g, P, x, o);
    return o.Y[2] > 0.0 && o.e <= gate;
}

// what one correspondence adds to H (a[0..21), upper triangle by lm_tri<6>) and to g (a[21..27)) at pose c:
// J = A(Y) [ -[RP]x | I ], w the Huber weight
LM_FN void rs_contribution(const double (&K)[9], const LmCam &c, double delta, const double (&P)[3], const double (&x)[2],
                           double (&a)[27]) {
    LmPoint o;
    lm_point(K, c, P, x, o);
    double A[2][3], J[2][6];
    lm_dproj(K, o.u, o.v, o.q2, A);
    lm_jac_rotation(A, o.RX, J);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        J[r][3] = A[r][0];
        J[r][4] = A[r][1];
        J[r][5] = A[r][2];
    }
    const double w = lm_weight(o.e, delta);
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = i; j < 6; j++) a[lm_tri<6>(i, j)] = w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
        a[21 + i] = w * (J[0][i] * o.r[0] + J[1][i] * o.r[1]);
    }
}

// (H + lambda max(diag H, floor)) d = -g from the 21 + 6 sums; false for a pivot that is not > 0 or a d that is not finite
LM_FN bool rs_solve(const double (&acc)[27], double lambda, double (&d)[6]) {
    double diag[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double h = acc[lm_tri<6>(j, j)];
        diag[j] = h + lambda * fmax(h, kDiagFloor);
    }
    return lm_chol_solve<6>(acc, diag, d);
}

// The rounds of the adjustment.  Src::each(f) calls f(P, x) for the correspondences this caller owns (all of them on the host;
// items l, l + 256, ... for lane l); Red::sum closes N partial sums over all callers and Red::any a flag, the same value everywhere
// afterwards, so every decision below is taken alike by every lane.  Returns true with the result in `out` when the pose moved,
// false when the item is left alone; stats as include/vslam_resect.h states them.
template <class Src, class Red>
LM_FN bool rs_run(const double (&K)[9], const LmCam &in, const RsParams &p, Src &src, Red &red, LmCam &out, double (&stats)[4]) {
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
    if (c1[0] < (double)p.min_links || bad || !kfin || !lm_finite(in)) return false;

    LmCam start, cur, gcam;
    lm_cam_start(in, start);
    cur = start;
    gcam = start;
    bool gated = false;
    int accepted = 0;
    for (int round = 0; round < p.rounds; round++) {
        // this round's participants and the objective over them at the current pose
        const bool g = round > 0;
        double co[2] = {0.0, 0.0};
        src.each([&](const double(&P)[3], const double(&x)[2]) {
            LmPoint o;
            lm_point(K, cur, P, x, o);
            if (g && !(o.Y[2] > 0.0 && o.e <= p.gate)) return;
            co[0] += 1.0;
            co[1] += lm_rho(o.e, p.huber);
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
            LmCam cand;
            if (rs_solve(acc, lambda, d)) {   // the same everywhere
                lm_cam_step(cur, d, cand);
                double so[1] = {0.0};
                bool behind = false;
                src.each([&](const double(&P)[3], const double(&x)[2]) {
                    if (gated && !rs_gate(K, gcam, p.gate, P, x)) return;
                    LmPoint o;
                    lm_point(K, cand, P, x, o);
                    so[0] += lm_rho(o.e, p.huber);
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
    if (accepted == 0 || !lm_finite(cur)) return false;
    // mean rho under the start and under the result over the last round's participants
    double sf[2] = {0.0, 0.0};
    src.each([&](const double(&P)[3], const double(&x)[2]) {
        if (gated && !rs_gate(K, gcam, p.gate, P, x)) return;
        LmPoint o;
        lm_point(K, start, P, x, o);
        sf[0] += lm_rho(o.e, p.huber);
        lm_point(K, cur, P, x, o);
        sf[1] += lm_rho(o.e, p.huber);
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
