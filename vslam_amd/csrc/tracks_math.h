// What decides something in the triangulation of a track from all its observations (include/vslam_tracks.h) and does not know
// about lanes: the inverse of K, which observations count, their rays and centres, the parallax test, the linear start, the
// Levenberg-Marquardt refinement of the three unknowns and the point's verdict.  Projection, Jacobian, Huber and the 3 x 3 Cholesky
// are lm_math.h's; GOOD is fuse_math.h's fu_good.  Compiled for the device by tracks.hip and for the host by
// tests/native/tracks_serial.cpp.  All f64, never fused (compile host code with -ffp-contract=off).  A point's rays, centres and
// cameras are formed afresh in every pass over its row: nothing per observation is kept, so nothing spills.
#pragma once

#include <cmath>
#include <cstdint>

#include "fuse_math.h"
#include "lm_math.h"

namespace vs_tracks {
using vs_lm::LmCam;
using vs_lm::LmChol3;
using vs_lm::LmPoint;

enum : int32_t { kTrNoPart = -1, kTrOk = 0, kTrTooFew = 1, kTrLowParallax = 2, kTrDegenerate = 3, kTrBehind = 4, kTrUnsupported = 5, kTrWorse = 6 };

struct TrParams {
    double cos_max, huber, r2;   // r2 = inlier_px * inlier_px, one product
    int32_t iterations, min_good, good10;
};

LM_FN TrParams tr_params(double cos_parallax_max, double huber_px, double inlier_px, int32_t iterations, int32_t min_good, int32_t good10) {
    TrParams p;
    p.cos_max = cos_parallax_max;
    p.huber = huber_px;
    p.r2 = inlier_px * inlier_px;
    p.iterations = iterations;
    p.min_good = min_good;
    p.good10 = good10;
    return p;
}

LM_FN bool tr_params_ok(double cos_parallax_max, double huber_px, double inlier_px, int32_t iterations, int32_t min_good, int32_t good10) {
    return std::isfinite(cos_parallax_max) && cos_parallax_max > -1.0 && cos_parallax_max <= 1.0 && std::isfinite(huber_px) && huber_px > 0.0 &&
           std::isfinite(inlier_px) && inlier_px > 0.0 && iterations >= 0 && iterations <= 64 && min_good >= 2 && good10 >= 0 && good10 <= 10;
}

// Kinv = adj(K) / det(K); false for a determinant that is 0 or not finite or an entry of Kinv that is not finite
LM_FN bool tr_kinv(const double (&K)[9], double (&Ki)[9]) {
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[2] * K[7] - K[1] * K[8], c02 = K[1] * K[5] - K[2] * K[4];
    const double c10 = K[5] * K[6] - K[3] * K[8], c11 = K[0] * K[8] - K[2] * K[6], c12 = K[2] * K[3] - K[0] * K[5];
    const double c20 = K[3] * K[7] - K[4] * K[6], c21 = K[1] * K[6] - K[0] * K[7], c22 = K[0] * K[4] - K[1] * K[3];
    const double det = (K[0] * c00 + K[1] * c10) + K[2] * c20;
    if (!(std::isfinite(det) && det != 0.0)) return false;
    Ki[0] = c00 / det; Ki[1] = c01 / det; Ki[2] = c02 / det;
    Ki[3] = c10 / det; Ki[4] = c11 / det; Ki[5] = c12 / det;
    Ki[6] = c20 / det; Ki[7] = c21 / det; Ki[8] = c22 / det;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(Ki[k]);
    return ok;
}

// an item's rows and cameras: obs_cam / obs_kp [obs_stride], R [cam_stride][9], T [cam_stride][3], xy [cam_stride][kp_stride][2]
struct TrItem {
    const int32_t *cam, *kp;
    const double *R, *T;
    const float *xy;
    int C, kp_stride;
};

// d' = R^t b, b = Kinv (x, y, 1), and nn = d'.d'
LM_FN void tr_ray_raw(const double (&Ki)[9], const LmCam &c, const double (&x)[2], double (&dr)[3], double &nn) {
    double b[3];
#pragma unroll
    for (int r = 0; r < 3; r++) b[r] = (Ki[3 * r] * x[0] + Ki[3 * r + 1] * x[1]) + Ki[3 * r + 2];
#pragma unroll
    for (int k = 0; k < 3; k++) dr[k] = (c.R[k] * b[0] + c.R[3 + k] * b[1]) + c.R[6 + k] * b[2];
    nn = (dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2];
}

// USABLE: the cull's, and a finite ray -- d' finite and d'.d' > 0, which is exactly when d = d' / sqrt(d'.d') is finite.  Loads the
// camera and the widened keypoint; dr and nn as tr_ray_raw leaves them.
LM_FN bool tr_usable(const double (&Ki)[9], const TrItem &it, int o, LmCam &c, double (&x)[2], double (&dr)[3], double &nn) {
    const int cam = it.cam[o], kp = it.kp[o];
    if (!vs_fuse::fu_valid(cam, kp, it.C, it.kp_stride)) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) c.R[k] = it.R[(size_t)cam * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) c.T[k] = it.T[(size_t)cam * 3 + k];
    if (!vs_lm::lm_finite(c)) return false;
    const float fx = it.xy[((size_t)cam * it.kp_stride + kp) * 2], fy = it.xy[((size_t)cam * it.kp_stride + kp) * 2 + 1];
    if (!(std::isfinite(fx) && std::isfinite(fy))) return false;
    x[0] = (double)fx;
    x[1] = (double)fy;
    tr_ray_raw(Ki, c, x, dr, nn);
    return std::isfinite(dr[0]) && std::isfinite(dr[1]) && std::isfinite(dr[2]) && nn > 0.0;
}

LM_FN void tr_unit(const double (&dr)[3], double nn, double (&d)[3]) {
    const double s = sqrt(nn);
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = dr[k] / s;
}

// c = -R^t T
LM_FN void tr_centre(const LmCam &c, double (&cc)[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) cc[r] = -((c.R[r] * c.T[0] + c.R[3 + r] * c.T[1]) + c.R[6 + r] * c.T[2]);
}

LM_FN double tr_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// One pass over the usable observations at X: the cost over those with Y_z > 0, whether one has !(Y_z > 0), the blocks V and g of
// those with Y_z > 0 (vslam_adjust.h's V_o and gx_o, summed in observation order) when `blocks`, and the GOOD count when `good`.
struct TrEval {
    double cost, V[6], g[3];
    bool behind;
    int n_good;
};

LM_FN void tr_eval(const double (&K)[9], const double (&Ki)[9], const TrItem &it, int o0, int o1, const double (&X)[3], const TrParams &p, bool blocks,
                   bool good, TrEval &e) {
    e.cost = 0.0;
    e.behind = false;
    e.n_good = 0;
#pragma unroll
    for (int q = 0; q < 6; q++) e.V[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; q++) e.g[q] = 0.0;
    for (int o = o0; o < o1; o++) {
        LmCam c;
        double x[2], dr[3], nn;
        if (!tr_usable(Ki, it, o, c, x, dr, nn)) continue;
        LmPoint pt;
        vs_lm::lm_point(K, c, X, x, pt);
        if (!(pt.Y[2] > 0.0)) {
            e.behind = true;
            continue;
        }
        e.cost += vs_lm::lm_rho(pt.e, p.huber);
        if (good) e.n_good += std::isfinite(pt.u) && std::isfinite(pt.v) && pt.r[0] * pt.r[0] + pt.r[1] * pt.r[1] <= p.r2 ? 1 : 0;
        if (!blocks) continue;
        double A[2][3], J[2][3];
        vs_lm::lm_dproj(K, pt.u, pt.v, pt.q2, A);
        vs_lm::lm_jac_point(A, c.R, J);
        const double w = vs_lm::lm_weight(pt.e, p.huber);
        int t = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = i; j < 3; j++) {
                e.V[t] += w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
                t++;
            }
            e.g[i] += w * (J[0][i] * pt.r[0] + J[1][i] * pt.r[1]);
        }
    }
}

struct TrResult {
    int32_t status, m, n_good;
    double X[3], cos_parallax, cost_in, cost_out;   // the three of d_info: NaN until the rule that forms them has been reached
};

LM_FN double tr_qnan() { return __builtin_nan(""); }

// One point.  o0, o1: offsets[i], offsets[i + 1]; in: the input row's x, y, z (read before anything is written)
LM_FN void tr_point(const double (&K)[9], const double (&Ki)[9], const TrItem &it, int o0, int o1, int obs_stride, float inx, float iny, float inz,
                    const TrParams &p, TrResult &res) {
    res.status = kTrNoPart;
    res.m = 0;
    res.n_good = 0;
    res.X[0] = res.X[1] = res.X[2] = 0.0;
    res.cos_parallax = res.cost_in = res.cost_out = tr_qnan();
    if (!(o0 >= 0 && o0 < o1 && o1 <= obs_stride)) return;

    // pass 1: m, and j1 = the usable observation whose ray has the smallest dot with the first usable one's (the first on ties)
    double d0[3] = {0.0, 0.0, 0.0}, d1[3] = {0.0, 0.0, 0.0}, best = 0.0;
    int m = 0;
    for (int o = o0; o < o1; o++) {
        LmCam c;
        double x[2], dr[3], nn, d[3];
        if (!tr_usable(Ki, it, o, c, x, dr, nn)) continue;
        tr_unit(dr, nn, d);
        if (m == 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) d0[k] = d[k];
        }
        const double s = tr_dot(d0, d);
        if (m == 0 || s < best) {
            best = s;
#pragma unroll
            for (int k = 0; k < 3; k++) d1[k] = d[k];
        }
        m++;
    }
    res.m = m;
    if (m < 2) {
        res.status = kTrTooFew;
        return;
    }

    // pass 2: cos_parallax = min_j d_j1 . d_j; and the linear start's sums, A = sum (I - d d^t), r = sum (I - d d^t) c
    double cosp = 0.0, A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
    bool first = true;
    for (int o = o0; o < o1; o++) {
        LmCam c;
        double x[2], dr[3], nn, d[3], cc[3];
        if (!tr_usable(Ki, it, o, c, x, dr, nn)) continue;
        tr_unit(dr, nn, d);
        const double s = tr_dot(d1, d);
        if (first || s < cosp) cosp = s;
        first = false;
        tr_centre(c, cc);
        const double M[6] = {1.0 - d[0] * d[0], -(d[0] * d[1]), -(d[0] * d[2]), 1.0 - d[1] * d[1], -(d[1] * d[2]), 1.0 - d[2] * d[2]};
#pragma unroll
        for (int q = 0; q < 6; q++) A[q] += M[q];
        r[0] += (M[0] * cc[0] + M[1] * cc[1]) + M[2] * cc[2];
        r[1] += (M[1] * cc[0] + M[3] * cc[1]) + M[4] * cc[2];
        r[2] += (M[2] * cc[0] + M[4] * cc[1]) + M[5] * cc[2];
    }
    res.cos_parallax = cosp;
    if (!(cosp <= p.cos_max)) {
        res.status = kTrLowParallax;
        return;
    }
    const LmChol3 ch0 = vs_lm::lm_chol3(A, 0.0);
    double X[3];
    ch0.solve(r, X);
    if (!(ch0.ok && std::isfinite(X[0]) && std::isfinite(X[1]) && std::isfinite(X[2]))) {
        res.status = kTrDegenerate;
        return;
    }

    // the refinement: one pass per iteration.  `cur` holds the cost, the blocks and "behind" at X; a refused candidate leaves them
    TrEval cur, cand;
    tr_eval(K, Ki, it, o0, o1, X, p, p.iterations > 0, p.iterations == 0, cur);
    double lambda = vs_lm::kLambda0;
    for (int iter = 0; iter < p.iterations; iter++) {
        const LmChol3 ch = vs_lm::lm_chol3(cur.V, lambda);
        double z[3], Xn[3];
        ch.solve(cur.g, z);
#pragma unroll
        for (int k = 0; k < 3; k++) Xn[k] = X[k] + (-z[k]);
        bool accept = false;
        if (ch.ok && std::isfinite(Xn[0]) && std::isfinite(Xn[1]) && std::isfinite(Xn[2])) {
            tr_eval(K, Ki, it, o0, o1, Xn, p, true, false, cand);
            accept = !cand.behind && cand.cost < cur.cost;   // false for a NaN cost
        }
        if (accept) {
            const double rel = (cur.cost - cand.cost) / cur.cost;
#pragma unroll
            for (int k = 0; k < 3; k++) X[k] = Xn[k];
            cur = cand;
            lambda = fmax(lambda / 10.0, vs_lm::kLambdaMin);
            if (rel < vs_lm::kRelStop) break;
        } else {
            lambda = lambda * 10.0;
            if (lambda > vs_lm::kLambdaMax) break;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) res.X[k] = X[k];
    res.cost_out = cur.cost;

    // the last pass, one walk for both: GOOD at the result (with iterations = 0 the first evaluation has counted it) and the input
    // row's cost; each is a sum of its own in observation order
    const bool in_finite = std::isfinite(inx) && std::isfinite(iny) && std::isfinite(inz), count_good = p.iterations > 0;
    res.n_good = cur.n_good;
    if (in_finite || count_good) {
        const double P[3] = {(double)inx, (double)iny, (double)inz};
        double cost_in = 0.0;
        bool behind_in = false;
        int n_good = 0;
        for (int o = o0; o < o1; o++) {
            LmCam c;
            double x[2], dr[3], nn;
            if (!tr_usable(Ki, it, o, c, x, dr, nn)) continue;
            LmPoint pt;
            if (count_good) {
                vs_lm::lm_point(K, c, X, x, pt);
                n_good += pt.Y[2] > 0.0 && std::isfinite(pt.u) && std::isfinite(pt.v) && pt.r[0] * pt.r[0] + pt.r[1] * pt.r[1] <= p.r2 ? 1 : 0;
            }
            if (in_finite) {
                vs_lm::lm_point(K, c, P, x, pt);
                if (pt.Y[2] > 0.0) cost_in += vs_lm::lm_rho(pt.e, p.huber);
                else behind_in = true;
            }
        }
        if (count_good) res.n_good = n_good;
        if (in_finite) res.cost_in = behind_in ? (double)INFINITY : cost_in;
    }
    if (cur.behind) {
        res.status = kTrBehind;
    } else if (!(res.n_good >= p.min_good && 10 * res.n_good >= p.good10 * m)) {
        res.status = kTrUnsupported;
    } else if (in_finite && std::isfinite(res.cost_in) && res.cost_out > res.cost_in) {
        res.status = kTrWorse;
    } else {
        res.status = kTrOk;
    }
}
}  // namespace vs_tracks
