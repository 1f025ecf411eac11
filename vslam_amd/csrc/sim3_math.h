// The arithmetic of the similarity between two views (vslam_sim3_ransac / vslam_sim3_refine, include/vslam_sim3.h) that does not know
// about lanes: the 3-point model with its two projection matrices, the division-free inlier test, the winner's key, and the rounds
// of the 7-parameter polish written over two policies (where the correspondences come from, how a sum is closed) as
// resect_math.h's are.  The sampler and the frame of three points are pnp_math.h's, by inclusion.  sim3.hip compiles it for the
// device; tests/native/sim3_serial.cpp compiles the same text for the host and is held to tests/ref_sim3.py without a GPU.  All
// f64, never fused (compile host code with -ffp-contract=off): operand order and parentheses are part of the contract.
#pragma once

#include "pnp_math.h"
#include "resect_math.h"

namespace vs_sim3 {
using namespace vs_pnp;
using vs_resect::RsParams;

constexpr double kS3RotTol = 1e-9;   // max |R^t R - I| of a model that is kept
constexpr int kS3MaxHyp = 1024;      // the key's low 10 bits
constexpr int kS3Sums = 35;          // H (28) and g (7)

struct S3Model {   // B = s R A + t
    double s, R[9], t[3];
};

struct S3Proj {   // Ma = K [R^t / s | -(R^t t) / s], Mb = K [s R | t], row-major 3 x 4
    double Ma[12], Mb[12];
};

// K [L | c] for a 3 x 3 L (row-major) and a column c
LM_FN void s3_kmul(const double (&K)[9], const double (&L)[9], const double (&c)[3], double (&M)[12]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int j = 0; j < 3; j++) M[4 * r + j] = (K[3 * r] * L[j] + K[3 * r + 1] * L[3 + j]) + K[3 * r + 2] * L[6 + j];
        M[4 * r + 3] = (K[3 * r] * c[0] + K[3 * r + 1] * c[1]) + K[3 * r + 2] * c[2];
    }
}

LM_FN void s3_proj(const double (&K)[9], const S3Model &m, S3Proj &p) {
    double L[9], u[3];
#pragma unroll
    for (int k = 0; k < 9; k++) L[k] = m.s * m.R[k];
    s3_kmul(K, L, m.t, p.Mb);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) L[3 * i + j] = m.R[3 * j + i] / m.s;
        u[i] = -(((m.R[i] * m.t[0] + m.R[3 + i] * m.t[1]) + m.R[6 + i] * m.t[2]) / m.s);
    }
    s3_kmul(K, L, u, p.Ma);
}

// the model of three pairs in sampling order and whether it is kept
LM_FN bool s3_model(const double (&K)[9], const double (&A)[3][3], const double (&B)[3][3], S3Model &m, S3Proj &p) {
    double cA[3], cB[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        cA[k] = ((A[0][k] + A[1][k]) + A[2][k]) / 3.0;
        cB[k] = ((B[0][k] + B[1][k]) + B[2][k]) / 3.0;
    }
    const double sa = (pn_dist2(A[0], cA) + pn_dist2(A[1], cA)) + pn_dist2(A[2], cA);
    const double sb = (pn_dist2(B[0], cB) + pn_dist2(B[1], cB)) + pn_dist2(B[2], cB);
    m.s = sqrt(sb / sa);
    double FA[3][3], FB[3][3];
    pn_frame(A[0], A[1], A[2], FA);
    pn_frame(B[0], B[1], B[2], FB);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) m.R[3 * i + j] = (FB[0][i] * FA[0][j] + FB[1][i] * FA[1][j]) + FB[2][i] * FA[2][j];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) m.t[r] = cB[r] - m.s * ((m.R[3 * r] * cA[0] + m.R[3 * r + 1] * cA[1]) + m.R[3 * r + 2] * cA[2]);
    s3_proj(K, m, p);
    bool good = std::isfinite(m.s) && m.s > 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) good = good && std::isfinite(m.R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) good = good && std::isfinite(m.t[k]);
#pragma unroll
    for (int k = 0; k < 12; k++) good = good && std::isfinite(p.Ma[k]) && std::isfinite(p.Mb[k]);
    double worst = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = i; j < 3; j++) {
            const double gij = (m.R[i] * m.R[j] + m.R[3 + i] * m.R[3 + j]) + m.R[6 + i] * m.R[6 + j];
            worst = fmax(worst, fabs(gij - (i == j ? 1.0 : 0.0)));
        }
    }
    return good && worst <= kS3RotTol;
}

// The model of hypothesis h of an item with n correspondences: at(i, A, B) fetches the two points of correspondence i.
template <class At>
LM_FN bool s3_hypothesis(const double (&K)[9], uint32_t seed, int h, int n, At at, S3Model &m, S3Proj &p) {
    int i0, i1, i2;
    if (!pn_sample(seed, h, n, i0, i1, i2)) return false;
    double A[3][3], B[3][3];
    at(i0, A[0], B[0]);
    at(i1, A[1], B[1]);
    at(i2, A[2], B[2]);
    return s3_model(K, A, B, m, p);
}

// (X, x) passes under the 3 x 4 matrix M: in front, inside the closed disc of px pixels, without a division
LM_FN bool s3_pass(const double (&M)[12], const double (&X)[3], const double (&x)[2], double px) {
    const double q0 = ((M[0] * X[0] + M[1] * X[1]) + M[2] * X[2]) + M[3];
    const double q1 = ((M[4] * X[0] + M[5] * X[1]) + M[6] * X[2]) + M[7];
    const double q2 = ((M[8] * X[0] + M[9] * X[1]) + M[10] * X[2]) + M[11];
    const double d0 = q0 - x[0] * q2, d1 = q1 - x[1] * q2, l = px * q2;
    const double ll = l * l;
    return q2 > 0.0 && d0 * d0 + d1 * d1 <= ll && std::isfinite(ll);
}

LM_FN bool s3_inlier(const S3Proj &p, const double (&A)[3], const double (&xa)[2], const double (&B)[3], const double (&xb)[2], double px) {
    return s3_pass(p.Mb, A, xb, px) && s3_pass(p.Ma, B, xa, px);
}

LM_FN bool s3_finite_row(const double (&A)[3], const double (&xa)[2], const double (&B)[3], const double (&xb)[2]) {
    return std::isfinite(A[0]) && std::isfinite(A[1]) && std::isfinite(A[2]) && std::isfinite(xa[0]) && std::isfinite(xa[1]) &&
           std::isfinite(B[0]) && std::isfinite(B[1]) && std::isfinite(B[2]) && std::isfinite(xb[0]) && std::isfinite(xb[1]);
}

// one order-free maximum: the larger count wins, then the smaller h; 0 where there is no model
LM_FN uint32_t s3_key(int count, int h) { return count < 0 ? 0u : ((uint32_t)count << 10) | (uint32_t)(kS3MaxHyp - 1 - h); }
LM_FN int s3_key_count(uint32_t key) { return (int)(key >> 10); }
LM_FN int s3_key_h(uint32_t key) { return kS3MaxHyp - 1 - (int)(key & (kS3MaxHyp - 1)); }

// ---- on the world (vslam_world_sim3, vslam_world_apply_sim3): Twc is a camera -> world matrix, row-major 4 x 4
// W^t (p - C): a world point in the camera's coordinates; the transpose stands for the inverse
LM_FN void s3_to_camera(const double *Twc, const double (&p)[3], double (&out)[3]) {
    const double D[3] = {p[0] - Twc[3], p[1] - Twc[7], p[2] - Twc[11]};
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = (Twc[i] * D[0] + Twc[4 + i] * D[1]) + Twc[8 + i] * D[2];
}

// X_a = s_w R_w X_b + t_w from the camera-to-camera model m (a -> b) and the two cameras' matrices
LM_FN void s3_world_similarity(const double *Ta, const double *Tb, const S3Model &m, double &sw, double (&Rw)[9], double (&tw)[3]) {
    sw = 1.0 / m.s;
    double M[9], u[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 * i + j] = (Ta[4 * i] * m.R[3 * j] + Ta[4 * i + 1] * m.R[3 * j + 1]) + Ta[4 * i + 2] * m.R[3 * j + 2];
        u[i] = (m.R[i] * m.t[0] + m.R[3 + i] * m.t[1]) + m.R[6 + i] * m.t[2];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Rw[3 * i + j] = (M[3 * i] * Tb[4 * j] + M[3 * i + 1] * Tb[4 * j + 1]) + M[3 * i + 2] * Tb[4 * j + 2];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double v = (Ta[4 * r] * u[0] + Ta[4 * r + 1] * u[1]) + Ta[4 * r + 2] * u[2];
        const double w = (Rw[3 * r] * Tb[3] + Rw[3 * r + 1] * Tb[7]) + Rw[3 * r + 2] * Tb[11];
        tw[r] = (Ta[4 * r + 3] - v / m.s) - sw * w;
    }
}

// s (R X) + t
LM_FN void s3_apply_point(const S3Model &m, const double (&X)[3], double (&out)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = m.s * ((m.R[3 * i] * X[0] + m.R[3 * i + 1] * X[1]) + m.R[3 * i + 2] * X[2]) + m.t[i];
}

// a camera -> world matrix carried through X' = s R X + t: rotation block R W, centre s (R C) + t, row 3 kept
LM_FN void s3_apply_pose(const S3Model &m, const double *in, double (&out)[16]) {
    const double C[3] = {in[3], in[7], in[11]};
    double Cn[3];
    s3_apply_point(m, C, Cn);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[4 * i + j] = (m.R[3 * i] * in[j] + m.R[3 * i + 1] * in[4 + j]) + m.R[3 * i + 2] * in[8 + j];
        out[4 * i + 3] = Cn[i];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) out[12 + j] = in[12 + j];
}

// ---- the polish
struct S3Obs {   // one correspondence under a model: both directions
    double W[3];   // s (R A)
    LmPoint b, a;  // b: A into image b (RX unused); a: B into image a
};

LM_FN void s3_obs(const double (&K)[9], const S3Model &m, const double (&A)[3], const double (&xa)[2], const double (&B)[3],
                  const double (&xb)[2], S3Obs &o) {
    double RA[3], unused[3];
    lm_transform(m.R, m.t, A, RA, unused);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        o.W[r] = m.s * RA[r];
        o.b.Y[r] = o.W[r] + m.t[r];
    }
    lm_project(K, o.b.Y, o.b.u, o.b.v, o.b.q2);
    o.b.r[0] = o.b.u - xb[0];
    o.b.r[1] = o.b.v - xb[1];
    o.b.e = sqrt(o.b.r[0] * o.b.r[0] + o.b.r[1] * o.b.r[1]);
    const double D[3] = {B[0] - m.t[0], B[1] - m.t[1], B[2] - m.t[2]};
#pragma unroll
    for (int r = 0; r < 3; r++) o.a.Y[r] = ((m.R[r] * D[0] + m.R[3 + r] * D[1]) + m.R[6 + r] * D[2]) / m.s;
    lm_project(K, o.a.Y, o.a.u, o.a.v, o.a.q2);
    o.a.r[0] = o.a.u - xa[0];
    o.a.r[1] = o.a.v - xa[1];
    o.a.e = sqrt(o.a.r[0] * o.a.r[0] + o.a.r[1] * o.a.r[1]);
}

LM_FN bool s3_front(const S3Obs &o) { return o.b.Y[2] > 0.0 && o.a.Y[2] > 0.0; }
LM_FN double s3_rho(const S3Obs &o, double delta) { return lm_rho(o.b.e, delta) + lm_rho(o.a.e, delta); }

LM_FN bool s3_gate(const double (&K)[9], const S3Model &g, double gate, const double (&A)[3], const double (&xa)[2], const double (&B)[3],
                   const double (&xb)[2]) {
    S3Obs o;
    s3_obs(K, g, A, xa, B, xb, o);
    return s3_front(o) && o.b.e <= gate && o.a.e <= gate;
}

// what one correspondence adds to H (a[0..28), upper triangle by lm_tri<7>) and to g (a[28..35)) at model m
LM_FN void s3_contribution(const double (&K)[9], const S3Model &m, double delta, const double (&A)[3], const double (&xa)[2],
                           const double (&B)[3], const double (&xb)[2], double (&a)[kS3Sums]) {
    S3Obs o;
    s3_obs(K, m, A, xa, B, xb, o);
    double Ab[2][3], Aa[2][3], Jb[2][7], Ja[2][7], N[2][7];
    lm_dproj(K, o.b.u, o.b.v, o.b.q2, Ab);
    lm_jac_rotation(Ab, o.W, Jb);
    lm_dproj(K, o.a.u, o.a.v, o.a.q2, Aa);
    lm_jac_rotation(Aa, o.a.Y, N);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        Jb[r][3] = Ab[r][0];
        Jb[r][4] = Ab[r][1];
        Jb[r][5] = Ab[r][2];
        Jb[r][6] = (Ab[r][0] * o.W[0] + Ab[r][1] * o.W[1]) + Ab[r][2] * o.W[2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Ja[r][k] = -((N[r][0] * m.R[3 * k] + N[r][1] * m.R[3 * k + 1]) + N[r][2] * m.R[3 * k + 2]);
            Ja[r][3 + k] = -(((Aa[r][0] * m.R[3 * k] + Aa[r][1] * m.R[3 * k + 1]) + Aa[r][2] * m.R[3 * k + 2]) / m.s);
        }
        Ja[r][6] = -((Aa[r][0] * o.a.Y[0] + Aa[r][1] * o.a.Y[1]) + Aa[r][2] * o.a.Y[2]);
    }
    const double wb = lm_weight(o.b.e, delta), wa = lm_weight(o.a.e, delta);
#pragma unroll
    for (int i = 0; i < 7; i++) {
#pragma unroll
        for (int j = i; j < 7; j++)
            a[lm_tri<7>(i, j)] = wb * (Jb[0][i] * Jb[0][j] + Jb[1][i] * Jb[1][j]) + wa * (Ja[0][i] * Ja[0][j] + Ja[1][i] * Ja[1][j]);
        a[28 + i] = wb * (Jb[0][i] * o.b.r[0] + Jb[1][i] * o.b.r[1]) + wa * (Ja[0][i] * o.a.r[0] + Ja[1][i] * o.a.r[1]);
    }
}

LM_FN bool s3_solve(const double (&acc)[kS3Sums], double lambda, double (&d)[7]) {
    double diag[7];
#pragma unroll
    for (int j = 0; j < 7; j++) {
        const double h = acc[lm_tri<7>(j, j)];
        diag[j] = h + lambda * fmax(h, kDiagFloor);
    }
    return lm_chol_solve<7>(acc, diag, d);
}

LM_FN bool s3_finite(const S3Model &m) {
    bool ok = std::isfinite(m.s);
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(m.R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(m.t[k]);
    return ok;
}

// The rounds of the polish: resect_math.h's rs_run over a similarity.  Src::each(f) calls f(A, xa, B, xb) for the correspondences
// this caller owns; Red closes sums and flags over all callers.  Returns true with the result in `out` when the model moved.
template <class Src, class Red>
LM_FN bool s3_run(const double (&K)[9], const S3Model &in, const RsParams &p, Src &src, Red &red, S3Model &out, double (&stats)[4]) {
    const double qnan = __builtin_nan("");
    stats[1] = stats[2] = stats[3] = qnan;
    double c1[1] = {0.0};
    bool bad = false;
    src.each([&](const double(&A)[3], const double(&xa)[2], const double(&B)[3], const double(&xb)[2]) {
        c1[0] += 1.0;
        bad = bad || !s3_finite_row(A, xa, B, xb);
    });
    red.sum(c1);
    bad = red.any(bad);
    stats[0] = c1[0];
    bool kfin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) kfin = kfin && std::isfinite(K[k]);
    if (c1[0] < (double)p.min_links || bad || !kfin || !s3_finite(in) || !(in.s > 0.0)) return false;

    S3Model start, cur, gm;
    start = in;
    lm_polar_step(in.R, start.R);
    cur = start;
    gm = start;
    bool gated = false;
    int accepted = 0;
    for (int round = 0; round < p.rounds; round++) {
        const bool g = round > 0;
        double co[2] = {0.0, 0.0};
        src.each([&](const double(&A)[3], const double(&xa)[2], const double(&B)[3], const double(&xb)[2]) {
            S3Obs o;
            s3_obs(K, cur, A, xa, B, xb, o);
            if (g && !(s3_front(o) && o.b.e <= p.gate && o.a.e <= p.gate)) return;
            co[0] += 1.0;
            co[1] += s3_rho(o, p.huber);
        });
        red.sum(co);
        if (g) {
            if (co[0] < (double)p.min_links) break;   // the previous round's result stands
            gm = cur;
            gated = true;
        }
        stats[0] = co[0];
        double obj = co[1], lambda = kLambda0;
        for (int it = 0; it < p.max_iterations; it++) {
            double acc[kS3Sums];
#pragma unroll
            for (int k = 0; k < kS3Sums; k++) acc[k] = 0.0;
            src.each([&](const double(&A)[3], const double(&xa)[2], const double(&B)[3], const double(&xb)[2]) {
                if (gated && !s3_gate(K, gm, p.gate, A, xa, B, xb)) return;
                double a[kS3Sums];
                s3_contribution(K, cur, p.huber, A, xa, B, xb, a);
#pragma unroll
                for (int k = 0; k < kS3Sums; k++) acc[k] += a[k];
            });
            red.sum(acc);
            double d[7];
            bool accept = false;
            double obj_new = 0.0;
            S3Model cand;
            if (s3_solve(acc, lambda, d)) {   // the same everywhere
                const double w[3] = {d[0], d[1], d[2]};
                lm_rotate(w, cur.R, cand.R);
#pragma unroll
                for (int k = 0; k < 3; k++) cand.t[k] = cur.t[k] + d[3 + k];
                cand.s = cur.s * (1.0 + d[6]);
                if (cand.s > 0.0) {
                    double so[1] = {0.0};
                    bool behind = false;
                    src.each([&](const double(&A)[3], const double(&xa)[2], const double(&B)[3], const double(&xb)[2]) {
                        if (gated && !s3_gate(K, gm, p.gate, A, xa, B, xb)) return;
                        S3Obs o;
                        s3_obs(K, cand, A, xa, B, xb, o);
                        so[0] += s3_rho(o, p.huber);
                        behind = behind || !s3_front(o);
                    });
                    red.sum(so);
                    behind = red.any(behind);
                    obj_new = so[0];
                    accept = !behind && obj_new < obj;   // false for a NaN objective
                }
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
    if (accepted == 0 || !s3_finite(cur)) return false;
    double sf[2] = {0.0, 0.0};
    src.each([&](const double(&A)[3], const double(&xa)[2], const double(&B)[3], const double(&xb)[2]) {
        if (gated && !s3_gate(K, gm, p.gate, A, xa, B, xb)) return;
        S3Obs o;
        s3_obs(K, start, A, xa, B, xb, o);
        sf[0] += s3_rho(o, p.huber);
        s3_obs(K, cur, A, xa, B, xb, o);
        sf[1] += s3_rho(o, p.huber);
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
}  // namespace vs_sim3
