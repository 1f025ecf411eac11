// Pose-graph optimisation over Sim(3) (include/vslam_graph.h): everything that does not know about lanes.  The residual of an edge
// and its two Jacobians, the normal equations' diagonal blocks, the matrix-free operator of the conjugate gradient, and the whole
// schedule (gr_run) over a `Par` that says who owns which unit and how sums are closed: graph.hip's is a workgroup of 256 lanes with
// block_reduce.h; tests/native/graph_serial.cpp's is one caller that owns everything.  All f64, never fused, operand order as
// written (compile host code with -ffp-contract=off).
#pragma once

#include <cmath>
#include <cstdint>

#include "lm_math.h"

namespace vs_graph {
using namespace vs_lm;

constexpr int kGrNode = 13;    // s, R [9], t [3]
constexpr int kGrLin = 38;     // an edge's linearisation: A [9], T [9], Bw [9], bs [3], se, r [7]
constexpr int kGrNodeF64 = 2 * kGrNode + 2 * 28 + 6 * 7;   // cur, cand, H, L, g, x, r, z, p, q
constexpr int kGrEdgeF64 = kGrLin + 7;                     // the linearisation and y = W u
constexpr int kGrNodeI32 = 4;                              // start, fill, active, (start's last word and padding share the 4th)
constexpr int kGrEdgeI32 = 3;                              // use, adj x 2

struct GrParams {
    int max_iterations, cg_iterations;
    double cg_tolerance;
};

struct GrNodeV {
    double s, R[9], t[3];
};

LM_FN void gr_load(const double *p, GrNodeV &n) {
    n.s = p[0];
#pragma unroll
    for (int k = 0; k < 9; k++) n.R[k] = p[1 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) n.t[k] = p[10 + k];
}

LM_FN void gr_store(const GrNodeV &n, double *p) {
    p[0] = n.s;
#pragma unroll
    for (int k = 0; k < 9; k++) p[1 + k] = n.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) p[10 + k] = n.t[k];
}

LM_FN bool gr_finite(const GrNodeV &n) {
    bool ok = std::isfinite(n.s);
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(n.R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(n.t[k]);
    return ok;
}

// the measurement of an edge: Z = (s, R, t) takes camera a to camera b; w = (w_rot, w_t, w_s)
struct GrMeas {
    GrNodeV Z;
    double w[3];
};

LM_FN bool gr_meas_ok(const GrMeas &m) {
    bool ok = gr_finite(m.Z) && m.Z.s > 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(m.w[k]) && m.w[k] >= 0.0;
    return ok;
}

// what the residual and the Jacobians share: P = S_b^-1 S_a and E = Z^-1 P
struct GrErr {
    double v[3], tp[3], se, r[7];
};

LM_FN void gr_residual(const GrNodeV &a, const GrNodeV &b, const GrNodeV &Z, GrErr &e) {
    const double sp = a.s / b.s;
    double Rp[9], Re[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Rp[3 * i + j] = (b.R[i] * a.R[j] + b.R[3 + i] * a.R[3 + j]) + b.R[6 + i] * a.R[6 + j];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) e.v[k] = a.t[k] - b.t[k];
#pragma unroll
    for (int i = 0; i < 3; i++) e.tp[i] = ((b.R[i] * e.v[0] + b.R[3 + i] * e.v[1]) + b.R[6 + i] * e.v[2]) / b.s;
    e.se = sp / Z.s;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Re[3 * i + j] = (Z.R[i] * Rp[j] + Z.R[3 + i] * Rp[3 + j]) + Z.R[6 + i] * Rp[6 + j];
    }
    const double d[3] = {e.tp[0] - Z.t[0], e.tp[1] - Z.t[1], e.tp[2] - Z.t[2]};
    e.r[0] = (Re[7] - Re[5]) / 2.0;
    e.r[1] = (Re[2] - Re[6]) / 2.0;
    e.r[2] = (Re[3] - Re[1]) / 2.0;
#pragma unroll
    for (int i = 0; i < 3; i++) e.r[3 + i] = ((Z.R[i] * d[0] + Z.R[3 + i] * d[1]) + Z.R[6 + i] * d[2]) / Z.s;
    e.r[6] = e.se - 1.0;
}

LM_FN double gr_cost(const double (&r)[7], const double (&w)[3]) {
    return (w[0] * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + w[1] * ((r[3] * r[3] + r[4] * r[4]) + r[5] * r[5])) + w[2] * (r[6] * r[6]);
}

// The linearisation of an edge at (a, b), into lin [38]: the blocks the two Jacobians are made of and the residual.
//   J_a: rows 0..2 x columns 0..2 = A;  rows 3..5 x columns 3..5 = T;  (6, 6) = se;  zero elsewhere.
//   J_b: rows 0..2 x columns 0..2 = -A; rows 3..5 x columns 0..2 = Bw; rows 3..5 x columns 3..5 = -T; rows 3..5 x column 6 = bs;
//        (6, 6) = -se; zero elsewhere.
LM_FN void gr_linearise(const GrNodeV &a, const GrNodeV &b, const GrNodeV &Z, double *lin) {
    GrErr e;
    gr_residual(a, b, Z, e);
    double Q[9];   // Z_R^t R_b^t
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Q[3 * i + j] = (Z.R[i] * b.R[3 * j] + Z.R[3 + i] * b.R[3 * j + 1]) + Z.R[6 + i] * b.R[3 * j + 2];
    }
    double *A = lin, *T = lin + 9, *Bw = lin + 18, *bs = lin + 27;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        // D = Q [e_k]x R_a: D_mn = Q_m,k2 Ra_k1,n - Q_m,k1 Ra_k2,n
        auto D = [&](int m, int n) { return Q[3 * m + k2] * a.R[3 * k1 + n] - Q[3 * m + k1] * a.R[3 * k2 + n]; };
        A[k] = (D(2, 1) - D(1, 2)) / 2.0;
        A[3 + k] = (D(0, 2) - D(2, 0)) / 2.0;
        A[6 + k] = (D(1, 0) - D(0, 1)) / 2.0;
#pragma unroll
        for (int i = 0; i < 3; i++) Bw[3 * i + k] = -(((Q[3 * i + k2] * e.v[k1] - Q[3 * i + k1] * e.v[k2]) / b.s) / Z.s);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) T[k] = (Q[k] / b.s) / Z.s;
#pragma unroll
    for (int i = 0; i < 3; i++) bs[i] = -(((Z.R[i] * e.tp[0] + Z.R[3 + i] * e.tp[1]) + Z.R[6 + i] * e.tp[2]) / Z.s);
    lin[30] = e.se;
#pragma unroll
    for (int k = 0; k < 7; k++) lin[31 + k] = e.r[k];
}

// the dense 7 x 7 Jacobian of one side (0: a, 1: b) from the linearisation
LM_FN void gr_dense(const double *lin, int side, double (&J)[7][7]) {
    const double *A = lin, *T = lin + 9, *Bw = lin + 18, *bs = lin + 27;
    const double se = lin[30];
#pragma unroll
    for (int i = 0; i < 7; i++) {
#pragma unroll
        for (int j = 0; j < 7; j++) J[i][j] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            J[i][j] = side ? -A[3 * i + j] : A[3 * i + j];
            J[3 + i][3 + j] = side ? -T[3 * i + j] : T[3 * i + j];
            if (side) J[3 + i][j] = Bw[3 * i + j];
        }
        if (side) J[3 + i][6] = bs[i];
    }
    J[6][6] = side ? -se : se;
}

// what one edge adds to a node's block H (acc[0..28), upper triangle by lm_tri<7>) and gradient g (acc[28..35)): for k <= l the sum
// over the rows i = 0 .. 6, left to right, of (W_i J_ik) J_il, and of (W_i J_ik) r_i
LM_FN void gr_accumulate(const double *lin, int side, const double (&w)[3], double (&acc)[35]) {
    double J[7][7];
    gr_dense(lin, side, J);
    const double W[7] = {w[0], w[0], w[0], w[1], w[1], w[1], w[2]};
#pragma unroll
    for (int k = 0; k < 7; k++) {
        double wj[7];
#pragma unroll
        for (int i = 0; i < 7; i++) wj[i] = W[i] * J[i][k];
#pragma unroll
        for (int l = k; l < 7; l++) {
            double s = wj[0] * J[0][l];
#pragma unroll
            for (int i = 1; i < 7; i++) s = s + wj[i] * J[i][l];
            acc[lm_tri<7>(k, l)] += s;
        }
        double s = wj[0] * lin[31];
#pragma unroll
        for (int i = 1; i < 7; i++) s = s + wj[i] * lin[31 + i];
        acc[28 + k] += s;
    }
}

// y = W (J_a p_a + J_b p_b), through the blocks
LM_FN void gr_edge_apply(const double *lin, const double *pa, const double *pb, const double (&w)[3], double *y) {
    const double *A = lin, *T = lin + 9, *Bw = lin + 18, *bs = lin + 27;
    const double dw[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]}, dt[3] = {pa[3] - pb[3], pa[4] - pb[4], pa[5] - pb[5]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        y[i] = w[0] * ((A[3 * i] * dw[0] + A[3 * i + 1] * dw[1]) + A[3 * i + 2] * dw[2]);
        const double t = (T[3 * i] * dt[0] + T[3 * i + 1] * dt[1]) + T[3 * i + 2] * dt[2];
        const double c = ((Bw[3 * i] * pb[0] + Bw[3 * i + 1] * pb[1]) + Bw[3 * i + 2] * pb[2]) + bs[i] * pb[6];
        y[3 + i] = w[1] * (t + c);
    }
    y[6] = w[2] * (lin[30] * (pa[6] - pb[6]));
}

// q += J_side^t y
LM_FN void gr_node_gather(const double *lin, int side, const double *y, double (&q)[7]) {
    const double *A = lin, *T = lin + 9, *Bw = lin + 18, *bs = lin + 27;
    double o[7];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o[k] = (A[k] * y[0] + A[3 + k] * y[1]) + A[6 + k] * y[2];
        o[3 + k] = (T[k] * y[3] + T[3 + k] * y[4]) + T[6 + k] * y[5];
    }
    o[6] = lin[30] * y[6];
    if (side) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            o[k] = ((Bw[k] * y[3] + Bw[3 + k] * y[4]) + Bw[6 + k] * y[5]) - o[k];
            o[3 + k] = -o[3 + k];
        }
        o[6] = ((bs[0] * y[3] + bs[1] * y[4]) + bs[2] * y[5]) - o[6];
    }
#pragma unroll
    for (int k = 0; k < 7; k++) q[k] += o[k];
}

// H* = H + lambda max(diag H, floor) = L L^t, L's lower triangle row by row (lm_chol_solve<7>'s factorisation, kept); false for a
// pivot that is not > 0
LM_FN bool gr_factor(const double *H, double lambda, double *L) {
    bool ok = true;
    double M[7][7];
#pragma unroll
    for (int j = 0; j < 7; j++) {
        const double h = H[lm_tri<7>(j, j)];
        double p = h + lambda * fmax(h, kDiagFloor);
#pragma unroll
        for (int k = 0; k < j; k++) p = p - M[j][k] * M[j][k];
        ok = ok && p > 0.0;
        M[j][j] = sqrt(p);
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = H[lm_tri<7>(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - M[i][k] * M[j][k];
            M[i][j] = s / M[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) L[i * (i + 1) / 2 + j] = M[i][j];
    }
    return ok;
}

// z = (L L^t)^-1 r
LM_FN void gr_precondition(const double *L, const double (&r)[7], double (&z)[7]) {
    double f[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double s = r[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[i * (i + 1) / 2 + k] * f[k];
        f[i] = s / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double s = f[i];
#pragma unroll
        for (int k = 6; k > i; k--) s = s - L[k * (k + 1) / 2 + i] * z[k];
        z[i] = s / L[i * (i + 1) / 2 + i];
    }
}

LM_FN double gr_dot7(const double *a, const double *b) {
    double s = a[0] * b[0];
#pragma unroll
    for (int k = 1; k < 7; k++) s = s + a[k] * b[k];
    return s;
}

// One item's arrays.  The caller's (read through these pointers, written only at the end) and the workspace; nothing is
// __restrict__: the passes hand values to each other through the workspace, between par.sync()s.
struct GrItem {
    int n_nodes, n_edges, node_stride, edge_stride;   // the counts as given
    double *scale, *R, *T;
    const int32_t *fixed, *ab;
    const double *z_scale, *z_R, *z_T, *z_w;
    double *nodes_a, *nodes_b, *H, *L, *g, *x, *r, *z, *p, *q;   // [node_stride] x 13, 13, 28, 28, 7 ...
    double *lin, *y;                                            // [edge_stride] x 38, 7
    int32_t *start, *fill, *active;                             // [node_stride + 1], [node_stride], [node_stride]
    int32_t *use, *adj;                                         // [edge_stride], [2 edge_stride]: edge << 1 | side
};

// the workspace of one item, in bytes, and its layout behind `base` (8-byte aligned)
LM_FN size_t gr_workspace_bytes(int node_stride, int edge_stride) {
    const size_t words = (size_t)kGrNodeI32 * node_stride + (size_t)kGrEdgeI32 * edge_stride + 4;
    return sizeof(double) * ((size_t)kGrNodeF64 * node_stride + (size_t)kGrEdgeF64 * edge_stride) + 4 * ((words + 1) / 2 * 2);
}

LM_FN void gr_workspace(void *base, GrItem &it) {
    const size_t N = (size_t)it.node_stride, E = (size_t)it.edge_stride;
    double *d = static_cast<double *>(base);
    it.nodes_a = d; d += kGrNode * N;
    it.nodes_b = d; d += kGrNode * N;
    it.H = d; d += 28 * N;
    it.L = d; d += 28 * N;
    it.g = d; d += 7 * N;
    it.x = d; d += 7 * N;
    it.r = d; d += 7 * N;
    it.z = d; d += 7 * N;
    it.p = d; d += 7 * N;
    it.q = d; d += 7 * N;
    it.lin = d; d += kGrLin * E;
    it.y = d; d += 7 * E;
    int32_t *w = reinterpret_cast<int32_t *>(d);
    it.start = w; w += N + 1;
    it.fill = w; w += N;
    it.active = w; w += N;
    it.use = w; w += E;
    it.adj = w;
}

LM_FN void gr_meas_load(const GrItem &it, int k, GrMeas &m) {
    m.Z.s = it.z_scale[k];
#pragma unroll
    for (int j = 0; j < 9; j++) m.Z.R[j] = it.z_R[9 * (size_t)k + j];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        m.Z.t[j] = it.z_T[3 * (size_t)k + j];
        m.w[j] = it.z_w[3 * (size_t)k + j];
    }
}

LM_FN void gr_input_load(const GrItem &it, int i, GrNodeV &n) {
    n.s = it.scale[i];
#pragma unroll
    for (int j = 0; j < 9; j++) n.R[j] = it.R[9 * (size_t)i + j];
#pragma unroll
    for (int j = 0; j < 3; j++) n.t[j] = it.T[3 * (size_t)i + j];
}

LM_FN bool gr_usable(const GrItem &it, int k, int N) {
    const int a = it.ab[2 * (size_t)k], b = it.ab[2 * (size_t)k + 1];
    if (!(a >= 0 && a < N && b >= 0 && b < N && a != b)) return false;
    if (it.fixed[a] != 0 && it.fixed[b] != 0) return false;
    GrMeas m;
    gr_meas_load(it, k, m);
    return gr_meas_ok(m);
}

// the cost of the usable edges under `nodes`, in every caller
template <class Par>
LM_FN double gr_total_cost(Par &par, const GrItem &it, int E, const double *nodes) {
    double c[1] = {0.0};
    par.each(E, [&](int k) {
        if (!it.use[k]) return;
        GrMeas m;
        gr_meas_load(it, k, m);
        GrNodeV a, b;
        gr_load(nodes + (size_t)kGrNode * it.ab[2 * (size_t)k], a);
        gr_load(nodes + (size_t)kGrNode * it.ab[2 * (size_t)k + 1], b);
        GrErr e;
        gr_residual(a, b, m.Z, e);
        c[0] += gr_cost(e.r, m.w);
    });
    par.sum(c);
    return c[0];
}

// The conjugate gradient on (H + lambda D) x = -g, x left in it.x.  0: the step is refused, otherwise 1; `iterations` counts.
template <class Par>
LM_FN int gr_solve(Par &par, const GrItem &it, int N, int E, double lambda, const GrParams &prm, int &iterations) {
    bool bad = false;
    double rho_v[1] = {0.0};
    par.each(N, [&](int i) {
        double *x = it.x + 7 * (size_t)i, *r = it.r + 7 * (size_t)i, *z = it.z + 7 * (size_t)i, *p = it.p + 7 * (size_t)i;
        if (!it.active[i]) {
#pragma unroll
            for (int k = 0; k < 7; k++) x[k] = r[k] = z[k] = p[k] = 0.0;
            return;
        }
        bad = bad || !gr_factor(it.H + 28 * (size_t)i, lambda, it.L + 28 * (size_t)i);
        double rr[7], zz[7];
#pragma unroll
        for (int k = 0; k < 7; k++) rr[k] = -it.g[7 * (size_t)i + k];
        gr_precondition(it.L + 28 * (size_t)i, rr, zz);
#pragma unroll
        for (int k = 0; k < 7; k++) {
            x[k] = 0.0;
            r[k] = rr[k];
            z[k] = zz[k];
            p[k] = zz[k];
        }
        rho_v[0] += gr_dot7(rr, zz);
    });
    bad = par.any(bad);
    par.sum(rho_v);
    if (bad) return 0;
    double rho = rho_v[0];
    const double rho0 = rho;
    for (int iter = 0; iter < prm.cg_iterations; iter++) {
        par.sync();   // p
        par.each(E, [&](int k) {
            if (!it.use[k]) return;
            double w[3];
#pragma unroll
            for (int j = 0; j < 3; j++) w[j] = it.z_w[3 * (size_t)k + j];
            gr_edge_apply(it.lin + (size_t)kGrLin * k, it.p + 7 * (size_t)it.ab[2 * (size_t)k], it.p + 7 * (size_t)it.ab[2 * (size_t)k + 1], w,
                          it.y + 7 * (size_t)k);
        });
        par.sync();   // y
        double pq[1] = {0.0};
        par.each(N, [&](int i) {
            if (!it.active[i]) return;
            const double *H = it.H + 28 * (size_t)i, *p = it.p + 7 * (size_t)i;
            double q[7];
#pragma unroll
            for (int k = 0; k < 7; k++) q[k] = 0.0;
            for (int s = it.start[i]; s < it.start[i + 1]; s++) {
                const int k = it.adj[s] >> 1;
                gr_node_gather(it.lin + (size_t)kGrLin * k, it.adj[s] & 1, it.y + 7 * (size_t)k, q);
            }
#pragma unroll
            for (int k = 0; k < 7; k++) {
                q[k] = q[k] + (lambda * fmax(H[lm_tri<7>(k, k)], kDiagFloor)) * p[k];
                it.q[7 * (size_t)i + k] = q[k];
            }
            pq[0] += gr_dot7(p, q);
        });
        par.sum(pq);
        if (!(pq[0] > 0.0) || !std::isfinite(pq[0])) {
            if (iter == 0) return 0;
            break;
        }
        const double alpha = rho / pq[0];
        double rn[1] = {0.0};
        par.each(N, [&](int i) {
            if (!it.active[i]) return;
            double *x = it.x + 7 * (size_t)i, *r = it.r + 7 * (size_t)i, *z = it.z + 7 * (size_t)i;
            const double *p = it.p + 7 * (size_t)i, *q = it.q + 7 * (size_t)i;
            double rr[7], zz[7];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                x[k] = x[k] + alpha * p[k];
                rr[k] = r[k] - alpha * q[k];
                r[k] = rr[k];
            }
            gr_precondition(it.L + 28 * (size_t)i, rr, zz);
#pragma unroll
            for (int k = 0; k < 7; k++) z[k] = zz[k];
            rn[0] += gr_dot7(rr, zz);
        });
        par.sum(rn);
        iterations++;
        if (rn[0] <= prm.cg_tolerance * rho0 || iter + 1 == prm.cg_iterations) break;
        const double beta = rn[0] / rho;
        rho = rn[0];
        par.each(N, [&](int i) {
            if (!it.active[i]) return;
            double *p = it.p + 7 * (size_t)i;
            const double *z = it.z + 7 * (size_t)i;
#pragma unroll
            for (int k = 0; k < 7; k++) p[k] = z[k] + beta * p[k];
        });
    }
    return 1;
}

// The whole schedule of one item.  Par: each(n, f) calls f(i) for the units i < n this caller owns (the same units in every pass);
// sum / any close sums and flags over all callers; sync() orders the workspace between passes; adjacency(it, N, E) fills start /
// adj from use.  Every caller returns the same: whether the item moved.  stats [4]; cg_total: the CG iterations taken.
template <class Par>
LM_FN bool gr_run(Par &par, GrItem &it, const GrParams &prm, double (&stats)[4], int &cg_total) {
    const double qnan = __builtin_nan("");
    stats[0] = 0.0;
    stats[1] = stats[2] = stats[3] = qnan;
    cg_total = 0;
    const int N = it.n_nodes, E = it.n_edges;
    if (N < 1 || N > it.node_stride || E < 0 || E > it.edge_stride) return false;
    bool bad = false, held = false;
    par.each(N, [&](int i) {
        GrNodeV n;
        gr_input_load(it, i, n);
        bad = bad || !gr_finite(n) || !(n.s > 0.0);
        held = held || it.fixed[i] != 0;
    });
    bad = par.any(bad);
    held = par.any(held);
    double cnt[1] = {0.0};
    par.each(E, [&](int k) {
        const bool u = gr_usable(it, k, N);
        it.use[k] = u ? 1 : 0;
        if (u) cnt[0] += 1.0;
    });
    par.sum(cnt);
    stats[0] = cnt[0];
    if (bad || !held || !(cnt[0] > 0.0)) return false;
    par.sync();   // use
    par.adjacency(it, N, E);
    double *cur = it.nodes_a, *cand = it.nodes_b;
    par.each(N, [&](int i) {
        GrNodeV n, s;
        gr_input_load(it, i, n);
        s = n;
        const bool free_node = it.fixed[i] == 0;
        if (free_node) lm_polar_step(n.R, s.R);
        it.active[i] = free_node && it.start[i + 1] > it.start[i] ? 1 : 0;
        gr_store(s, cur + (size_t)kGrNode * i);
    });
    par.sync();   // cur
    const double obj0 = gr_total_cost(par, it, E, cur);
    double obj = obj0, lambda = kLambda0;
    int accepted = 0;
    for (int iter = 0; iter < prm.max_iterations; iter++) {
        par.each(E, [&](int k) {
            if (!it.use[k]) return;
            GrMeas m;
            gr_meas_load(it, k, m);
            GrNodeV a, b;
            gr_load(cur + (size_t)kGrNode * it.ab[2 * (size_t)k], a);
            gr_load(cur + (size_t)kGrNode * it.ab[2 * (size_t)k + 1], b);
            gr_linearise(a, b, m.Z, it.lin + (size_t)kGrLin * k);
        });
        par.sync();   // lin
        par.each(N, [&](int i) {
            if (!it.active[i]) return;
            double acc[35];
#pragma unroll
            for (int k = 0; k < 35; k++) acc[k] = 0.0;
            for (int s = it.start[i]; s < it.start[i + 1]; s++) {
                const int k = it.adj[s] >> 1;
                double w[3];
#pragma unroll
                for (int j = 0; j < 3; j++) w[j] = it.z_w[3 * (size_t)k + j];
                gr_accumulate(it.lin + (size_t)kGrLin * k, it.adj[s] & 1, w, acc);
            }
#pragma unroll
            for (int k = 0; k < 28; k++) it.H[28 * (size_t)i + k] = acc[k];
#pragma unroll
            for (int k = 0; k < 7; k++) it.g[7 * (size_t)i + k] = acc[28 + k];
        });
        bool accept = false;
        double obj_new = 0.0;
        if (gr_solve(par, it, N, E, lambda, prm, cg_total)) {
            bool neg = false;
            par.each(N, [&](int i) {
                GrNodeV c, d;
                gr_load(cur + (size_t)kGrNode * i, c);
                d = c;
                if (it.active[i]) {
                    const double *x = it.x + 7 * (size_t)i;
                    const double w[3] = {x[0], x[1], x[2]};
                    lm_rotate(w, c.R, d.R);
#pragma unroll
                    for (int k = 0; k < 3; k++) d.t[k] = c.t[k] + x[3 + k];
                    d.s = c.s * (1.0 + x[6]);
                    neg = neg || !(d.s > 0.0);
                }
                gr_store(d, cand + (size_t)kGrNode * i);
            });
            neg = par.any(neg);
            par.sync();   // cand
            if (!neg) {
                obj_new = gr_total_cost(par, it, E, cand);
                accept = obj_new < obj;   // false for a NaN
            }
        }
        if (accept) {
            const double rel = (obj - obj_new) / obj;
            double *t = cur;
            cur = cand;
            cand = t;
            obj = obj_new;
            accepted++;
            lambda = fmax(lambda / 10.0, kLambdaMin);
            if (rel < kRelStop) break;
        } else {
            lambda = lambda * 10.0;
            if (lambda > kLambdaMax) break;
        }
        par.sync();   // the edge pass of the next iteration overwrites lin, which this iteration's last gather read
    }
    if (accepted == 0) return false;
    bool nf = false;
    par.each(N, [&](int i) {
        GrNodeV c;
        gr_load(cur + (size_t)kGrNode * i, c);
        nf = nf || (it.active[i] && !gr_finite(c));
    });
    nf = par.any(nf);
    const double s1 = obj0 / stats[0], s2 = obj / stats[0];
    if (nf || !(std::isfinite(s1) && std::isfinite(s2))) return false;
    stats[1] = s1;
    stats[2] = s2;
    stats[3] = (double)accepted;
    par.each(N, [&](int i) {
        if (!it.active[i]) return;
        GrNodeV c;
        gr_load(cur + (size_t)kGrNode * i, c);
        it.scale[i] = c.s;
#pragma unroll
        for (int k = 0; k < 9; k++) it.R[9 * (size_t)i + k] = c.R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) it.T[3 * (size_t)i + k] = c.t[k];
    });
    return true;
}
}  // namespace vs_graph
