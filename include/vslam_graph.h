/* Pose-graph optimisation over Sim(3): spreading the error of loops over the frames between their ends, for a batch of independent
 * graphs, on the device.  A monocular world drifts in scale, rotation and position along a track; place recognition (vslam_places.h)
 * finds which earlier frame a frame revisits, vslam_sim3_ransac / vslam_world_sim3 (vslam_sim3.h) measure the similarity between the
 * two views, and this header moves every frame in between.  Explicit calls: nothing in the other headers launches a kernel of this
 * file, and no existing output changes a bit.
 *
 * THIS TEXT and tests/ref_graph.py are the contract, under the conventions of vslam_adjust.h and vslam_sim3.h: ALL arithmetic is f64,
 * never fused, in the written order; every 3-term sum is (x + y) + z; there are no floating-point atomics; an item's bits depend on
 * the item alone: the same in every run, batch size and batch slot.
 *
 * ---- vslam_graph_optimize.  An item: N = d_n_nodes nodes, 1 <= N <= node_stride, and E = d_n_edges edges, 0 <= E <= edge_stride.
 * Node i is a camera -> world similarity X_w = s_i R_i X_c + t_i: d_scale [node_stride], d_R [..][9] (row-major), d_T [..][3], f64,
 * IN / OUT; d_fixed [node_stride] int32, != 0 holds the node.  Edge k joins nodes (a, b) = d_edge_ab [edge_stride][2] and carries the
 * measured similarity Z_k = (z_s, Z_R, z_t) = d_edge_scale, d_edge_R [..][9], d_edge_T [..][3], which takes camera a to camera b (B =
 * z_s Z_R A + z_t: exactly what vslam_sim3_ransac writes), and three weights d_edge_weight [..][3] = (w_rot, w_t, w_s).
 *   USABLE.  Edge k < E is usable iff 0 <= a, b < N and a != b; a and b are not both fixed; z_s, Z_R, z_t are finite and z_s > 0; the
 *   three weights are finite and >= 0.  Every other edge is ignored.
 *   RESIDUAL of edge k, 7 values, from the prediction P = S_b^-1 S_a and the error E = Z^-1 P:
 *        s_p = s_a / s_b;   R_p,ij = (Rb_0i Ra_0j + Rb_1i Ra_1j) + Rb_2i Ra_2j;   v = t_a - t_b;
 *        t_p,i = ((Rb_0i v_0 + Rb_1i v_1) + Rb_2i v_2) / s_b;
 *        s_e = s_p / z_s;   R_e,ij = (Z_0i Rp_0j + Z_1i Rp_1j) + Z_2i Rp_2j;   d = t_p - z_t;
 *        t_e,i = ((Z_0i d_0 + Z_1i d_1) + Z_2i d_2) / z_s;
 *        r_0..2 = ((R_e,21 - R_e,12) / 2, (R_e,02 - R_e,20) / 2, (R_e,10 - R_e,01) / 2);   r_3..5 = t_e;   r_6 = s_e - 1.
 *   The rotation part is division-free and has no inverse trigonometry: it is sin(angle) times the axis, so IT VANISHES AGAIN AT 180
 *   DEGREES; a caller's loops are verified measurements a few degrees off, not guesses.
 *   COST.  The sum over the usable edges of (w_rot ((r_0 r_0 + r_1 r_1) + r_2 r_2) + w_t ((r_3 r_3 + r_4 r_4) + r_5 r_5)) + w_s (r_6
 *   r_6).  THERE IS NO ROBUST LOSS: a caller verifies its loops with vslam_sim3_ransac first.
 *   UPDATE.  A node's update is d = (w, tau, sigma): R' = exp([w]x) R as vslam_refine_pairs forms it, t' = t + tau, s' = s (1 +
 *   sigma): vslam_sim3_refine's update.  A candidate with an s' that is not > 0 is refused like a failed solve.
 *   JACOBIANS at d = 0, J_a and J_b (7 x 7, rows the residuals, columns d_a and d_b), from four blocks; k1 = (k + 1) mod 3, k2 = (k +
 *   2) mod 3:
 *        Q_ij   = (Z_0i Rb_j0 + Z_1i Rb_j1) + Z_2i Rb_j2                                        (Z_R^t R_b^t)
 *        D^k_mn = Q_m,k2 Ra_k1,n - Q_m,k1 Ra_k2,n                                               (Q [e_k]x R_a, six entries used)
 *        A_0k = (D^k_21 - D^k_12) / 2;  A_1k = (D^k_02 - D^k_20) / 2;  A_2k = (D^k_10 - D^k_01) / 2
 *        T_ij   = (Q_ij / s_b) / z_s
 *        Bw_ik  = -(((Q_i,k2 v_k1 - Q_i,k1 v_k2) / s_b) / z_s)
 *        bs_i   = -(((Z_0i tp_0 + Z_1i tp_1) + Z_2i tp_2) / z_s)
 *        J_a: rows 0..2 x columns 0..2 = A; rows 3..5 x columns 3..5 = T; (6, 6) = s_e; zero elsewhere.
 *        J_b: rows 0..2 x columns 0..2 = -A; rows 3..5 x columns 0..2 = Bw; rows 3..5 x columns 3..5 = -T; rows 3..5 x column 6 = bs;
 *             (6, 6) = -s_e; zero elsewhere.
 *   NORMAL EQUATIONS.  With W = (w_rot x 3, w_t x 3, w_s): an edge adds to the block H (k <= l, 28 sums) and the gradient g (7 sums)
 *   of its free node on side c the sums over the rows i = 0 .. 6, left to right, of (W_i J_c,ik) J_c,il and of (W_i J_c,ik) r_i.  A
 *   node's sums run over its incident usable edges in ASCENDING EDGE INDEX, from zero; the adjacency is built on the device stably,
 *   by edge index (counts, a scan, a fill).  Only the diagonal blocks are formed: the solve is matrix-free.
 *   OUTER ITERATION: vslam_resect.h's schedule.  lambda starts at 1e-3; the damping is lambda max(H_jj, 2^-40) on the diagonal; a
 *   step is accepted iff the cost is strictly lower, then lambda = max(lambda / 10, 1e-15) and the run stops at a relative decrease
 *   (cost - cost') / cost < 2^-40; a refused step sets lambda = 10 lambda and the run stops above 1e12; at most max_iterations.
 *   START.  Every free node's R is lm_polar_step's result (R (3 I - R^t R) / 2); s and t are kept as given.
 *   INNER SOLVE: preconditioned conjugate gradient on (H + lambda D) x = -g over the ACTIVE nodes -- free with at least one usable
 *   edge; every vector of another node is zero --, block-Jacobi.
 *      The preconditioner M is the damped diagonal blocks, factored once per outer iteration (Cholesky, vslam_resect.h's, 7 x 7); a
 *      pivot that is not > 0 refuses the step.
 *      x = 0, r = -g, z = M^-1 r, p = z, rho = r . z, rho_0 = rho.  Each iteration:
 *        per usable edge  dw = p_a,0..2 - p_b,0..2;  dt = p_a,3..5 - p_b,3..5;
 *                         y_i     = w_rot ((A_i0 dw_0 + A_i1 dw_1) + A_i2 dw_2)                                       i < 3
 *                         y_3+i   = w_t (((T_i0 dt_0 + T_i1 dt_1) + T_i2 dt_2) + ((((Bw_i0 pb_0 + Bw_i1 pb_1) + Bw_i2 pb_2)) + bs_i pb_6))
 *                         y_6     = w_s (s_e (p_a,6 - p_b,6))              (y = W (J_a p_a + J_b p_b); a fixed side's p is zero)
 *        per active node  q = the sum over its edges in ascending index, from zero, of J_side^t y:
 *                         side a:  o_k = (A_0k y_0 + A_1k y_1) + A_2k y_2;  o_3+k = (T_0k y_3 + T_1k y_4) + T_2k y_5;  o_6 = s_e y_6
 *                         side b:  ((Bw_0k y_3 + Bw_1k y_4) + Bw_2k y_5) - o_k;   -o_3+k;   ((bs_0 y_3 + bs_1 y_4) + bs_2 y_5) - o_6
 *                         and then q_j = q_j + (lambda max(H_jj, 2^-40)) p_j.
 *        alpha = rho / (p . q).  A p . q that is not > 0 or not finite ends the solve with the current x, or refuses the step in the
 *        first iteration.
 *        x = x + alpha p;  r = r - alpha q;  z = M^-1 r;  rho' = r . z.
 *        Stop when rho' <= cg_tolerance rho_0 or after cg_iterations; otherwise p = z + (rho' / rho) p and rho = rho'.
 *      SUMS.  A dot product is over the nodes i < N, a node's 7 terms left to right; the cost is over the edges k < E.  Both are
 *      formed as vslam_resect_poses forms its sums: lane l of 256 adds its units l, l + 256, ... in ascending order from zero, then
 *      VsBlockReduce's butterfly and the four wave sums in wave order.
 *   LEFT ALONE -- d_scale, d_R, d_T keep their bits, statistics 1 .. 3 are NaN --: N or E out of range (statistic 0 is then 0); a
 *   node i < N that is not finite or has s not > 0; no fixed node; no usable edge; no accepted step; a result that is not finite.
 *   WHERE IT MOVED only the ACTIVE nodes are written.  Every other node keeps its bits, the padding from N on included.
 *   d_stats [4] f64 (may be NULL): [0] the number of usable edges, [1] cost / usable edges under the start, [2] the same under the
 *   result, [3] the accepted steps.
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (params and d_stats may be); batch, node_stride or
 * edge_stride not positive; parameters out of range (below); an f64 array or d_edge_ab off 8 bytes, another array off 4.
 * VSLAM_ERR_CAPACITY: node_stride > VSLAM_GRAPH_MAX_NODES or edge_stride > VSLAM_GRAPH_MAX_EDGES.
 * ONE launch, one workgroup of 256 per item, stream-ordered on the context, no synchronisation.  The workspace comes from the
 * context's grow-only arena: per item 1008 node_stride + 372 edge_stride + 16 bytes, rounded up to a multiple of 8 (per node: two
 * copies of the nodes, H, its factor, g and the five CG vectors, 124 f64, and four int32; per edge: A, T, Bw, bs, s_e, r and y, 45
 * f64, and three int32).  The kernel's LDS is static and small (the reductions and the adjacency's scan); the vectors stay in L2.
 *
 * ---- vslam_world_close_loops: the same on a world ATTACHED to `map` (vslam_map_attach_world); it does not run behind a step.
 * `loops` items on the device: d_track, d_frame_a, d_frame_b, d_use [loops] int32 and the camera a -> camera b model d_scale [loops],
 * d_R [..][9], d_T [..][3] f64 of a same-track item of vslam_world_sim3.  seq_weight [3] and loop_weight [3] (HOST, NULL: 1 1 1) are
 * the weights of the two kinds of edges.  Per track with F frames recorded, one graph:
 *   node f = (1, the rotation block W_f of d_Twc[f], its centre C_f); node 0 is fixed.
 *   edges 0 .. F - 2 are sequential, f -> f + 1, measured from the world as it stands: z_s = 1, Z_R,ij = (W'_0i W_0j + W'_1i W_1j) +
 *   W'_2i W_2j, z_t,i = (W'_0i c_0 + W'_1i c_1) + W'_2i c_2 with W' = W_f+1 and c = C_f - C_f+1.  THE TRANSPOSE STANDS FOR THE
 *   INVERSE, as in vslam_sim3.h.
 *   then the TAKEN loops of that track, in list order: use != 0, track in 0 .. tracks - 1, the two frames distinct and in 0 .. F - 1,
 *   (s, R, t) finite and s > 0; edge (frame_a, frame_b) with that model.  At most VSLAM_GRAPH_MAX_EDGES - (F - 1) are taken.  A track
 *   without a taken loop is left alone.
 *   WRITE-BACK, only where the item moved, for every written frame f (s_f, R_f, t_f the node's result):  d_Twc gets R_f and t_f, row
 *   3 kept;  d_pose is the same rounded once;  d_scale[f] = d_scale[f] s_f.  Valid d_carry rows (d_carry_index >= 0) are multiplied
 *   by s_F-1 when the last frame was written.  Every d_world_points row i below the map's d_sizes whose x, y, z are finite moves with
 *   its ANCHOR, the frame of the first observation of point i in the map's own log (vslam_map_observations' CSR; vslam_map_step
 *   pushes (last frame, first) first, and the world lifts a pair's points with Twc of that frame): with W, C of the anchor from
 *   before the call, Y_i = (W_0i D_0 + W_1i D_1) + W_2i D_2 of D = X - C, X'_r = s_f ((R_f,r0 Y_0 + R_f,r1 Y_1) + R_f,r2 Y_2) + t_f,r in
 *   f64, rounded once, w kept.  NaN rows, points without an observation, points whose anchor is out of range and points whose anchor
 *   was not written keep their bits.  d_links, d_fuse_to, the resection's statistics and every array of the map keep their bits;
 *   vslam_world_reset undoes the call.
 *   d_stats [tracks][4] (may be NULL) as above; a track without a taken loop gets (0, NaN, NaN, NaN).
 * Launches: the map's CSR, a gather, the kernel above, a scatter.  Refusals: VSLAM_ERR_INVALID for a null pointer (seq_weight,
 * loop_weight, params and d_stats may be), a world that is not the one attached to that map, loops not positive, weights that are
 * not finite or negative, parameters out of range, d_scale, d_R, d_T or d_stats off 8 bytes, another array off 4; VSLAM_ERR_CAPACITY
 * when the frames recorded exceed VSLAM_GRAPH_MAX_NODES.
 *
 * Left open: a robust loss on the edges; graphs across tracks (merging stays vslam_world_apply_sim3's); a stronger preconditioner
 * than block-Jacobi, e.g. block-tridiagonal along the chain -- the CG iterations grow with the length of the track --; running
 * behind a step; a policy for accepting loops.                                                                                   */
#ifndef VSLAM_GRAPH_H
#define VSLAM_GRAPH_H

#include "vslam_amd.h"

#define VSLAM_GRAPH_MAX_NODES 4096
#define VSLAM_GRAPH_MAX_EDGES 8192

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vslam_graph_params {
    int32_t max_iterations;   /* 1 .. 64                               */
    int32_t cg_iterations;    /* 1 .. 8192                             */
    double  cg_tolerance;     /* in (0, 1)                             */
} vslam_graph_params;
/* {20, 2048, 1e-8} */
int vslam_graph_params_default(vslam_graph_params *out);

int vslam_graph_optimize(vslam_ctx *ctx,
        double *d_scale, double *d_R, double *d_T,                 /* [batch][node_stride], [..][9], [..][3]: IN / OUT             */
        const int32_t *d_fixed, const int32_t *d_n_nodes,          /* [batch][node_stride], [batch]                                */
        int batch, int node_stride,
        const int32_t *d_edge_ab,                                  /* [batch][edge_stride][2]                                      */
        const double *d_edge_scale, const double *d_edge_R, const double *d_edge_T,   /* [batch][edge_stride], [..][9], [..][3]    */
        const double *d_edge_weight,                               /* [batch][edge_stride][3]                                      */
        const int32_t *d_n_edges, int edge_stride,
        const vslam_graph_params *params /* NULL: defaults */, double *d_stats /* [batch][4] or NULL */);

int vslam_world_close_loops(vslam_ctx *ctx, vslam_world *world, vslam_map *map,
        const int32_t *d_track, const int32_t *d_frame_a, const int32_t *d_frame_b, const int32_t *d_use,   /* [loops]              */
        const double *d_scale, const double *d_R, const double *d_T, int loops,                             /* [loops], [..][9], [..][3] */
        const double *seq_weight, const double *loop_weight /* HOST [3], NULL: 1 1 1 */,
        const vslam_graph_params *params /* NULL: defaults */, double *d_stats /* [tracks][4] or NULL */);

#ifdef __cplusplus
}
#endif

#endif
