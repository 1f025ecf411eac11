/* Adjusting a window of cameras and the points they share together (a windowed bundle adjustment), as a batch entry for a caller's
 * own problems and as one explicit call on a world attached to a map (vslam_world_adjust, below).  Explicit calls: nothing in vslam_amd.h or vslam_resect.h launches a kernel of this file, and no existing output
 * changes a bit.
 *
 * THIS TEXT and tests/ref_adjust.py are the contract.  ALL arithmetic is f64, never fused; f32 inputs are widened first.  No
 * floating-point atomics; the order of every sum is stated below and is a function of the item alone (its counts and its CSR as
 * given), so an item's bits are the same in every run, batch size and batch slot.
 *
 * An item.  C cameras (1 <= C <= VSLAM_ADJUST_MAX_CAMS), camera c a world -> camera pose (R_c [9] row-major, T_c [3]); N points
 * X_i [3]; observations in CSR by point, the shape vslam_map_observations produces: the observations of point i are k =
 * offsets[i] .. offsets[i + 1] - 1, observation k was made by camera cam[k] at the keypoint xy[k].  The first n_fixed cameras are
 * held.  With n_fixed = 1 the scale of the whole item is a free direction that only the damping holds: 2 is recommended and is
 * the default.
 *
 * One observation.  Y = R X + T (RX_r = (R_r0 x + R_r1 y) + R_r2 z, Y_r = RX_r + T_r); q = K Y row by row, (u, v) = (q0 / q2,
 * q1 / q2); r = (u, v) - xy; e = sqrt(r0 r0 + r1 r1); A = d(u, v) / dY = (K_row0 - u K_row2, K_row1 - v K_row2) / q2 -- all as
 * in vslam_refine_pairs and vslam_resect_poses.  rho(e) = e e for e <= delta, (2 delta) e - delta delta otherwise (delta =
 * huber_px); w = 1 for e <= delta, delta / e otherwise, taken at the current iterate.  Jx = A R (2 x 3, Jx_rk = (A_r0 R_0k +
 * A_r1 R_1k) + A_r2 R_2k); Jc = A [ -[RX]x | I ] (2 x 6, the columns of the resection).  With B^t M C for a 2-row B, C meaning
 * B_0i C_0j + B_1i C_1j, the observation's blocks are
 *     V_o = w Jx^t Jx (3 x 3, upper 6), gx_o = w Jx^t r (3), U_o = w Jc^t Jc (6 x 6, upper 21), gc_o = w Jc^t r (6),
 *     W_o = w Jc^t Jx (6 x 3)                      -- w times the two-term sum, as vslam_resect_poses forms H and g.
 *
 * Participation is fixed per round (rounds 1 .. 4, default 3).
 *   a. an observation is USABLE when 0 <= cam[k] < C and X_i and xy[k] are finite.  Round 0 takes the usable observations with
 *      Y_z > 0 under the start; a later round those with Y_z > 0 and e <= gate_px (default 6) under the previous round's result.
 *   b. a point takes part iff the observations a. leaves it lie in at least two distinct cameras; otherwise they all drop out.
 *   c. n_c = the participating observations of camera c after b.  Camera c is FREE in the round iff c >= n_fixed and n_c >=
 *      min_obs (>= 6, default 8); every other camera is held for the round (its observations still take part).
 *   d. a round > 0 without a free camera ends the run with the previous round's result (and the previous round's participants).
 *      Round 0 without a free camera leaves the item alone.
 *   The free cameras in ascending order are the SLOTS s = 0 .. F - 1 (F <= 7); unknown 6 s + j is row j of slot s.
 *
 * The iteration (per round: lambda = 1e-3, the objective obj = sum of rho over the participants at the current iterate):
 *   1. per participating point, its observations in CSR order: V = sum V_o, gx = sum gx_o; per slot s the point has observations
 *      in: W_s = sum W_o, U_s = sum U_o, gc_s = sum gc_o (a camera is normally seen once; a second observation by the same camera
 *      adds to the first's blocks).  V* = V + lambda max(V_jj, 2^-40) on the diagonal = L L^t (a pivot that is not > 0 refuses
 *      the step).  z = V*^-1 gx and row j of Y_s = V*^-1 (row j of W_s), each by L then L^t.
 *   2. the reduced system, every entry ONE chain over the points i = 0, 1, .. N - 1 in ascending order (points that do not take
 *      part, or have no observation in the slot(s), are skipped), dot(a, b) = (a0 b0 + a1 b1) + a2 b2:
 *        S[6 s + j][6 s + l]  = sum_i ( U_s[j][l] - dot(Y_s row j, W_s row l) )          Ud[6 s + j] = sum_i U_s[j][j]
 *        S[6 s + j][6 t + l]  = sum_i ( - dot(Y_s row j, W_t row l) ),  s < t
 *        rhs[6 s + j]         = sum_i ( gc_s[j] - dot(W_s row j, z) )
 *      and the damping S[a][a] + lambda max(Ud[a], 2^-40).  (S) dc = -rhs by Cholesky: column j ascending, every sum over k
 *      ascending (p_j = S*_jj - sum_k<j L_jk L_jk; L_ij = (S_ij - sum_k<j L_ik L_jk) / sqrt(p_j)); forward f_i = (rhs_i - sum_k<i
 *      L_ik f_k) / L_ii, back d_i = (f_i - sum_k>i L_ki d_k) / L_ii with k DEscending, dc = -d.  A pivot that is not > 0 or a dc
 *      that is not finite refuses the step.
 *   3. dX_i = -(z + sum_s Y_s^t dc_s), slots ascending, (Y_s^t dc_s)_m = sum_j Y_s[j][m] dc[6 s + j] with j ascending from 0; a
 *      dX that is not finite refuses the step.  Candidate: X' = X + dX for the participating points; R'_c = exp([dc_0..2]x) R_c
 *      exactly as vslam_refine_pairs forms it and T'_c = T_c + dc_3..5 for the free cameras; everything else as it is.
 *   4. accepted iff every participating observation has Y'_z > 0 and the objective is strictly lower.  Accepted: lambda =
 *      max(lambda / 10, 1e-15), the round ends when (old - new) / old < 2^-40.  Refused: lambda = 10 lambda, the round ends when
 *      lambda > 1e12.  At most max_iterations iterations per round (1 .. 64, default 20) -- vslam_resect_poses' schedule.
 *   Sums over the observations (the objective, n_c, the statistics) are formed as vslam_resect_poses forms its sums, with the
 *   POINT as the unit: lane l of 256 adds the observations of points l, l + 256, ... (each point's in CSR order) in ascending
 *   order, a butterfly inside each wave, then the four wave sums in wave order.
 *   The start: R_c (3 I - R_c^t R_c) / 2 for every camera c >= n_fixed (the refinement's step towards a rotation); the first
 *   n_fixed cameras, every T and every X as given.
 *
 * Left alone, outputs equal to the inputs bit for bit: C outside 1 .. cam_stride or N outside 0 .. pt_stride; offsets[0] < 0,
 * decreasing offsets or an offset above obs_stride (within 0 .. N); a non-finite K, R_c or T_c (c < C); no free camera in round 0;
 * no accepted step in any round; a camera, a point or a statistic of the result that is not finite.  Where the item moved, R_c
 * and T_c of every camera that was free in some round and X_i of every point that took part in the LAST round that ran are
 * overwritten; everything else keeps its bits (a point that took part earlier and dropped out keeps its input: what drove it
 * out may have been its own false observations).
 * stats [4] f64 per item: [0] the participating observations of the last round that ran (0 when the counts or offsets are out of
 * range or something is not finite), [1] the mean of rho over them under the start, [2] the same under the result, [3] the accepted
 * steps of all rounds; [1..3] are NaN for an item left alone.
 *
 * Alignment of device pointers (VSLAM_ERR_INVALID before anything is queued, as everywhere in vslam_amd.h): the f64 arrays (d_R,
 * d_T, d_points, d_stats) and d_obs_xy 8 bytes, the int32 arrays (d_n_cams, d_n_points, d_obs_offsets, d_obs_cam) 4. */
#ifndef VSLAM_ADJUST_H
#define VSLAM_ADJUST_H

#include "vslam_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_ADJUST_MAX_CAMS 8

typedef struct vslam_adjust_params {
    int32_t max_iterations;   /* per round, 1 .. 64                                   */
    int32_t rounds;           /* 1 .. 4                                               */
    int32_t min_obs;          /* >= 6: below it a camera is held for the round        */
    int32_t n_fixed;          /* >= 1: the first n_fixed cameras are held             */
    double huber_px;          /* delta: > 0 and finite                                */
    double gate_px;           /* > 0 and finite                                       */
} vslam_adjust_params;
/* {20, 3, 8, 2, 2.0, 6.0} */
int vslam_adjust_params_default(vslam_adjust_params *out);

/* The adjustment for a batch of independent items.  d_R [batch][cam_stride][9] and d_T [batch][cam_stride][3] f64 IN / OUT,
 * d_n_cams [batch]; d_points [batch][pt_stride][3] f64 IN / OUT, d_n_points [batch]; d_obs_offsets [batch][pt_stride + 1],
 * d_obs_cam [batch][obs_stride] int32, d_obs_xy [batch][obs_stride][2] f32; h_K [9] f32 on the host (row-major); params (NULL:
 * the defaults); d_stats [batch][4] f64 or NULL.  VSLAM_ERR_INVALID: a null pointer (d_stats and params may be), a size that is
 * not positive, parameters out of range, a pointer off its alignment.  VSLAM_ERR_CAPACITY: cam_stride > VSLAM_ADJUST_MAX_CAMS.
 * One launch, one workgroup of 256 per item, stream-ordered on the context, no synchronisation.  What it keeps per point and
 * per observation between its passes (two copies of the points, the per-slot blocks of step 1, the participation flags:
 * batch x (pt_stride x 3604 + obs_stride x 2) bytes) comes from the context's grow-only arena: allocated on the first call of a
 * size, never afterwards.                                                                                                   */
int vslam_adjust_windows(vslam_ctx *ctx, double *d_R, double *d_T, const int32_t *d_n_cams, int cam_stride, double *d_points,
                         const int32_t *d_n_points, int pt_stride, const int32_t *d_obs_offsets, const int32_t *d_obs_cam,
                         const float *d_obs_xy, int obs_stride, int batch, const float *h_K, const vslam_adjust_params *params,
                         double *d_stats);

/* ---- on the world: one explicit call that adjusts the last `window` frames of every track of a world ATTACHED to `map`
 * (vslam_map_attach_world) together with the map points they observe.  VSLAM_ERR_INVALID: a null pointer (params and d_stats may
 * be), a world that is not the one attached to that map, window outside 2 .. 8, xy_frames below the frames recorded, d_xy off 8
 * bytes or d_stats off 8, parameters out of range.
 * The problem, per track, with f1 = frames recorded - 1 and f0 = max(0, f1 - window + 1):
 *   camera c   frame f0 + c, from M = d_Twc[track][f0 + c] (camera -> world): R = R_wc^t, R_rc = M[4 c + r]; T_r = -((M[r] M[3] +
 *              M[4 + r] M[7]) + M[8 + r] M[11]).
 *   point i    map point i, i < d_sizes[track], from d_world_points, widened.
 *   observations of point i: those of the map's log (vslam_map_observations' CSR) whose frame lies in f0 .. f1 and whose keypoint
 *              index lies in 0 .. kp_stride - 1, in the log's push order; camera = frame - f0, the keypoint is
 *              d_xy[(track * xy_frames + frame)][keypoint] -- the layout vslam_track_sequences leaves.
 * Launches: the map's CSR (the two launches of vslam_map_observations), then three of this file for all tracks -- the gather,
 * the kernel of vslam_adjust_windows (cam_stride 8, pt_stride map_capacity, obs_stride obs_capacity), the scatter.  Workspace
 * from the context's arena, nothing allocated after the first call of a size, no synchronisation.
 * Write-back, only where the item moved:
 *   d_Twc of every camera that was free in some round: M'[4 r + c] = R'_cr (c < 3), M'[4 r + 3] = -((R'_0r T'_0 + R'_1r T'_1) +
 *              R'_2r T'_2), row 3 = (0, 0, 0, 1); d_pose = M' rounded once to f32.
 *   d_world_points of the points that took part in the last round: X' rounded once to f32, w = 1.
 *   the latest step's carry (vslam_world_view's d_carry, every entry with d_carry_index >= 0), when the LAST camera was written:
 *              w_r = ((M[4 r] p_0 + M[4 r + 1] p_1) + M[4 r + 2] p_2) + M[4 r + 3] with M the last frame's d_Twc BEFORE the call,
 *              then p'_r = ((R'_r0 w_0 + R'_r1 w_1) + R'_r2 w_2) + T'_r.
 *   d_scale, d_links and the resection statistics are records of the steps and keep their bits; so do the map's own arrays.
 * d_stats [tracks][4] f64 or NULL: the statistics of vslam_adjust_windows per track.                                         */
int vslam_world_adjust(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy, int xy_frames, const float *h_K,
                       int window, const vslam_adjust_params *params, double *d_stats);

#ifdef __cplusplus
}
#endif

#endif
