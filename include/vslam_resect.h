/* Tracking against the map: a pose-only adjustment of a camera from 3-D / 2-D correspondences (a resection), as a batch entry of
 * its own and as an opt-in stage of the world frame (include/vslam_amd.h, "the world frame").  Default off: a world without
 * vslam_world_set_resection runs no launch of this file and keeps every bit of its outputs.
 *
 * THIS TEXT and tests/ref_resect.py are the contract.  ALL arithmetic is f64, never fused; f32 inputs are widened first.  A sum
 * over correspondences is formed as vslam_refit_fundamental forms its sums: lane l of 256 adds items l, l + 256, ... in ascending
 * order, a butterfly inside each wave, then the four wave sums in wave order; no floating-point atomics.  An item's bits depend on
 * the item alone: the same in every run, batch size and batch slot.
 *
 * The adjustment.  An item has n correspondences (P_i, x_i) -- a point in the coordinates of the LAST camera and the keypoint it
 * was seen at in the CURRENT image --, the camera matrix K and a start (R, T) taking last-camera coordinates to the current
 * camera.  Projection and A(Y) = d(u, v) / dY are vslam_refine_pairs' (q = K Y row by row, (u, v) = (q0 / q2, q1 / q2), A =
 * (K_row0 - u K_row2, K_row1 - v K_row2) / q2).  Y = R P + T with RP_r = (R_r0 x + R_r1 y) + R_r2 z and Y_r = RP_r + T_r;
 * r = (u, v) - x; e = sqrt(r0 r0 + r1 r1).
 *   1. start   R0 = R (3 I - R^t R) / 2 (the refinement's step towards a rotation), T0 = T, lambda = 1e-3 at the start of every
 *              round.
 *   2. objective over a round's participants: the sum of rho(e), rho = e e for e <= delta and (2 delta) e - delta delta
 *              otherwise; delta = huber_px (default 2, the square root of the reference's thresholdSq = 4).
 *   3. one iteration: w = 1 (e <= delta) or delta / e at the current iterate; J = A(Y) [ -[RP]x | I ] (2 x 6: columns 0..2
 *              A_r2 RP_1 - A_r1 RP_2, A_r0 RP_2 - A_r2 RP_0, A_r1 RP_0 - A_r0 RP_1; columns 3..5 A_r0..2); a correspondence adds
 *              w (J_0k J_0l + J_1k J_1l) to H_kl (k <= l, 21 sums) and w (J_0k r0 + J_1k r1) to g_k (6 sums).  Damping:
 *              H_kk + lambda max(H_kk, 2^-40).  (H) d = -g by Cholesky; a pivot that is not > 0 or a d that is not finite
 *              refuses the step.
 *   4. candidate R' = exp([d_0..2]x) R exactly as vslam_refine_pairs forms it, T' = T + d_3..5; accepted iff every participant
 *              has Y'_z > 0 and the objective is strictly lower.  Accepted: lambda = max(lambda / 10, 1e-15), and the round ends
 *              when (old - new) / old < 2^-40.  Refused: lambda = 10 lambda, and the round ends when lambda > 1e12.  A round
 *              takes at most max_iterations iterations (1 .. 64, default 20).
 *   5. rounds (1 .. 4, default 3): round 0 runs over all n.  The participants of each later round are the correspondences with
 *              Y_z > 0 and e <= gate_px under the previous round's result (default 6 = 3 delta: the prototype's choice on
 *              synthetic scenes, not tuned on real data); the round starts from that result.  A round with fewer than min_links
 *              participants (>= 6, default 8) ends the run with the previous round's result.
 *   6. left alone, outputs equal to the inputs bit for bit: n < min_links; a non-finite K, R, T, or P_i, x_i with i < n; no
 *              accepted step in any round; a result or a statistic that is not finite.
 * stats [4] f64 per item: [0] the participants of the last round that ran (n when none did), [1] the mean of rho over them under
 * the start (R0, T0), [2] the same under the result, [3] the accepted steps of all rounds; [1..3] are NaN for an item left alone.
 *
 * Alignment of device pointers (VSLAM_ERR_INVALID before anything is queued, as everywhere in vslam_amd.h): d_xy, d_xy_cur and
 * d_matches 8 bytes, d_points4d 16, the f64 arrays (d_points, d_R and d_T of vslam_resect_poses, d_stats) 8, every other array 4. */
#ifndef VSLAM_RESECT_H
#define VSLAM_RESECT_H

#include "vslam_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vslam_resect_params {
    int32_t max_iterations;   /* per round, 1 .. 64                                   */
    int32_t rounds;           /* 1 .. 4                                               */
    int32_t min_links;        /* >= 6                                                 */
    double huber_px;          /* delta: > 0 and finite                                */
    double gate_px;           /* > 0 and finite                                       */
} vslam_resect_params;
/* {20, 3, 8, 2.0, 6.0} */
int vslam_resect_params_default(vslam_resect_params *out);

/* The adjustment for a batch of independent items: d_points [batch][stride][3] f64, d_xy [batch][stride][2] f32, d_n [batch]
 * (clamped to 0 .. stride), h_K [9] f32 on the host (row-major), params (NULL: the defaults), d_R [batch][9] and d_T [batch][3]
 * f64 IN / OUT, d_stats [batch][4] f64 or NULL.  stride <= VSLAM_MAX_KP (VSLAM_ERR_CAPACITY).  One launch, stream-ordered on the
 * context, nothing allocated.                                                                                              */
int vslam_resect_poses(vslam_ctx *ctx, const double *d_points, const float *d_xy, const int32_t *d_n, int batch, int stride,
                       const float *h_K, const vslam_resect_params *params, double *d_R, double *d_T, double *d_stats);

/* ---- in the world frame
 * With resection set, the step for frame f also takes the current frame's keypoints d_xy_cur [tracks][kp_stride][2] and h_K.
 *   links   as in vslam_amd.h; the correspondences of the resection are the links whose d_xy_cur[second] is finite, in match
 *           order: (carry[first], xy_cur[second]).  d_links stays L, the count of links.
 *   scale   s0 = the step's scale as in vslam_amd.h (the median path is unchanged).
 *   the resection runs from (R, s0 t), R and t widened, s0 t_k one product each.
 *   where it moves the pose: Twc_f = Twc_(f-1) * [R'^t | -(R'^t T')], (R'^t T')_i = ((R'_0i T'_0 + R'_1i T'_1) + R'_2i T'_2), the
 *           product written out as the plain step's; s_f = sqrt((T'_0 T'_0 + T'_1 T'_1) + T'_2 T'_2); the new carry of a usable
 *           match is R' (s_f X) + T', row r = ((R'_r0 (s_f x) + R'_r1 (s_f y)) + R'_r2 (s_f z)) + T'_r.  Which matches are
 *           usable and which of two wins a keypoint is decided as in the plain step, under the pair's own R, t.
 *   where the item is left alone, and for a pair without a winner, the step is the plain step's bit for bit.
 *   the lift is unchanged: it uses Twc_(f-1) and s_f, so new points keep the resected baseline's unit.
 * Shape: the plain step kernel writes the new carry into a second table, a second kernel (one workgroup of 256 per track, one
 * launch for all tracks) reads the old carry and s0 and overwrites Twc_f, pose_f, scale_f and the new carry's values, then the
 * two tables change places: vslam_world_view's d_carry / d_carry_index are those of the latest step and change from step to step.
 *
 * vslam_world_set_resection: params != NULL sets (and allocates the second table and the statistics, once), NULL clears.  Allowed
 * only at frame 0 (after vslam_world_create / _reset), VSLAM_ERR_INVALID otherwise.                                          */
int vslam_world_set_resection(vslam_world *world, const vslam_resect_params *params);
/* vslam_world_step's arguments, then d_xy_cur (8-byte aligned) and h_K [9] f32 on the host.  VSLAM_ERR_INVALID when resection is
 * not set; vslam_world_step on a world with resection set is VSLAM_ERR_INVALID as well.  A step beyond max_frames does nothing
 * and raises the sticky error word.                                                                                         */
int vslam_world_step_resect(vslam_ctx *ctx, vslam_world *world, const int32_t *d_matches, const int32_t *d_best,
                            const float *d_points4d, const float *d_R, const float *d_t, const int32_t *d_n_last,
                            const int32_t *d_n_cur, const float *d_xy_cur, const float *h_K);
/* *d_stats: [tracks][max_frames][4] f64, the statistics of each step's resection (frame 0 and a pair without a winner:
 * 0, NaN, NaN, NaN); NULL while resection has never been set.  vslam_world_arrays keeps its layout.                          */
int vslam_world_resection_view(vslam_world *world, double **d_stats);
/* A map with such a world attached (vslam_map_attach_world) runs the resecting step behind each map step, with the step's own
 * d_xy_cur and h_K.                                                                                                         */

#ifdef __cplusplus
}
#endif

#endif
