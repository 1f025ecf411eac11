/* Each track -- a point with its list of observations -- triangulated from ALL its observations: a batch entry point for a caller's
 * own problem and its call on a world.  Explicit calls: nothing in vslam_amd.h, vslam_resect.h, vslam_adjust.h, vslam_search.h,
 * vslam_pnp.h or vslam_fuse.h launches a kernel of this file while they are unused, and no existing output changes a bit.
 *
 * Why.  vslam_world_fuse (vslam_fuse.h) merges the map's duplicate points into tracks of three to four observations, but a
 * survivor keeps the position one two-view triangulation of its oldest pair gave it, in that pair's own scale estimate.  Only
 * vslam_world_adjust moves a point by its merged list, for one window of frames.  This is the step between "tracks exist" and
 * bundle adjustment: every track triangulated from all its views, refused without parallax, refused where the result lies behind
 * a camera or its own observations do not support it.
 *
 * THIS TEXT and tests/ref_tracks.py are the contract.  ALL arithmetic is f64, never fused; f32 inputs are widened first; only + -
 * x / sqrt are used; every sum runs in observation order (the order of the point's CSR row) from 0.  An item's bits depend on the
 * item alone -- a point's on the point alone --: the same in every run, batch size and batch slot.
 *
 * ---- vslam_triangulate_tracks
 * An item, exactly as vslam_cull_points (vslam_fuse.h) takes it.  n points (d_points rows [x y z w] f32, w is not read), n =
 * d_n_points clamped to 0 .. pt_stride; their observations in CSR by point: d_obs_offsets [pt_stride + 1], the observations of
 * point i are rows offsets[i] .. offsets[i + 1] - 1 of d_obs_cam / d_obs_kp [obs_stride] (a camera and a keypoint of it); C cameras
 * taking the points' coordinates to the camera, d_R [cam_stride][9] row-major and d_T [cam_stride][3] f64, C = d_n_cams clamped
 * to 0 .. cam_stride; the cameras' keypoints d_xy [cam_stride][kp_stride][2] f32; h_K (row-major f32), K = h_K widened.
 *   Point i TAKES PART iff i < n and 0 <= offsets[i] < offsets[i + 1] <= obs_stride.  A finite position is NOT required: the point's
 *   own row is only compared against (WORSE, below), never started from.
 *   Kinv, once per call on the host in f64: c00 = K4 K8 - K5 K7, c01 = K2 K7 - K1 K8, c02 = K1 K5 - K2 K4, c10 = K5 K6 - K3 K8, c11 =
 *   K0 K8 - K2 K6, c12 = K2 K3 - K0 K5, c20 = K3 K7 - K4 K6, c21 = K1 K6 - K0 K7, c22 = K0 K4 - K1 K3; det = (K0 c00 + K1 c10) + K2
 *   c20; Kinv_ij = c_ij / det.
 *   An observation (cam, kp) with keypoint (x, y) has the RAY b_r = (Kinv_r0 x + Kinv_r1 y) + Kinv_r2, d'_k = (R_0k b_0 + R_1k b_1) +
 *   R_2k b_2 (d' = R^t b), nn = (d'_0 d'_0 + d'_1 d'_1) + d'_2 d'_2, d = d' / sqrt(nn) entry by entry, and the CENTRE c_r = -((R_0r T_0
 *   + R_1r T_1) + R_2r T_2) (c = -R^t T, the order in which vslam_adjust.h writes M'[4 r + 3]).
 *   An observation is USABLE iff 0 <= cam < C, 0 <= kp < kp_stride, that camera's R and T are finite, the keypoint's x, y are finite
 *   (so far vslam_cull_points' USABLE), and its ray is finite: d' is finite and nn > 0, which is exactly when d is.  m = the usable
 *   observations of the point; "the observations" below are the usable ones, in row order.
 *   dot(a, b) = (a0 b0 + a1 b1) + a2 b2.
 * The status of a point is that of the FIRST rule that applies:
 *   -1  the point took no part (n <= i < pt_stride included).
 *    1  TOO_FEW: m < 2.
 *    2  LOW_PARALLAX.  j0 = the first observation; j1 = the observation with the smallest dot(d_j0, d_j), the first one on ties (j0
 *       itself is among the candidates); cos_parallax = the smallest dot(d_j1, d_j) over all observations j (j1 among them).  The
 *       point is refused unless cos_parallax <= cos_parallax_max.  Two walks of the row, O(m): the angle found is at least half the
 *       largest angle between any two rays of the row (the farthest ray from j0 is at least half that angle away from j0, and j1's
 *       farthest is no nearer), and exactly the largest for m = 2.
 *    3  DEGENERATE: the linear start failed.  With M = I - d d^t written as M00 = 1 - d0 d0, M01 = -(d0 d1), M02 = -(d0 d2), M11 = 1 -
 *       d1 d1, M12 = -(d1 d2), M22 = 1 - d2 d2: A = sum M (six sums: 00 01 02 11 12 22) and r = sum M c, (M c)_0 = (M00 c0 + M01 c1)
 *       + M02 c2, (M c)_1 = (M01 c0 + M11 c1) + M12 c2, (M c)_2 = (M02 c0 + M12 c1) + M22 c2 (three sums); X0 = A^-1 r by the Cholesky
 *       factorisation of vslam_adjust.h's step 1 with lambda = 0 (V* = A), L then L^t.  The status applies to a pivot that is not
 *       > 0 or an X0 that is not finite.  (X0 is the point nearest to all rays taken as whole lines.)
 *       The refinement -- not a status.  It starts at X0, NEVER at the input row: the result does not inherit the survivor's stale
 *       position.  One observation under X as vslam_adjust.h writes it: Y = R X + T, (u, v), r, e, A = d(u, v) / dY, Jx = A R, rho
 *       and the weight w with delta = huber_px.  At an iterate X: cost(X) = sum of rho(e) over the observations with Y_z > 0;
 *       behind(X) = some observation has !(Y_z > 0); V = sum of V_o = w Jx^t Jx (upper 6) and g = sum of gx_o = w Jx^t r over the same
 *       observations as the cost, w taken at X.  lambda = 1e-3.  `iterations` times: V* = V + lambda max(V_jj, 2^-40) on the diagonal
 *       = L L^t, z = V*^-1 g, the candidate X' = X + (-z); the step is ACCEPTED iff no pivot failed, X' is finite, !behind(X') and
 *       cost(X') < cost(X) (false for a NaN).  Accepted: X = X', lambda = max(lambda / 10, 1e-15), and the loop ends when (old - new)
 *       / old < 2^-40.  Refused: X stays, lambda = 10 lambda, and the loop ends when lambda > 1e12 -- vslam_adjust.h's schedule for a
 *       point.  The count is fixed by `iterations`; the two early ends depend on the point's own values only.  iterations = 0
 *       leaves X = X0.  cost_out = cost(X) at the end.
 *    4  BEHIND: behind(X) at the result.
 *    5  UNSUPPORTED.  An observation is GOOD at X exactly as in vslam_cull_points (Y_z > 0, (u, v) finite, r0 r0 + r1 r1 <= inlier_px
 *       inlier_px, a closed disc, the right side one product).  The point is refused unless n_good >= min_good and 10 n_good >=
 *       good10 m.
 *    6  WORSE: the input row's x, y, z are finite, cost_in is finite and cost_out > cost_in, where cost_in = cost(input row, widened),
 *       or +inf when behind(input row).
 *    0  OK.
 * Outputs, for EVERY i < pt_stride.  d_out_points: status 0: X rounded once to f32 and w = 1; any other status: the input row's
 * four words bit for bit.  d_status.  d_counts [pt_stride][2] or NULL: m and n_good (n_good is 0 for a status of -1, 1, 2, 3; m is
 * 0 for -1).  d_info [pt_stride][3] f64 or NULL: cos_parallax, cost_in, cost_out, each the quiet NaN 0x7FF8000000000000 where the
 * point's status came before the value was formed: all three for -1 and 1, the costs for 2 and 3; cost_in also for an input row
 * that is not finite.  d_stats [4] int32 per item: the points taking part, OK, LOW_PARALLAX, every other refusal (integer sums:
 * the order of arrival does not matter).
 * d_out_points may be d_points itself (a row is read before it is written, by the one lane that owns it); no other overlap of an
 * output with an input or another output is allowed.
 * The call is pure: it writes nothing but its outputs.  One launch (one lane per point) behind one fill of d_stats; no workspace;
 * stream-ordered on the context, no synchronisation.
 * vslam_track_params {cos_parallax_max, huber_px, inlier_px, iterations, min_good, good10}, defaults {0.9998, 2.0, 6.0, 10, 2, 5}:
 * 0.9998 is the cosine of about 1.15 degrees; huber_px and inlier_px are vslam_adjust_params' huber_px and gate_px; half of what a
 * point has must be good.  THESE VALUES ARE UNTUNED: they have been run on synthetic scenes only.
 *
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (params, d_counts and d_info may be); batch, pt_stride,
 * obs_stride, cam_stride or kp_stride not positive; cos_parallax_max not finite or outside (-1, 1]; huber_px or inlier_px not finite
 * or not > 0; iterations outside 0 .. 64; min_good < 2; good10 outside 0 .. 10; a non-finite h_K, a determinant that is 0 or not
 * finite, an entry of Kinv that is not finite; d_points or d_out_points off 16 bytes, d_xy, d_R, d_T or d_info off 8, another array
 * off 4.  VSLAM_ERR_CAPACITY: kp_stride > VSLAM_MAX_KP or cam_stride > 1024.
 *
 * ---- on the world: vslam_world_retriangulate, an explicit call for a world ATTACHED to `map` (vslam_map_attach_world); it never runs
 * behind a step.  It runs vslam_triangulate_tracks in place on d_world_points with n = d_sizes, the CSR the world's (vslam_fuse.h,
 * "THE WORLD'S CSR": the merged lists once a fusion exists, the map's own otherwise; pt_stride = map_capacity, obs_stride =
 * obs_capacity), camera f = recorded frame f formed from d_Twc as vslam_adjust.h forms "camera c" (C = the frames recorded,
 * cam_stride = max_frames) and d_xy the keypoints of every frame in the layout vslam_world_cull takes ([tracks][xy_frames][kp_stride]
 * [2], xy_frames >= the frames recorded).  Only the rows with status 0 are written.  d_fuse_to and the fusion state, d_Twc, d_pose,
 * the carry (it lives in the last camera's frame, and no camera moves), d_scale, d_links and every array of the map and its log keep
 * their bits.  An absorbed or culled point has an empty row, takes no part and keeps its NaN row.  vslam_world_reset and
 * vslam_map_reset need nothing new.  d_status [tracks][map_capacity] int32 or NULL; d_stats [tracks][4] int32 or NULL.
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (params, d_status and d_stats may be), a world that is not
 * the one attached to that map or has not as many frames, xy_frames below the frames recorded, parameters out of range, an h_K
 * refused above, d_xy off 8 bytes, d_status or d_stats off 4.  VSLAM_ERR_CAPACITY: max_frames > 1024.
 * Workspace from the context's arena, allocated on the first call of a size and never afterwards: what forms the world's CSR
 * (vslam_fuse.h) plus tracks x (map_capacity + 6 + 2 obs_capacity) x 4 + tracks x max_frames x 96 bytes.
 *
 * Left open: running behind a step (geometric fusing through a search by projection is vslam_fuse_project.h's); tuning on footage; culling by parallax as a
 * policy (here it is only a status: a refused point keeps its row).                                                            */
#ifndef VSLAM_TRACKS_H
#define VSLAM_TRACKS_H

#include "vslam_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_TRACK_NO_PART (-1)
#define VSLAM_TRACK_OK 0
#define VSLAM_TRACK_TOO_FEW 1
#define VSLAM_TRACK_LOW_PARALLAX 2
#define VSLAM_TRACK_DEGENERATE 3
#define VSLAM_TRACK_BEHIND 4
#define VSLAM_TRACK_UNSUPPORTED 5
#define VSLAM_TRACK_WORSE 6

typedef struct vslam_track_params {
    double  cos_parallax_max;   /* in (-1, 1]: a point whose widest pair of rays found has a larger cosine is refused */
    double  huber_px;           /* delta: > 0, finite                                                                 */
    double  inlier_px;          /* > 0, finite                                                                        */
    int32_t iterations;         /* 0 .. 64 Levenberg-Marquardt steps; 0: the linear start                             */
    int32_t min_good;           /* >= 2: good observations a point needs                                              */
    int32_t good10;             /* 0 .. 10: tenths of a point's usable observations that must be good                 */
} vslam_track_params;
/* {0.9998, 2.0, 6.0, 10, 2, 5} */
int vslam_track_params_default(vslam_track_params *out);

int vslam_triangulate_tracks(vslam_ctx *ctx,
        const float *d_points, const int32_t *d_n_points, int pt_stride,          /* [batch][pt_stride][4] f32, w not read    */
        const int32_t *d_obs_offsets, const int32_t *d_obs_cam, const int32_t *d_obs_kp, int obs_stride,
        const double *d_R, const double *d_T, const int32_t *d_n_cams, int cam_stride,   /* [batch][cam_stride][9], [..][3], [batch] */
        const float *d_xy, int kp_stride,                                         /* [batch][cam_stride][kp_stride][2] f32    */
        const float *h_K, int batch, const vslam_track_params *params /* NULL: defaults */,
        float *d_out_points,                                                      /* [batch][pt_stride][4] f32; may be d_points */
        int32_t *d_status,                                                        /* [batch][pt_stride]                       */
        int32_t *d_counts /* [batch][pt_stride][2] or NULL */, double *d_info /* [batch][pt_stride][3] or NULL */,
        int32_t *d_stats /* [batch][4] */);

int vslam_world_retriangulate(vslam_ctx *ctx, vslam_world *world, vslam_map *map,
                              const float *d_xy, int xy_frames,                  /* [tracks][xy_frames][kp_stride][2] f32 */
                              const float *h_K, const vslam_track_params *params /* NULL: defaults */,
                              int32_t *d_status /* [tracks][map_capacity] or NULL */, int32_t *d_stats /* [tracks][4] or NULL */);

#ifdef __cplusplus
}
#endif

#endif
