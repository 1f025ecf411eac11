/* The relation between two views of one scene in a monocular world: a similarity B = s R A + t, found by hypothesise-and-count
 * (RANSAC) over 3-D / 3-D correspondences with a 3-point minimal solver, for a batch of independent items, and polished by a
 * 7-parameter Levenberg-Marquardt iteration on the core the other optimizers share.  Every track of a world (vslam_amd.h, "the
 * world frame") has its own origin, orientation and unit, so a rigid pose (vslam_pnp_ransac) cannot relate two of them.  Explicit
 * calls: nothing in the other headers launches a kernel of this file, and no existing output changes a bit.
 *
 * THIS TEXT and tests/ref_sim3.py are the contract, under the conventions of vslam_pnp.h: ALL floating-point arithmetic is f64, never
 * fused, in the written order, with + - * / and sqrt only on the way to every integer output (the polish also uses what
 * vslam_resect_poses uses: the sine of its rotation update); f32 inputs are widened first.  Counts are integers and the choice is
 * one maximum over integer keys, so an item's bits depend on the item alone: the same in every run, batch size and batch slot.
 *
 * An item: n correspondences (A_i, xa_i, B_i, xb_i), n = d_n clamped to 0 .. stride.  A_i is a point in camera a's coordinates and
 * xa_i its keypoint in image a; B_i is the same physical point in camera b's coordinates AND b's unit, xb_i its keypoint in image
 * b.  d_A, d_B [stride][3] f64; d_xa, d_xb [stride][2] f32; the camera matrix K (h_K [9] f32, row-major, on the host) serves both
 * images; a seed.  The model (s, R, t) takes a to b: B = s R A + t.
 *   1. SETS.  The sampler of vslam_pnp.h, step 1, word for word (mix, draw c of hypothesis h, the multiply-shift, repeats
 *      skipped, 16 draws, three distinct indices i0, i1, i2 in sampling order).  One model per hypothesis.
 *   2. MODEL.  From the three pairs p0, p1, p2, with |v|^2 = (x x + y y) + z z and every sum left to right:
 *        c     = ((p0 + p1) + p2) / 3, component by component, on each side: cA, cB;
 *        s     = sqrt(((|B0 - cB|^2 + |B1 - cB|^2) + |B2 - cB|^2) / ((|A0 - cA|^2 + |A1 - cA|^2) + |A2 - cA|^2));
 *        F     the orthonormal frame vslam_pnp.h's P3P builds on three points: e1 = (p1 - p0) / |.|, e3 = (e1 x (p2 - p0)) / |.|,
 *              e2 = e3 x e1; FA on the A side, FB on the B side;
 *        R_ij  = (FB.e1_i FA.e1_j + FB.e2_i FA.e2_j) + FB.e3_i FA.e3_j;
 *        t_r   = cB_r - s ((R_r0 cA_0 + R_r1 cA_1) + R_r2 cA_2).
 *      The two 3 x 4 projection matrices of the count, rows r = 0 .. 2, with (K X)_r = (K_r0 X_0 + K_r1 X_1) + K_r2 X_2 for a
 *      column X:
 *        M_b = K [s R | t]:             column c < 3 is K applied to (s R_0c, s R_1c, s R_2c), one product each; column 3 is K t;
 *        M_a = K [R^t / s | -(R^t t) / s]:  column c < 3 is K applied to (R_c0 / s, R_c1 / s, R_c2 / s); column 3 is K applied to
 *              u, u_i = -(((R_0i t_0 + R_1i t_1) + R_2i t_2) / s).
 *      A model is dropped when s is not finite or not > 0; when an entry of R, t, M_a or M_b is not finite; or when
 *      max |R^t R - I| > 1e-9 ((R^t R)_ij = (R_0i R_0j + R_1i R_1j) + R_2i R_2j).  Collinear or repeated points divide by zero in
 *      a frame or in s and fall to these tests.
 *   3. COUNT.  q = M (X, 1) row by row, q_r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3.  (X, x) passes under M iff q_2 > 0 and
 *      d_0 d_0 + d_1 d_1 <= l l with d_0 = q_0 - x_0 q_2, d_1 = q_1 - x_1 q_2, l = inlier_px q_2, and l l finite: a closed disc
 *      tested WITHOUT a division.  A comparison with a NaN is false.  Correspondence i < n is an inlier iff (A_i, xb_i) passes
 *      under M_b AND (B_i, xa_i) passes under M_a.  Both are needed: reprojection into one image alone leaves the scale about that
 *      camera's centre free.
 *   4. CHOICE.  The largest count wins, ties to the smallest h: the maximum of count << 10 | (1023 - h).  FOUND iff that count >=
 *      min_inliers.  The item is LEFT ALONE -- not found, d_scale / d_R / d_T keep their bits, no hypothesis has a model -- when
 *      n < 4, when a K is not finite, or when an A_i, B_i, xa_i or xb_i with i < n is not finite.
 *   5. OUTPUTS.  d_scale [1], d_R [9], d_T [3] f64: written only for a found item.  d_inlier [stride] int32: 1 / 0 for the winner
 *      below n, 0 from n on and everywhere for an item that is not found.  d_corr_index [stride] (may be NULL): the winner's
 *      inliers compacted in ascending index; slots from the count on keep their bits.  d_n_inliers: their count (0 when not
 *      found).  d_winner: h, or -1.  d_counts [hypotheses] int32 or NULL: every hypothesis' count, -1 where it has no model.
 *      d_stats [4] f64 or NULL: the statistics of the polish; NaN NaN NaN NaN without one.
 *   6. POLISH.  With polish != NULL, vslam_sim3_refine (below) runs behind the choice from the winner's (s, R, t) over the
 *      correspondences of d_inlier, in place on d_scale / d_R / d_T.  The mask, d_corr_index, d_n_inliers and the counts are NOT
 *      recomputed.
 *
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (params, polish, d_corr_index, d_counts and d_stats may
 * be); batch or stride not positive; hypotheses not a multiple of 64 in 64 .. 1024; min_inliers < 4; inlier_px not finite or not
 * > 0; polish parameters vslam_resect_poses would refuse; a pointer off its alignment: the f64 arrays (d_A, d_B, d_scale, d_R,
 * d_T, d_stats), d_xa and d_xb 8 bytes, every other array 4.  VSLAM_ERR_CAPACITY: stride > VSLAM_MAX_KP.
 *
 * Three launches (solve, count, select) and the polish's one, stream-ordered on the context, no synchronisation.  The workspace
 * (every model with its two matrices, 37 f64, and three int32 per hypothesis) comes from the context's grow-only arena: allocated
 * on the first call of a size, never afterwards.  inlier_px and min_inliers are untuned on real footage.
 *
 * ---- vslam_sim3_refine: Levenberg-Marquardt on the 7 unknowns d = (w, tau, sigma) of a similarity (s, R, t), IN / OUT in d_scale
 * [batch], d_R [batch][9], d_T [batch][3].  The correspondences taking part are those i < n with d_mask[i] != 0 (d_mask
 * [batch][stride] int32; NULL: every i < n).  Per correspondence, two observations, formed with vslam_resect.h's transform and
 * projection (q = K Y row by row, (u, v) = (q_0 / q_2, q_1 / q_2)):
 *      direction b:  RA_r = (R_r0 x + R_r1 y) + R_r2 z of A;  W = s RA (one product each);  Y_b = W + t;  r_b = (u, v) - xb;
 *      direction a:  D = B - t;  Y_a,r = ((R_0r D_0 + R_1r D_1) + R_2r D_2) / s;  r_a = (u, v) - xa;
 *      e = sqrt(r_0 r_0 + r_1 r_1) for each; the cost is the sum over the participants of rho(e_b) + rho(e_a), rho Huber's as in
 *      vslam_resect.h.
 * The update: R' = exp([w]x) R exactly as vslam_refine_pairs forms it, t' = t + tau, s' = s (1 + sigma) (no exponential); a
 * candidate whose s' is not > 0 is refused like a failed solve.  The Jacobian's columns at d = 0, with A(Y) = d(u, v) / dY of
 * vslam_resect.h for each direction (rows r = 0, 1; a_k = A_rk):
 *      J_b: columns 0..2  a_2 W_1 - a_1 W_2,  a_0 W_2 - a_2 W_0,  a_1 W_0 - a_0 W_1;   columns 3..5  a_0, a_1, a_2;
 *           column 6      (a_0 W_0 + a_1 W_1) + a_2 W_2.
 *      J_a: with N = (a_2 Y_1 - a_1 Y_2,  a_0 Y_2 - a_2 Y_0,  a_1 Y_0 - a_0 Y_1), Y = Y_a:
 *           column k < 3  -((N_0 R_k0 + N_1 R_k1) + N_2 R_k2);   column 3 + k  -(((a_0 R_k0 + a_1 R_k1) + a_2 R_k2) / s);
 *           column 6      -((a_0 Y_0 + a_1 Y_1) + a_2 Y_2).
 * A correspondence adds w_b (Jb_0k Jb_0l + Jb_1k Jb_1l) + w_a (Ja_0k Ja_0l + Ja_1k Ja_1l) to H_kl (k <= l, 28 sums) and
 * w_b (Jb_0k rb_0 + Jb_1k rb_1) + w_a (Ja_0k ra_0 + Ja_1k ra_1) to g_k (7 sums), w the Huber weights.  The schedule is
 * vslam_resect.h's steps 3 to 6, word for word, under vslam_resect_params: the damping, the Cholesky solve (7 x 7), lambda, the
 * acceptance (every participant with Y_z > 0 in BOTH directions and a strictly lower cost), the rounds (a participant of a gated
 * round has Y_z > 0 and e <= gate_px in BOTH directions under the previous round's result), min_links counted in correspondences,
 * the start (R a polar step closer to a rotation, s and t as they are), the left-alone rules (with s not finite or not > 0 added)
 * and the four statistics (the means of rho(e_b) + rho(e_a) per participant).  Sums are formed as vslam_resect.h forms them.
 * Refusals: VSLAM_ERR_INVALID for a null pointer (d_mask, params and d_stats may be), batch or stride not positive, parameters
 * vslam_resect_poses would refuse, d_A, d_B, d_scale, d_R, d_T, d_stats, d_xa or d_xb off 8 bytes, d_n or d_mask off 4;
 * VSLAM_ERR_CAPACITY for stride > VSLAM_MAX_KP.  One launch, stream-ordered, nothing allocated.
 *
 * ---- on the world: two explicit calls for a world ATTACHED to `map` (vslam_map_attach_world); neither runs behind a step.
 * vslam_world_sim3 relates `items` pairs of recorded frames (track_a, frame_a, track_b, frame_b), device arrays [items]; the
 * tracks of a pair may be equal (a loop inside one track).  Per item: d_matches [kp_stride][2] and d_n_matches (clamped to 0 ..
 * kp_stride) in the layout vslam_match_features writes -- `first` a keypoint of frame a, `second` a keypoint of frame b --, and
 * the two frames' keypoints d_xy_a, d_xy_b [kp_stride][2].  An item whose tracks are not in 0 .. tracks - 1 or whose frames are
 * not in 0 .. frames recorded - 1 has no correspondence.
 *   GATHER.  Match k < n is TAKEN iff 0 <= first, second < kp_stride; both keypoints have a map point (d_map_point_ids of their
 *   track and frame >= 0 and < map_capacity; -1 = none); once a fusion exists (vslam_fuse.h) each id is replaced by its d_fuse_to,
 *   and -1 (culled) is not taken; the x, y, z of both d_world_points rows are finite; and both keypoints' x, y are finite.  With
 *   Twc = d_Twc of the track and frame, rotation block W (W_rc = Twc[4 r + c]) and centre C (C_r = Twc[4 r + 3]), p the point's
 *   row widened and D = p - C:  A_i = (W_0i D_0 + W_1i D_1) + W_2i D_2 on side a, B likewise on side b.  THE TRANSPOSE STANDS FOR THE
 *   INVERSE: the block is a product of f32-rounded rotations and is not re-orthonormalised (vslam_amd.h).  The taken matches are
 *   compacted in match order; d_n_corr their count; d_point_a / d_point_b [kp_stride] (either may be NULL) the two ids of each
 *   (after d_fuse_to), slots past the count keep their bits.
 *   Steps 1 to 6 above run on the compacted rows (stride kp_stride), the polish when polish != NULL.
 *   Outputs.  d_scale, d_R, d_T: the camera-to-camera model as vslam_sim3_ransac writes it (only where found).  d_found (1 / 0),
 *   d_n_inliers, d_winner as vslam_sim3_ransac's.  For a found item the world-to-world similarity X_a = s_w R_w X_b + t_w, from
 *   the (polished) model, into d_s_w [1], d_R_w [9], d_t_w [3] (other items keep their bits):
 *        s_w = 1 / s;   M_ij = (Wa_i0 R_j0 + Wa_i1 R_j1) + Wa_i2 R_j2;   R_w,ij = (M_i0 Wb_j0 + M_i1 Wb_j1) + M_i2 Wb_j2;
 *        u_i = (R_0i t_0 + R_1i t_1) + R_2i t_2;   v_r = (Wa_r0 u_0 + Wa_r1 u_1) + Wa_r2 u_2;   w_r = (R_w,r0 Cb_0 + R_w,r1 Cb_1) +
 *        R_w,r2 Cb_2;   t_w,r = (Ca_r - v_r / s) - s_w w_r.
 *   THE IDS ARE THE MAP'S, AS THE REFERENCE SETS THEM: vslam_map_step gives a keypoint an id by propagation and by association only, and the
 *   points a pair appends get none (vslam_amd.h, step 5), so on a map advanced by vslam_map_step alone few keypoints carry one and a pair
 *   of frames may gather too few correspondences to be found.  A caller that has better correspondences forms them itself and calls
 *   vslam_sim3_ransac.  A gather through the world's observation log is left open.
 *   It writes nothing into the world or the map.  Refusals: VSLAM_ERR_INVALID for a null pointer (params, polish, d_point_a,
 *   d_point_b and d_stats may be), items not positive, a world that is not the one attached to that map or has not as many frames,
 *   parameters vslam_sim3_ransac would refuse, d_matches, d_xy_a, d_xy_b or an f64 array off 8 bytes, another array off 4.  The
 *   workspace (the compacted rows and the mask: items x kp_stride x 68 bytes) comes from the arena.  Launches: the gather, the
 *   three (and the polish's one) of vslam_sim3_ransac, and one for d_found and the world-to-world similarity.
 *
 * vslam_world_apply_sim3 carries whole tracks through X' = s R X + t (map merging: with the world-to-world similarity of a found
 * item, track b's world becomes track a's).  h_track [items] is a HOST array -- a track listed twice or outside 0 .. tracks - 1 is
 * VSLAM_ERR_INVALID, checked before anything is queued --; d_s [items], d_R [items][9], d_t [items][3] f64 and d_apply [items]
 * on the device.  An item with apply == 0, or whose s, R, t are not finite or s not > 0, leaves its track alone.  Otherwise, for
 * every recorded frame f of the track:  d_Twc gets the rotation block (R W)_ij = (R_i0 W_0j + R_i1 W_1j) + R_i2 W_2j and the centre
 * C'_i = s ((R_i0 C_0 + R_i1 C_1) + R_i2 C_2) + t_i, row 3 kept;  d_pose is the same sixteen values rounded once;  d_scale[f] = d_scale[f] s.
 * Valid d_carry rows (d_carry_index >= 0) are multiplied by s, component by component.  Every d_world_points row below the map's
 * d_sizes whose x, y, z are finite becomes s ((R_i0 x + R_i1 y) + R_i2 z) + t_i in f64, rounded once; NaN rows and w stay.  d_links,
 * d_fuse_to, the resection's statistics and every array of the map keep their bits; vslam_world_reset undoes it as it undoes
 * everything else.  h_track is read before the call returns and handed to the kernel by value, 64 tracks a launch: no copy is queued,
 * nothing is allocated, the launches are stream-ordered.  Refusals:
 * VSLAM_ERR_INVALID for a null pointer, items not positive or above the world's tracks, a world that is not the one attached to that
 * map, d_s, d_R or d_t off 8 bytes, d_apply off 4.
 *
 * Spreading a loop's error over the frames between its ends is vslam_graph.h's (vslam_world_close_loops takes a same-track item's
 * camera-to-camera model as it stands).  Left open: merging two tracks' point lists into one map (the two ends of a loop INSIDE a track: vslam_fuse_project.h); deciding when to accept a loop; an f64 matrix-core count
 * (v_mfma_f64_16x16x4 has K = 4 = (x, y, z, 1), but its internal summation order is not this contract's); pushing the verified
 * matches into the map's log.                                                                                                    */
#ifndef VSLAM_SIM3_H
#define VSLAM_SIM3_H

#include "vslam_amd.h"
#include "vslam_resect.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vslam_sim3_params {
    int32_t hypotheses;    /* a multiple of 64 in 64 .. 1024        */
    int32_t min_inliers;   /* >= 4                                  */
    double  inlier_px;     /* > 0 and finite                        */
} vslam_sim3_params;
/* {128, 8, 2.0} */
int vslam_sim3_params_default(vslam_sim3_params *out);

int vslam_sim3_ransac(vslam_ctx *ctx,
        const double *d_A, const float *d_xa, const double *d_B, const float *d_xb,   /* [batch][stride][3] f64, [..][2] f32      */
        const int32_t *d_n, int batch, int stride,
        const float *h_K, const uint32_t *d_seeds /* [batch] */,
        const vslam_sim3_params *params /* NULL: defaults */, const vslam_resect_params *polish /* NULL: no polish */,
        double *d_scale, double *d_R, double *d_T,        /* [batch], [batch][9], [batch][3]: written where found              */
        int32_t *d_inlier,                                /* [batch][stride]                                                   */
        int32_t *d_corr_index,                            /* [batch][stride] or NULL                                           */
        int32_t *d_n_inliers, int32_t *d_winner,          /* [batch]                                                           */
        int32_t *d_counts /* [batch][hypotheses] or NULL */, double *d_stats /* [batch][4] or NULL */);

int vslam_sim3_refine(vslam_ctx *ctx,
        const double *d_A, const float *d_xa, const double *d_B, const float *d_xb, const int32_t *d_n, int batch, int stride,
        const int32_t *d_mask /* [batch][stride] or NULL */, const float *h_K, const vslam_resect_params *params /* NULL: defaults */,
        double *d_scale, double *d_R, double *d_T /* IN / OUT */, double *d_stats /* [batch][4] or NULL */);

int vslam_world_sim3(vslam_ctx *ctx, vslam_world *world, vslam_map *map,
        const int32_t *d_track_a, const int32_t *d_frame_a, const int32_t *d_track_b, const int32_t *d_frame_b, int items,
        const int32_t *d_matches, const int32_t *d_n_matches,             /* [items][kp_stride][2], [items]                      */
        const float *d_xy_a, const float *d_xy_b,                         /* [items][kp_stride][2]                               */
        const float *h_K, const uint32_t *d_seeds /* [items] */,
        const vslam_sim3_params *params /* NULL: defaults */, const vslam_resect_params *polish /* NULL: no polish */,
        double *d_scale, double *d_R, double *d_T,                        /* camera a -> camera b, where found                   */
        double *d_s_w, double *d_R_w, double *d_t_w,                      /* world b -> world a, where found                     */
        int32_t *d_found, int32_t *d_n_corr, int32_t *d_n_inliers, int32_t *d_winner,   /* [items]                            */
        int32_t *d_point_a, int32_t *d_point_b /* [items][kp_stride], may be NULL */, double *d_stats /* [items][4] or NULL */);

int vslam_world_apply_sim3(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const int32_t *h_track /* HOST [items] */,
                           const double *d_s, const double *d_R, const double *d_t, const int32_t *d_apply, int items);

#ifdef __cplusplus
}
#endif

#endif
