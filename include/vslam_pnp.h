/* A pose without a prior: hypothesise-and-count (RANSAC) over 3-D / 2-D correspondences with a minimal solver (P3P), for a batch of
 * independent items.  Every other way to a pose in this project needs a start that is already close (the chain from the pair's
 * fundamental matrix, vslam_resect_poses, vslam_search_projection's window); this one needs none.  An explicit call: nothing in
 * vslam_amd.h, vslam_resect.h, vslam_adjust.h or vslam_search.h launches a kernel of this file, and no existing output changes a
 * bit.  Below it: a match of world points to keypoints that needs no pose (vslam_match_points) and the two joined into one call
 * that relocalises a track of a world (vslam_world_relocalise).
 *
 * THIS TEXT and tests/ref_pnp.py are the contract.  ALL floating-point arithmetic is f64, never fused, in the written order, with
 * + - * / and sqrt only; f32 inputs are widened first.  Counts are integers and the choice is one maximum over integer keys, so
 * nothing depends on the order in which lanes arrive, and an item's bits depend on the item alone: the same in every run, batch
 * size and batch slot.
 *
 * An item: n correspondences (P_i, x_i) in the layout vslam_resect_poses reads -- d_points [stride][3] f64, d_xy [stride][2] f32,
 * n = d_n clamped to 0 .. stride --, the camera matrix K (h_K [9] f32, row-major, on the host), a seed.
 *   1. SETS.  mix(x) on u32: x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16.  Draw c of hypothesis h
 *      is r = mix(mix(seed ^ (0x9e3779b9 * (h + 1))) + c), its index ((u64) r * n) >> 32.  Draws c = 0, 1, ... are taken in order,
 *      one that repeats an index already chosen is skipped, and after 16 draws a hypothesis without three distinct indices has
 *      no pose.  A hypothesis depends on (seed, h, n) alone.
 *   2. POSES.  P3P on the three points and their unit bearings K^-1 (x, y, 1) / |.|: up to 4 poses (R, T), world -> camera, Y = R P
 *      + T as vslam_resect_poses takes it, in solution slots s = 0 .. 3.  The formulation (vslam_amd/csrc/pnp_math.h, which states
 *      every expression): with the distances s_1 = u s_0 and s_2 = v s_0 along the bearings, the two law-of-cosines ratios are
 *      quadratics in u whose resultant is a quartic in v; its roots by Ferrari's method, the resolvent cubic's root by a
 *      bracketed Newton iteration of at most 64 steps, each root then taken 6 Newton steps on the quartic itself; slots 0, 1 are
 *      the roots of the first quadratic factor, 2, 3 of the second.  The pose of a root: R from the orthonormal frames of the
 *      three camera points s_i f_i and of the three points, T = s_0 f_0 - R P_0.  A solution is dropped when u, v or a distance is
 *      not finite or not > 0, when R or T is not finite, or when max |R^t R - I| > 1e-9.  Collinear or repeated points give no
 *      pose.  No cbrt, acos, cos or pow, and no loop whose trip count depends on the data beyond the caps above.
 *   3. COUNT.  Correspondence i < n is an inlier of a pose iff Y = R P + T has Y_z > 0; (u, v) = (q0 / q2, q1 / q2), q = K Y, is
 *      finite; and r0 r0 + r1 r1 <= inlier_px inlier_px with r = (u, v) - x (a closed disc; the right side is one product).  Y, q
 *      and (u, v) are formed exactly as vslam_resect.h writes them.
 *   4. CHOICE.  The winner is the pose with the largest count; ties go to the smallest 4 h + s.  The item is FOUND iff that count
 *      >= min_inliers.  The item is LEFT ALONE -- not found, its d_R / d_T bits kept -- when n < 4, when a K is not finite, or
 *      when a P_i or x_i with i < n is not finite; such an item has no pose in any hypothesis.
 *   5. OUTPUTS.  d_R [9], d_T [3] f64: written only for a found item.  d_inlier [stride] int32: 1 / 0 for the winner below n, 0
 *      from n on and everywhere for an item that is not found.  The winner's inliers compacted in ascending index into
 *      d_corr_points [stride][3] f64, d_corr_xy [stride][2] f32, d_corr_index [stride] (may be NULL), d_n_inliers their count (0
 *      when not found): the layout vslam_resect_poses reads; slots from the count on keep their bits.  d_winner: 4 h + s, or -1.
 *      d_counts [hypotheses][4] int32 or NULL: every pose's count, -1 where there is no solution.  d_stats [4] f64 or NULL: the
 *      statistics of the polish as vslam_resect_poses writes them; NaN NaN NaN NaN without one.
 *   6. POLISH.  With polish != NULL, vslam_resect_poses' kernel runs from the winner's (R, T) over the compacted inliers, in
 *      place on d_R / d_T: its result replaces (R, T) where the resection moved the item (an item that is not found has no
 *      correspondences and is left alone by it too).  The mask, the compacted rows and d_n_inliers are NOT recomputed.
 *
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (params, polish, d_corr_index, d_counts and d_stats may
 * be); batch or stride not positive; hypotheses not a multiple of 64 in 64 .. 1024; min_inliers < 4; inlier_px not finite or not
 * > 0; polish parameters vslam_resect_poses would refuse; a pointer off its alignment: the f64 arrays (d_points, d_R, d_T,
 * d_corr_points, d_stats), d_xy and d_corr_xy 8 bytes, every other array 4.  VSLAM_ERR_CAPACITY: stride > VSLAM_MAX_KP.
 *
 * Three launches (solve, count, select) and the polish's one, stream-ordered on the context, no synchronisation.  The workspace
 * (every pose and its count: batch x hypotheses x 4 x 104 bytes) comes from the context's grow-only arena: allocated on the
 * first call of a size, never afterwards.  inlier_px and min_inliers are untuned on real footage.                            */
#ifndef VSLAM_PNP_H
#define VSLAM_PNP_H

#include "vslam_amd.h"
#include "vslam_resect.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vslam_pnp_params {
    int32_t hypotheses;    /* a multiple of 64 in 64 .. 1024                                                  */
    int32_t min_inliers;   /* >= 4                                                                            */
    double  inlier_px;     /* > 0 and finite; 2 is the square root of the reference's thresholdSq = 4         */
} vslam_pnp_params;
/* {128, 8, 2.0} */
int vslam_pnp_params_default(vslam_pnp_params *out);

int vslam_pnp_ransac(vslam_ctx *ctx,
        const double *d_points, const float *d_xy, const int32_t *d_n, int batch, int stride,   /* as vslam_resect_poses      */
        const float *h_K, const uint32_t *d_seeds /* [batch] */,
        const vslam_pnp_params *params /* NULL: defaults */, const vslam_resect_params *polish /* NULL: no polish */,
        double *d_R, double *d_T,                                         /* [batch][9], [batch][3]: written where found      */
        int32_t *d_inlier,                                                /* [batch][stride]                                  */
        double *d_corr_points, float *d_corr_xy, int32_t *d_corr_index,   /* [batch][stride][3], [..][2], [..] (may be NULL)  */
        int32_t *d_n_inliers, int32_t *d_winner,                          /* [batch]                                          */
        int32_t *d_counts /* [batch][hypotheses][4] or NULL */, double *d_stats /* [batch][4] or NULL */);

/* ---- world points to keypoints without a pose: vslam_search_projection (include/vslam_search.h) with its step 1 (visibility) and
 * the disc of its step 2 taken out.  Integers only.
 *   A point i < n (n = d_n_points clamped to 0 .. pt_stride) TAKES PART iff its CSR range is valid (0 <= offsets[i] < offsets[i +
 *   1] <= obs_stride) and its x, y, z are finite.  Every keypoint k < n_kp (n_kp = d_n_kp clamped to 0 .. kp_stride) that is not
 *   taken (d_kp_taken NULL, or taken[k] < 0) is a candidate of every such point; d_xy is only copied, never tested.  d(i, k), the
 *   choice (d0, k0), d1, the proposal rule (d0 < dist_threshold and the ratio10 test), the one-to-one resolution by the smallest
 *   (d0, i) and the outputs are the text of vslam_search.h, steps 2 to 5, unchanged; d_stats [4] int32: the points taking part,
 *   those with at least one candidate, those proposing, those found.
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (d_kp_taken, params, d_corr_point, d_corr_kp and d_stats
 * may be); batch, pt_stride, obs_stride or kp_stride not positive; dist_threshold outside 1 .. 257; ratio10 outside 0 .. 10; a
 * pointer off its alignment: d_points, d_desc and d_obs_desc 16 bytes; d_xy, d_corr_xy and d_corr_points 8; every other array 4.
 * VSLAM_ERR_CAPACITY: kp_stride > VSLAM_MAX_KP.
 * Two launches behind one fill of the keys, stream-ordered, no synchronisation; the workspace (batch x (kp_stride + pt_stride) x 8
 * bytes) comes from the arena.  The cost is every point against every keypoint: dist_threshold and ratio10 are untuned.        */
typedef struct vslam_match_params {
    int32_t dist_threshold;   /* 1 .. 257 (64 is the reference's DISTANCE_THRESHOLD)             */
    int32_t ratio10;          /* 0 = no ratio test, else 1 .. 10                                 */
} vslam_match_params;
/* {64, 8} */
int vslam_match_params_default(vslam_match_params *out);

int vslam_match_points(vslam_ctx *ctx,
        const float *d_points, const int32_t *d_n_points, int pt_stride,          /* [batch][pt_stride][4] f32, w not read   */
        const int32_t *d_obs_offsets, const uint8_t *d_obs_desc, int obs_stride,  /* CSR as vslam_search_projection takes    */
        const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp, int kp_stride,
        const int32_t *d_kp_taken /* may be NULL */, int batch, const vslam_match_params *params /* NULL: defaults */,
        int32_t *d_kp_of_point, int32_t *d_dist,          /* [batch][pt_stride]                                               */
        double *d_corr_points, float *d_corr_xy,          /* [batch][kp_stride][3] f64, [batch][kp_stride][2] f32              */
        int32_t *d_corr_point, int32_t *d_corr_kp,        /* [batch][kp_stride]; either may be NULL                            */
        int32_t *d_n_corr, int32_t *d_stats /* [batch][4] or NULL */);

/* ---- on the world: one explicit call for a world ATTACHED to `map` (vslam_map_attach_world) that finds the pose of the caller's
 * latest frame from the map alone.  The last recorded pose is NOT READ on the way to the result.  Per track, with f1 = frames
 * recorded - 1:
 *   1. the map's CSR with descriptors, as vslam_world_search obtains it (vslam_map_observation_descriptors, in the arena);
 *   2. vslam_match_points over d_world_points rows < d_sizes[track] (pt_stride = map_capacity) against d_xy_cur / d_desc_cur /
 *      d_n_cur [tracks][kp_stride], nothing taken;
 *   3. vslam_pnp_ransac on what was matched (stride kp_stride), with the polish when polish != NULL;
 *   4. for the tracks that were FOUND, the write-back of vslam_world_search, word for word, with (R', T') the result of 3:
 *      d_Twc[f1], d_pose[f1] and the latest carry re-expressed (w from the frame's d_Twc BEFORE the call, then p' = R' w + T').
 * d_scale, d_links, the steps' resection statistics, d_world_points and every array of the map keep their bits; a track that is not
 * found keeps every bit.
 * Outputs: d_found [tracks] (1 / 0), d_winner, d_n_inliers [tracks] as vslam_pnp_ransac writes them; d_corr_point / d_corr_kp
 * [tracks][kp_stride] and d_n_corr [tracks] as vslam_match_points writes them; d_stats [tracks][4] f64 or NULL: the polish's.
 * VSLAM_ERR_INVALID: a null pointer (match, pnp, polish and d_stats may be), a world that is not the one attached to that map,
 * d_xy_cur off 8 bytes, d_desc_cur off 16, d_stats off 8, another array off 4, parameters either call would refuse.            */
int vslam_world_relocalise(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                           const int32_t *d_n_cur, const float *h_K, const uint32_t *d_seeds /* [tracks] */,
                           const vslam_match_params *match, const vslam_pnp_params *pnp, const vslam_resect_params *polish,
                           int32_t *d_found, int32_t *d_winner, int32_t *d_n_inliers,
                           int32_t *d_corr_point, int32_t *d_corr_kp, int32_t *d_n_corr, double *d_stats);

#ifdef __cplusplus
}
#endif

#endif
