/* Search by projection: the points of a track projected into a frame with a pose of the caller's choice, and for each of them the
 * best keypoint of that frame by descriptor distance inside a pixel window; ambiguous matches rejected, the result made
 * one-to-one, and written in the layout vslam_resect_poses reads.  A batch entry of its own and one explicit call on a world
 * attached to a map (vslam_world_search, below).  Explicit calls: nothing in vslam_amd.h, vslam_resect.h or vslam_adjust.h
 * launches a kernel of this file, and no existing output changes a bit.  (vslam_associate_map_points stays what it is: the
 * reference's loop, in the pair's coordinates, radius 2, first acceptable hit.)
 *
 * THIS TEXT and tests/ref_search.py are the contract.  ALL floating-point arithmetic is f64, never fused, in the written order;
 * f32 inputs are widened first.  Everything behind the disc test is integers.  Every choice is a minimum over integer keys, so
 * nothing depends on the order in which lanes or atomics arrive, and an item's bits depend on the item alone: the same in every
 * run, batch size and batch slot.
 *
 * An item.  n points P_i (d_points rows [x y z w] f32, w is not read), n = d_n_points clamped to 0 .. pt_stride; the points'
 * observation descriptors in CSR by point, as vslam_associate_map_points takes them: d_obs_offsets [pt_stride + 1] per item, the
 * observations of point i are rows offsets[i] .. offsets[i + 1] - 1 of d_obs_desc [obs_stride][32]; a pose (R [9] row-major, T
 * [3]) taking the points' coordinates to the camera, as vslam_resect_poses takes it; n_kp keypoints (d_xy, d_desc), n_kp = d_n_kp
 * clamped to 0 .. kp_stride; optionally d_kp_taken: a keypoint k with taken[k] >= 0 is no candidate.
 *   1. VISIBLE.  Point i < n is visible iff 0 <= offsets[i] < offsets[i + 1] <= obs_stride; x, y, z are finite; Y = R P + T (RP_r
 *      = (R_r0 x + R_r1 y) + R_r2 z, Y_r = RP_r + T_r) is finite with Y_z > 0; (u, v) = (q0 / q2, q1 / q2), q = K Y row by row
 *      (q_r = (K_r0 Y_0 + K_r1 Y_1) + K_r2 Y_2) -- both exactly as vslam_resect_poses forms them -- are finite; and 0 <= u <
 *      width, 0 <= v < height.  An item whose R or T is not finite has no visible point.
 *   2. CANDIDATES of a visible point: the keypoints k < n_kp that are not taken, whose x_k, y_k are finite, and with dx =
 *      (double)x_k - u, dy = (double)y_k - v: dx dx + dy dy <= radius radius (a closed disc; radius radius is one product).
 *      d(i, k) = the minimum over the point's observations of the 256-bit Hamming distance to keypoint k's descriptor.
 *   3. CHOICE.  (d0, k0) = the smallest (d, k) in lexicographic order.  d1 = the smallest d among the OTHER candidates (equal to
 *      d0 when another keypoint ties; none when the point has one candidate).  The point PROPOSES k0 iff d0 < dist_threshold and
 *      (ratio10 == 0, or there is no d1, or 10 d0 < ratio10 d1).
 *   4. ONE-TO-ONE.  A keypoint proposed to by several points goes to the smallest (d0, i).  The others get nothing in this call:
 *      there is no second choice.
 *   5. OUTPUTS.  d_kp_of_point / d_dist, for EVERY i < pt_stride: the keypoint found and its distance, or -1 and -1.  The found
 *      pairs compacted in ascending point index into d_corr_points (x, y, z widened to f64), d_corr_xy (the keypoint's f32 xy),
 *      d_corr_point, d_corr_kp (the two indices; either may be NULL); d_n_corr their count; slots from d_n_corr on keep their
 *      bits.  d_stats [4] int32 per item, or NULL: the points visible, those with at least one candidate, those proposing,
 *      those found.
 *
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (d_kp_taken, params, d_corr_point, d_corr_kp and
 * d_stats may be); batch, pt_stride, obs_stride, kp_stride, width or height not positive; radius_px not finite, not > 0 or > 64;
 * dist_threshold outside 1 .. 257; ratio10 outside 0 .. 10; a non-finite h_K; a pointer off its alignment: d_points, d_desc and
 * d_obs_desc 16 bytes; d_xy, d_corr_xy and the f64 arrays (d_R, d_T, d_corr_points) 8; every other array 4.
 * VSLAM_ERR_CAPACITY: kp_stride > VSLAM_MAX_KP, or width or height above 16384.
 *
 * Two launches (the proposals, the resolution) behind one fill of the keys, stream-ordered on the context, no synchronisation.
 * The workspace (one 64-bit key per keypoint slot, one proposal per point slot: batch x (kp_stride + pt_stride) x 8 bytes) comes
 * from the context's grow-only arena: allocated on the first call of a size, never afterwards.                               */
#ifndef VSLAM_SEARCH_H
#define VSLAM_SEARCH_H

#include "vslam_amd.h"
#include "vslam_resect.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vslam_search_params {
    double  radius_px;        /* > 0, finite, <= 64                                              */
    int32_t dist_threshold;   /* 1 .. 257 (64 is the reference's DISTANCE_THRESHOLD)             */
    int32_t ratio10;          /* 0 = no ratio test, else 1 .. 10                                 */
} vslam_search_params;
/* {8.0, 64, 8} */
int vslam_search_params_default(vslam_search_params *out);

int vslam_search_projection(vslam_ctx *ctx,
        const float *d_points, const int32_t *d_n_points, int pt_stride,          /* [batch][pt_stride][4] f32, w not read   */
        const int32_t *d_obs_offsets, const uint8_t *d_obs_desc, int obs_stride,  /* CSR as vslam_associate_map_points takes */
        const double *d_R, const double *d_T,                                     /* [batch][9], [batch][3]: points' frame -> camera */
        const float *h_K, int width, int height,
        const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp, int kp_stride,
        const int32_t *d_kp_taken /* may be NULL: [batch][kp_stride], a keypoint with a value >= 0 is no candidate */,
        int batch, const vslam_search_params *params /* NULL: defaults */,
        int32_t *d_kp_of_point, int32_t *d_dist,          /* [batch][pt_stride]: keypoint or -1, its distance or -1           */
        double *d_corr_points, float *d_corr_xy,          /* [batch][kp_stride][3] f64, [batch][kp_stride][2] f32              */
        int32_t *d_corr_point, int32_t *d_corr_kp,        /* [batch][kp_stride]; either may be NULL                            */
        int32_t *d_n_corr, int32_t *d_stats /* [batch][4] or NULL */);

/* The map's observation descriptors in the CSR order of vslam_map_observations: d_offsets [tracks][map_capacity + 1] as that call
 * writes them, d_desc [tracks][obs_capacity][32] (16-byte aligned): row o is the descriptor of the observation that
 * vslam_map_observations puts at row o; rows past a track's total keep their bits.  The two launches of vslam_map_observations
 * with the descriptor destination set.  VSLAM_ERR_INVALID: a null pointer, a map of another context, d_offsets off 4 bytes or
 * d_desc off 16.                                                                                                            */
int vslam_map_observation_descriptors(vslam_ctx *ctx, vslam_map *map, int32_t *d_offsets, uint8_t *d_desc);

/* ---- on the world: one explicit call for a world ATTACHED to `map` (vslam_map_attach_world) that searches every track's world
 * points in the caller's latest frame and, with resect != NULL, resects that frame's pose against what it found.  It does not
 * run behind a step.  VSLAM_ERR_INVALID: a null pointer (search, resect and d_stats may be), a world that is not the one
 * attached to that map, d_xy_cur off 8 bytes, d_desc_cur off 16, d_stats off 8, another array off 4, a non-finite h_K, width or
 * height not positive, parameters out of range; VSLAM_ERR_CAPACITY: width or height above 16384.
 * Per track, with f1 = frames recorded - 1:
 *   the pose   from M = d_Twc[track][f1] (camera -> world), as vslam_adjust.h forms "camera c": R_rc = M[4 c + r], T_r = -((M[r]
 *              M[3] + M[4 + r] M[7]) + M[8 + r] M[11]).
 *   the points d_world_points rows < d_sizes[track] (pt_stride = map_capacity); their descriptors the CSR of
 *              vslam_map_observation_descriptors, in the arena; the keypoints d_xy_cur / d_desc_cur / d_n_cur [tracks][kp_stride],
 *              nothing taken.
 * Launches: the map's CSR with descriptors (two), the pose (one), vslam_search_projection's; with resect the kernel of
 * vslam_resect_poses on (d_corr_points, d_corr_xy, d_n_corr) from (R, T), and the write-back (one).  Workspace from the arena.
 * Write-back, ONLY where the resection moved the item, exactly as vslam_adjust.h's "Write-back" states it for the last camera:
 *   d_Twc[f1]: M'[4 r + c] = R'_cr (c < 3), M'[4 r + 3] = -((R'_0r T'_0 + R'_1r T'_1) + R'_2r T'_2), row 3 = (0, 0, 0, 1);
 *   d_pose[f1] = M' rounded once to f32; the latest carry (every entry with d_carry_index >= 0): w_r = ((M[4 r] p_0 + M[4 r + 1]
 *   p_1) + M[4 r + 2] p_2) + M[4 r + 3] with M the frame's d_Twc BEFORE the call, then p'_r = ((R'_r0 w_0 + R'_r1 w_1) + R'_r2
 *   w_2) + T'_r.
 * d_scale, d_links, the steps' resection statistics, d_world_points and every array of the map keep their bits; a call with
 * resect == NULL writes nothing but its outputs.
 * Outputs: d_corr_point / d_corr_kp [tracks][kp_stride] and d_n_corr [tracks] as vslam_search_projection writes them; d_stats
 * [tracks][4] f64 or NULL: the statistics of vslam_resect_poses per track (not written when resect == NULL).                */
int vslam_world_search(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                       const int32_t *d_n_cur, const float *h_K, int width, int height, const vslam_search_params *search,
                       const vslam_resect_params *resect /* NULL: search only */,
                       int32_t *d_corr_point, int32_t *d_corr_kp, int32_t *d_n_corr,   /* [tracks][kp_stride], [tracks] */
                       double *d_stats /* [tracks][4] resection statistics, or NULL */);

#ifdef __cplusplus
}
#endif

#endif
