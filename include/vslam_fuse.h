/* Map points that share an observation fused into tracks, and the points their observations do not support culled: two batch
 * entry points and their calls on a world.  Explicit calls: nothing in vslam_amd.h, vslam_resect.h, vslam_adjust.h, vslam_search.h
 * or vslam_pnp.h launches a kernel of this file while they are unused, and no existing output changes a bit.
 *
 * Why.  The map copies the reference bit for bit, and the reference's add_reprojection_inliers never sets map_point_ids for the
 * point it appends (vslam_amd.h, step 5 of vslam_map_step): the next pair triangulates the same feature again, as a new point
 * whose first observation is the (frame, keypoint) the old point's second one was.  Almost every map point therefore has two
 * observations, and most physical features are in the map several times.  The calls here work on COPIES of the map's lists (the
 * CSR vslam_map_observations writes) and never on the map.
 *
 * THIS TEXT and tests/ref_fuse.py are the contract.  vslam_fuse_points is integers only: its results are minima and counts, so
 * nothing depends on the order in which lanes or atomics arrive.  vslam_cull_points is f64, never fused, in the written order, f32
 * inputs widened first; its sums are integer counts.  An item's bits depend on the item alone: the same in every run, batch size
 * and batch slot.
 *
 * ---- vslam_fuse_points: groups by shared observation, merged lists
 * An item.  n points, n = d_n_points clamped to 0 .. pt_stride; their observations in CSR by point, the shape
 * vslam_map_observations writes: d_obs_offsets [pt_stride + 1], the observations of point i are rows offsets[i] .. offsets[i + 1] -
 * 1 of d_obs_cam / d_obs_kp [obs_stride] (a frame and a keypoint of it); optionally d_mask [pt_stride].
 *   Point i TAKES PART iff i < n and (d_mask is NULL or mask[i] >= 0).
 *   An observation is VALID iff 0 <= cam < cam_stride and 0 <= kp < kp_stride.
 *   Two points that take part are LINKED iff they hold valid observations with equal (cam, kp).  A GROUP is a connected component
 *   of links; its SURVIVOR is its smallest index.
 *   MERGED ORDER of a group: its members in ascending index, each member's entries in input order.  An entry is KEPT iff it is
 *   valid and no earlier entry of the group's merged order has the same (cam, kp).
 * Outputs.  d_fuse_to [pt_stride]: the survivor's index for a point that takes part (a point standing for itself gets i), -1 for i
 * < n that takes no part, i for i >= n.  The merged CSR d_out_offsets [pt_stride + 1], d_out_cam, d_out_kp and d_out_src
 * [obs_stride] (d_out_src: the input row of each output entry; may be NULL): the survivor's row is its group's kept entries in
 * merged order, every other row is empty, offsets from n on repeat the total, slots past the total keep their bits.  d_stats [4]
 * int32 per item, or NULL: the points taking part, the groups with more than one member, the points absorbed (taking part, not
 * their own survivor), the entries kept.
 * Broken CSR.  An item with offsets[0] < 0, an offset below its predecessor, or an offset above obs_stride (all within offsets[0 ..
 * n]) is left alone: fuse_to[i] = i for every i < pt_stride, every out offset is 0, the stats are 0.
 * d_mask may be d_fuse_to itself (a point's mask is read before its fuse_to is written); no other output may overlap an input or
 * another output.
 *
 * One launch (one workgroup per item) behind one fill of the workspace.  Labels start as the points' own indices; a round posts
 * every point's label into the cell (cam, kp) of each of its valid observations by an integer atomic minimum, lets every point take
 * the minimum over its cells, and jumps once through the label's own label; labels only decrease, and a round that changes none
 * ends the loop, which is also capped at n + 1 rounds in code.  The kept entries are a second minimum per cell, over input rows
 * (input order is merged order: the CSR's rows ascend with the point).  Workspace from the context's grow-only arena, allocated
 * on the first call of a size and never afterwards: batch x (cam_stride x kp_stride + 3 pt_stride) x 4 bytes.
 *
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (d_mask, d_out_src and d_stats may be); batch,
 * pt_stride, obs_stride, cam_stride or kp_stride not positive; an array off 4 bytes.  VSLAM_ERR_CAPACITY: kp_stride >
 * VSLAM_MAX_KP or cam_stride > 1024.
 *
 * ---- vslam_cull_points: which points their observations support
 * An item.  n points P_i (d_points rows [x y z w] f32, w is not read), n as above; the CSR as above; C cameras taking the points'
 * coordinates to the camera, d_R [cam_stride][9] row-major and d_T [cam_stride][3] f64 as vslam_resect_poses takes a pose, C =
 * d_n_cams clamped to 0 .. cam_stride; the cameras' keypoints d_xy [cam_stride][kp_stride][2] f32; h_K (row-major f32).
 *   Point i TAKES PART iff i < n, its x, y, z are finite, and 0 <= offsets[i] < offsets[i + 1] <= obs_stride.
 *   An observation is USABLE iff 0 <= cam < C, 0 <= kp < kp_stride, that camera's R and T are finite, and the keypoint's x, y are
 *   finite.
 *   An observation is GOOD iff it is usable, Y = R P + T has Y_z > 0, (u, v) = (q0 / q2, q1 / q2) with q = K Y is finite -- Y, q
 *   and (u, v) exactly as vslam_resect.h writes them --, and with r0 = u - (double)x, r1 = v - (double)y: r0 r0 + r1 r1 <=
 *   inlier_px inlier_px (a closed disc; the right side is one product).
 *   Per point: n_usable, n_good, and last = the largest usable cam (-1 when there is none).  need = mature_good when last +
 *   mature_age < C, else min_good.  The point is KEPT iff n_good >= need and 10 n_good >= good10 n_usable.
 * Outputs, for EVERY i < pt_stride.  d_keep: 1 kept, 0 culled, -1 for a point that took no part (i >= n included).  d_counts
 * [pt_stride][2] or NULL: n_usable and n_good (0 and 0 for a point that took no part).  d_stats [4] int32 per item: the points
 * taking part, kept, culled, and the good observations of the points taking part.
 * The call is pure: it writes nothing but its outputs.  One launch behind one fill of d_stats; no workspace.
 * vslam_cull_params {inlier_px, min_good, mature_good, mature_age, good10}, defaults {6.0, 2, 3, 3, 5}: 6 is
 * vslam_adjust_params.gate_px; a point whose last usable frame lies mature_age or more frames back must have gathered
 * mature_good good observations, a younger one min_good; and half of what a point has must be good.  THESE VALUES ARE UNTUNED:
 * they have been run on synthetic scenes only.
 *
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (params and d_counts may be); batch, pt_stride,
 * obs_stride, cam_stride or kp_stride not positive; inlier_px not finite or not > 0; min_good or mature_good < 1; mature_age < 0
 * or > 1048576; good10 outside 0 .. 10; a non-finite h_K; d_points off 16 bytes, d_xy, d_R or d_T off 8, another array off 4.
 * VSLAM_ERR_CAPACITY: kp_stride > VSLAM_MAX_KP or cam_stride > 1024.
 *
 * ---- on the world: explicit calls for a world ATTACHED to `map` (vslam_map_attach_world); none of them runs behind a step.  The map's
 * own arrays and its log never change -- they are the reference's --; everything here is state of the world beside the map.
 * The world gains d_fuse_to [tracks][map_capacity] int32: allocated by the first vslam_world_fuse or vslam_world_cull, freed with the
 * world, the identity at first; fuse_to[i] is the survivor point i stands behind, -1 means culled.  It is reached through
 * vslam_world_fusion_view (vslam_world_arrays keeps its layout): *d_fuse_to is NULL and *state 0 while there is "no fusion"; state
 * bit 0: vslam_world_fuse has run, bit 1: vslam_world_cull has run.  vslam_world_reset and vslam_map_reset put it back to "no
 * fusion".
 *   vslam_world_fuse runs vslam_fuse_points over the map's log (vslam_map_observations into the arena; pt_stride = map_capacity,
 *   obs_stride = obs_capacity, cam = the frame, cam_stride = max_frames), from scratch on every call, with d_mask = d_fuse_to: culled
 *   points stay culled, an absorbed point whose log grew later still counts.  It writes d_fuse_to, sets the d_world_points row of
 *   every NEWLY absorbed point (absorbed now, its own survivor before) to three quiet NaNs (0x7FC00000) and w = 0, and leaves every
 *   other row alone: the survivor keeps its own position.  d_stats [tracks][4] int32 or NULL as vslam_fuse_points writes them.
 *   THE WORLD'S CSR, once a fusion exists (state bit 0), is that same computation on the map's log as it is NOW, d_mask = d_fuse_to:
 *   it is formed afresh wherever it is read, so steps taken since the last vslam_world_fuse are in it (a point they link into a group
 *   has an empty row from then on; its d_world_points row turns NaN at the next vslam_world_fuse).  Without a fusion it is the
 *   map's own CSR.  vslam_world_observations returns it: d_offsets [tracks][map_capacity + 1], d_frame_ids / d_point_ids
 *   [tracks][obs_capacity], d_desc [tracks][obs_capacity][32] or NULL (the descriptors, gathered through d_out_src); slots past a
 *   track's total keep their bits.  vslam_world_search, vslam_world_relocalise and vslam_world_adjust read it in place of the map's own
 *   (one helper, vs_world_csr); without a fusion they make exactly the launches they made before this header existed.
 *   Nothing else changes: a point with a NaN row is already invisible to each consumer by its own stated rule -- the search's step 1,
 *   "TAKES PART" of vslam_match_points, "USABLE" of the adjustment, "drawn iff finite" of the renderer -- and a point with an empty
 *   row to the first three.  PointMap.view()["world_points"] (the Python binding) then shows NaN rows.
 *   vslam_world_cull runs vslam_cull_points with camera f = recorded frame f, formed from d_Twc as vslam_adjust.h forms "camera c"
 *   (C = the frames recorded, cam_stride = max_frames), the points d_world_points, the CSR the world's, d_xy the keypoints of every
 *   frame in the layout vslam_world_adjust takes ([tracks][xy_frames][kp_stride][2], xy_frames >= the frames recorded).  A point
 *   with keep == 0 gets d_fuse_to = -1 and a NaN row; every point whose survivor (by d_fuse_to) was culled gets -1 too.  d_stats
 *   [tracks][4] int32 or NULL as vslam_cull_points writes them.
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (params, d_stats and d_desc may be), a world that is not
 * the one attached to that map or has not as many frames, xy_frames below the frames recorded, parameters out of range, a
 * non-finite h_K, d_xy off 8 bytes, d_desc off 16, another array off 4.  VSLAM_ERR_CAPACITY: max_frames > 1024.
 * Workspace from the arena: vslam_fuse_points' own plus tracks x (2 map_capacity + 1 + 5 obs_capacity) x 4 bytes, and tracks x
 * obs_capacity x 32 where descriptors are gathered.
 *
 * Geometric fusing through a search by projection (points that never shared a keypoint) is vslam_fuse_project.h's, whose extras
 * enter the world's CSR above as further entries of the map's log.  Left open: running behind every step;
 * tuning on footage.  The survivor keeps its own position here: vslam_world_retriangulate (vslam_tracks.h) gives every track the
 * position all its observations support, with a parallax test as one of its refusals.                                          */
#ifndef VSLAM_FUSE_H
#define VSLAM_FUSE_H

#include "vslam_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vslam_cull_params {
    double  inlier_px;      /* > 0, finite                                                       */
    int32_t min_good;       /* >= 1: good observations a young point needs                       */
    int32_t mature_good;    /* >= 1: and a mature one                                            */
    int32_t mature_age;     /* 0 .. 1048576: frames behind the newest camera that make a point mature */
    int32_t good10;         /* 0 .. 10: tenths of a point's usable observations that must be good */
} vslam_cull_params;
/* {6.0, 2, 3, 3, 5} */
int vslam_cull_params_default(vslam_cull_params *out);

int vslam_fuse_points(vslam_ctx *ctx,
        const int32_t *d_n_points, int pt_stride,                                 /* [batch]                                  */
        const int32_t *d_obs_offsets, const int32_t *d_obs_cam, const int32_t *d_obs_kp, int obs_stride,
                                                                                  /* [batch][pt_stride + 1], [batch][obs_stride] twice */
        int cam_stride, int kp_stride,
        const int32_t *d_mask /* may be NULL: [batch][pt_stride], a point with a value < 0 takes no part */,
        int batch,
        int32_t *d_fuse_to,                                                       /* [batch][pt_stride]                       */
        int32_t *d_out_offsets, int32_t *d_out_cam, int32_t *d_out_kp,            /* [batch][pt_stride + 1], [batch][obs_stride] twice */
        int32_t *d_out_src /* [batch][obs_stride] or NULL */, int32_t *d_stats /* [batch][4] or NULL */);

int vslam_cull_points(vslam_ctx *ctx,
        const float *d_points, const int32_t *d_n_points, int pt_stride,          /* [batch][pt_stride][4] f32, w not read    */
        const int32_t *d_obs_offsets, const int32_t *d_obs_cam, const int32_t *d_obs_kp, int obs_stride,
        const double *d_R, const double *d_T, const int32_t *d_n_cams, int cam_stride,   /* [batch][cam_stride][9], [..][3], [batch] */
        const float *d_xy, int kp_stride,                                         /* [batch][cam_stride][kp_stride][2] f32    */
        const float *h_K, int batch, const vslam_cull_params *params /* NULL: defaults */,
        int32_t *d_keep,                                                          /* [batch][pt_stride]                       */
        int32_t *d_counts /* [batch][pt_stride][2] or NULL */, int32_t *d_stats /* [batch][4] */);

int vslam_world_fuse(vslam_ctx *ctx, vslam_world *world, vslam_map *map, int32_t *d_stats /* [tracks][4] or NULL */);

int vslam_world_cull(vslam_ctx *ctx, vslam_world *world, vslam_map *map,
                     const float *d_xy, int xy_frames,                  /* [tracks][xy_frames][kp_stride][2] f32 */
                     const float *h_K, const vslam_cull_params *params /* NULL: defaults */, int32_t *d_stats /* [tracks][4] or NULL */);

int vslam_world_observations(vslam_ctx *ctx, vslam_world *world, vslam_map *map,
                             int32_t *d_offsets, int32_t *d_frame_ids, int32_t *d_point_ids,   /* as vslam_map_observations takes them */
                             uint8_t *d_desc /* [tracks][obs_capacity][32] or NULL */);

/* *d_fuse_to: [tracks][map_capacity] int32, or NULL while there is no fusion; *state (may be NULL): bit 0 fused, bit 1 culled */
int vslam_world_fusion_view(vslam_world *world, int32_t **d_fuse_to, int32_t *state);

#ifdef __cplusplus
}
#endif

#endif
