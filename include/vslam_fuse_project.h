/* Geometric fusing: the points of an item projected into EVERY camera of the item that does not see them yet, and for each such
 * (point, camera) pair the best keypoint of that camera by descriptor distance inside a pixel window -- the search by projection
 * of vslam_search.h, once per camera, with nothing "taken" -- made one-to-one per keypoint, and reported with the point that
 * already HOLDS the keypoint, if one does.  A found pair whose keypoint has a holder says "these two points are one feature" (the
 * duplicates that never shared a keypoint, which vslam_fuse_points cannot see); one whose keypoint is free is a new observation of
 * its point.  ORB-SLAM calls the step SearchAndFuse.  An explicit call: nothing in any other header launches a kernel of this
 * file, and no existing output changes a bit.
 *
 * THIS TEXT and tests/ref_fuse_project.py are the contract.  ALL floating-point arithmetic is f64, never fused, in the written
 * order; f32 inputs are widened first.  Everything behind the disc test is integers.  Every choice is a minimum over integer keys,
 * so nothing depends on the order in which lanes or atomics arrive, and an item's bits depend on the item alone: the same in every
 * run, batch size and batch slot.
 *
 * An item.  n points P_i (d_points rows [x y z w] f32, w is not read), n = d_n_points clamped to 0 .. pt_stride; their observations
 * in CSR by point as vslam_cull_points takes them (d_obs_offsets [pt_stride + 1], d_obs_cam / d_obs_kp [obs_stride]) and the
 * descriptor of every CSR row as vslam_search_projection takes them (d_obs_desc [obs_stride][32]); C cameras taking the points'
 * coordinates to the camera, d_R [cam_stride][9] row-major and d_T [cam_stride][3] f64, C = d_n_cams clamped to 0 .. cam_stride;
 * per camera its keypoints d_xy [cam_stride][kp_stride][2] f32, d_desc [cam_stride][kp_stride][32] and their count d_n_kp
 * [cam_stride], each clamped to 0 .. kp_stride; optionally d_cam_mask [cam_stride]; h_K (row-major f32), width, height.
 *   1. Point i TAKES PART as in the cull: i < n, x, y, z finite, and 0 <= offsets[i] < offsets[i + 1] <= obs_stride.
 *   2. Camera c TAKES PART iff c < C, its R and T are finite, and (d_cam_mask is NULL or cam_mask[c] >= 0).
 *   3. A pair (i, c) of the two is TRIED iff point i has no VALID entry (vslam_fuse.h: 0 <= cam < cam_stride, 0 <= kp < kp_stride)
 *      with cam == c: a point already seen in a frame is never given a second keypoint there.
 *   4. A tried pair goes through steps 1 to 3 of vslam_search.h unchanged -- VISIBLE, CANDIDATES, CHOICE -- with camera c's pose
 *      and camera c's keypoints.  Nothing is taken: a keypoint that another point holds is a candidate.
 *   5. ONE-TO-ONE per (c, k): a keypoint proposed to by several points goes to the smallest (d0, i).  The others get nothing in
 *      that camera.
 *   6. The HOLDER of a found pair (i, c, k) is the smallest j < n with a valid CSR entry (c, k), or -1 when there is none.
 * Outputs.  The found pairs compacted in ascending (c, i) into d_found_point, d_found_cam, d_found_kp, d_found_dist (d0) and
 * d_found_holder [found_stride]; when more than found_stride are found, the first found_stride in that order are written;
 * d_n_found is the count written; slots from d_n_found on keep their bits.  d_stats [6] int32 per item, or NULL: [0] pairs tried,
 * [1] pairs visible, [2] pairs proposing, [3] pairs found before the clamp to found_stride, [4] of them with a holder, [5] pairs
 * written.
 * Broken CSR (as vslam_fuse.h defines it: offsets[0] < 0, an offset below its predecessor or above obs_stride, within offsets[0 ..
 * n]): the item has 0 found and zero stats.
 *
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (d_cam_mask, params and d_stats may be); batch,
 * pt_stride, obs_stride, cam_stride, kp_stride, found_stride, width or height not positive; radius_px not finite, not > 0 or > 64;
 * dist_threshold outside 1 .. 257; ratio10 outside 0 .. 10; a non-finite h_K; a pointer off its alignment: d_points, d_desc and
 * d_obs_desc 16 bytes; d_xy, d_R and d_T 8; every other array 4.  VSLAM_ERR_CAPACITY: kp_stride > VSLAM_MAX_KP, cam_stride > 1024,
 * batch > 65535, or width or height above 16384.
 *
 * Four launches behind one fill, stream-ordered on the context, no synchronisation: the CSR check and the holders (one workgroup
 * per item), the proposals (one workgroup per camera and 1024 points, the camera's keypoints binned into the grid of
 * vslam_search.h in LDS), the counts per camera, and the ordered fill.  Workspace from the context's grow-only arena, allocated on
 * the first call of a size and never afterwards: batch x (cam_stride x (12 kp_stride + 4 pt_stride + 32) + 4) bytes -- a 64-bit
 * key and a holder per keypoint slot, a proposal per (camera, point), eight counts per camera, a flag per item.
 *
 * ---- on the world: one explicit call for a world ATTACHED to `map` (vslam_map_attach_world); it does not run behind a step.  The
 * map's own arrays and its log never change -- they are the reference's --; everything here is state of the world beside the map.
 * vslam_world_fuse_project, per track: the points are d_world_points rows < d_sizes[track]; the CSR and its descriptors are the
 * world's (vslam_fuse.h, "THE WORLD'S CSR"); camera f is recorded frame f, formed from d_Twc as vslam_adjust.h forms "camera c" (C =
 * the frames recorded, cam_stride = max_frames); the cameras frame_lo <= f < frame_hi take part; the keypoints are the caller's:
 * d_xy [tracks][xy_frames][kp_stride][2], d_desc [tracks][xy_frames][kp_stride][32], d_n_kp [tracks][xy_frames], xy_frames >= the
 * frames recorded; found_stride = obs_capacity.  It then
 *   1. runs the kernels above;
 *   2. APPENDS every found pair, in output order, to the world's EXTRA LOG: d_extra_point, d_extra_frame, d_extra_kp
 *      [tracks][obs_capacity], d_extra_desc [tracks][obs_capacity][32] (the keypoint's descriptor, copied from d_desc) and d_n_extra
 *      [tracks].  The log is made by the first call and freed with the world; pairs past its capacity are dropped from the end;
 *   3. does exactly what vslam_world_fuse does: a new d_fuse_to, and NaN rows for the newly absorbed points.
 * State bit 2 of vslam_world_fusion_view means "extras exist"; vslam_world_reset and vslam_map_reset empty the log and clear the
 * bit.  vslam_world_fuse_project_view hands out the log (every pointer NULL and *capacity 0 while no extras exist).
 * THE WORLD'S CSR ONCE EXTRAS EXIST.  The input of the fusion (wherever vslam_fuse.h forms the world's CSR) is the map's log with each
 * point's extras appended to its row, in the order they were appended; the longest prefix of the extra log is admitted with which
 * the total stays within obs_capacity.  Then follows the same fusion with d_mask = d_fuse_to; descriptors are gathered through
 * d_out_src from the map's or from d_extra_desc.  An extra on a keypoint that another point holds is therefore a shared
 * observation, and the existing rule unites the two points; an extra on a free keypoint is a new observation of its point.
 * vslam_world_search, _relocalise, _adjust, _cull, _retriangulate and _observations see both and do not change.  A world without
 * extras makes exactly the launches it made before this header existed.
 * d_stats [tracks][8] int32 or NULL: the six above, the extras appended by this call, the extras held afterwards.
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (search and d_stats may be), a world that is not the one
 * attached to that map or has not as many frames, xy_frames below the frames recorded, not 0 <= frame_lo <= frame_hi <= the frames
 * recorded, width or height not positive, parameters out of range, a non-finite h_K, d_xy off 8 bytes, d_desc off 16, another
 * array off 4, a log made for another obs_capacity.  VSLAM_ERR_CAPACITY: max_frames > 1024, more than 65535 tracks, width or
 * height above 16384.
 * Launches: the world's CSR with descriptors, the cameras (one), the mask (one), the four above behind their fill, the append (one),
 * vslam_world_fuse's -- in which, as wherever the world's CSR is formed from now on, one merge launch sits in front of the fusion
 * and the descriptors' gather reads the log too.  Workspace from the arena: the kernels' own plus tracks x (map_capacity + 7
 * obs_capacity + max_frames + 11) x 4 + tracks x obs_capacity x 32 + tracks x max_frames x 96 bytes, and wherever the world's CSR is
 * formed tracks x (3 map_capacity + 1 + 3 obs_capacity) x 4 more.
 *
 * Left open: fusing across tracks (one point list per track remains); a depth or viewing-angle test on links; running behind a
 * step; several rounds in one call; tuning of radius and distance on footage -- nothing here has seen real footage.            */
#ifndef VSLAM_FUSE_PROJECT_H
#define VSLAM_FUSE_PROJECT_H

#include "vslam_amd.h"
#include "vslam_search.h"

#ifdef __cplusplus
extern "C" {
#endif

int vslam_fuse_project(vslam_ctx *ctx,
        const float *d_points, const int32_t *d_n_points, int pt_stride,          /* [batch][pt_stride][4] f32, w not read    */
        const int32_t *d_obs_offsets, const int32_t *d_obs_cam, const int32_t *d_obs_kp, const uint8_t *d_obs_desc, int obs_stride,
                                                                /* [batch][pt_stride + 1], [batch][obs_stride] twice, [..][32] */
        const double *d_R, const double *d_T, const int32_t *d_n_cams, int cam_stride,   /* [batch][cam_stride][9], [..][3], [batch] */
        const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp, int kp_stride,
                                                  /* [batch][cam_stride][kp_stride][2] f32, [..][kp_stride][32], [batch][cam_stride] */
        const int32_t *d_cam_mask /* may be NULL: [batch][cam_stride], a camera with a value < 0 takes no part */,
        const float *h_K, int width, int height, int batch, const vslam_search_params *params /* NULL: defaults */,
        int32_t *d_found_point, int32_t *d_found_cam, int32_t *d_found_kp, int32_t *d_found_dist, int32_t *d_found_holder,
        int found_stride,                                                         /* five arrays [batch][found_stride]        */
        int32_t *d_n_found /* [batch] */, int32_t *d_stats /* [batch][6] or NULL */);

int vslam_world_fuse_project(vslam_ctx *ctx, vslam_world *world, vslam_map *map,
                             const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp, int xy_frames,
                                              /* [tracks][xy_frames][kp_stride][2] f32, [..][kp_stride][32], [tracks][xy_frames] */
                             const float *h_K, int width, int height, int frame_lo, int frame_hi,
                             const vslam_search_params *search /* NULL: defaults */, int32_t *d_stats /* [tracks][8] or NULL */);

/* the extra log: [tracks][*capacity] int32 three times, [tracks][*capacity][32], [tracks]; all NULL and 0 while no extras exist */
int vslam_world_fuse_project_view(vslam_world *world, int32_t **d_extra_point, int32_t **d_extra_frame, int32_t **d_extra_kp,
                                  uint8_t **d_extra_desc, int32_t **d_n_extra, int32_t *capacity /* may be NULL */);

#ifdef __cplusplus
}
#endif

#endif
