/*
 * vslam_amd.h — C ABI of the MI355X (gfx950) front-end: keypoint extraction + rBRIEF,
 * Hamming k=2 matching, RANSAC fundamental matrix, 2-D k-d tree build / radius query.
 *
 * This is the drop-in boundary for the per-frame hot path of rahulaggarwal965/vslam.
 * The reference has no FFI: its consumers include Frame.h / KDTree.h / RansacFilter.h and link
 * the objects (src/vslam.cpp:6-10).  The header-only adapters under include/vslam/ re-present
 * those C++ surfaces and call the entry points below; INTEGRATION.md shows the binding.
 * Each entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - Plain pointers and sizes only.  `d_` parameters are DEVICE pointers (HBM), `h_` are host.
 *   - Batched layout: item b of a batch lives at base + b * stride elements, with a per-item
 *     count array (device, int32).  "kp_stride" = keypoint slots per frame.
 *   - All device entry points are asynchronous on the context's stream and return a status;
 *     VSLAM_OK == 0.  There is NO CPU fallback: without a HIP device every call fails.
 *   - Descriptors are 32 bytes per keypoint (cv::ORB default), points are (x, y) float pairs
 *     (cv::Point2f), index pairs are (queryIdx, trainIdx) int32.
 *
 * Alignment of device pointers
 *   The caller's device memory may come from anywhere -- an allocation of its own, a slot of an arena, a slice of a larger
 *   batch -- but the kernels read some arrays in wider units than their element type.  A KIND of array has one requirement
 *   wherever it appears (the widest access any entry point makes through it, composite entry points included: what one entry
 *   point writes the next one reads):
 *     16 bytes   descriptors (d_desc*, d_obs_desc: uint4), the k-NN rows (d_knn: int4), homogeneous points (d_points4d,
 *                d_map_points, d_points, the d_out of vslam_world_lift: float4), both buffers of vslam_debug_stream_copy;
 *      8 bytes   keypoints and point pairs (d_xy*, d_queries, d_p1, d_p2: float2), index pairs (d_pairs, d_matches: int2),
 *                f64 arrays (d_stats, d_error);
 *      4 bytes   every other int32 / uint32 / float array: the alignment C gives its element type;
 *     any address  image planes in and out (d_bgr, d_bgr_cur, d_bgr_out, d_gray, d_blurred, the d_out of vslam_gaussian7),
 *                map colours (d_colors), the inlier mask (d_mask), the rBRIEF table (d_pattern), and what the copy calls move
 *                (d_dst, d_src, d_ptr).  The kernels behind these read and write bytes, load unaligned, or are chosen by the
 *                address: a plane on a 4- or 16-byte boundary whose width is a multiple of 4 or 16 gets the faster kernel,
 *                and every choice gives the same bits.
 *   A violated requirement is VSLAM_ERR_INVALID, and vslam_last_error names the argument.  The test is made on the host before
 *   the entry point queues anything or touches the context's workspaces: a refused call leaves every output byte as it was,
 *   and the context (or pipeline slot) is as usable as before.  Composite entry points (vslam_extract_features,
 *   vslam_match_features, vslam_frontend_*, vslam_track_sequences, vslam_map_step, the vslam_pipeline_submit_* forms) test
 *   all their arguments up front, members of `params` and `pose` included, so none of them fails half-way through a batch.
 *   Where an entry point slices an array per frame, pair or track, the slices lie kp_stride x 32 / 16 / 8 bytes (or whole
 *   elements) apart, so an aligned base aligns every slice: no stride can break it.  NULL passes every test (whether an
 *   argument may be NULL is said at the entry point).  It is the address that is tested, not whether it starts an allocation.
 *   tests/alignment_contract.py lists every pointer argument of this header with its requirement; tests/test_gpu_alignment.py
 *   holds the entry points to it.
 */
#ifndef VSLAM_AMD_H
#define VSLAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_OK 0
#define VSLAM_ERR_INVALID (-1)   /* bad argument (null pointer, size out of range)           */
#define VSLAM_ERR_HIP (-2)       /* a HIP runtime call failed; see vslam_last_error()         */
#define VSLAM_ERR_NO_DEVICE (-3) /* no gfx950 device visible                                 */
#define VSLAM_ERR_CAPACITY (-4)  /* a size exceeds what the kernels were built for           */
#define VSLAM_ERR_DEGENERATE (-5)/* input the reference leaves undefined (<2 train rows, <8 matches) */
#define VSLAM_ERR_COMM (-6)      /* RCCL is missing or one of its calls failed; see vslam_last_error()  */

#define VSLAM_DESC_BYTES 32
#define VSLAM_SET_SIZE 8         /* RansacFilter draws 8-subsets: src/RansacFilter.cpp:17    */
#define VSLAM_MAX_KP 16384       /* keypoint slots per frame the match key packing supports  */

typedef struct vslam_ctx vslam_ctx;

/* ------------------------------------------------------------------ context */
int vslam_ctx_create(int device, vslam_ctx **out);
int vslam_ctx_destroy(vslam_ctx *ctx);
/* HIP's current device is per host thread: vslam_ctx_create leaves the context's device current on the creating thread, and
 * every call on a context (allocation included) expects it to be.  A thread that did not create the context -- or that has
 * since worked on another device -- calls this first.                                                                      */
int vslam_ctx_make_current(vslam_ctx *ctx);
/* Borrow a caller-owned hipStream_t (e.g. torch's current stream).  Taken literally: NULL is
 * HIP's default stream.  A fresh context runs on a private non-blocking stream.
 *
 * Stream order.  "Stream-ordered" and "asynchronous on the context's stream" mean the same three things for every entry point,
 * whatever streams of its own the library uses inside (an auxiliary stream for the blur, the rBRIEF table rotation, the k-d
 * build and the generator's prefetch; a copy stream for vslam_upload_async):
 *   - device inputs are read no earlier than the work that was queued on the context's stream before the call: a producer
 *     may queue the kernels that fill them and the entry point on that stream and never stop the host;
 *   - outputs and resident state (maps, worlds, the context's workspaces) are complete for work queued on that stream after
 *     the call, and no input is read any more by then: the caller may recycle every array in stream order;
 *   - host arguments (h_K, h_c1 / h_c2, h_view, the vslam_extract_params and vslam_pose_outputs structs) are consumed before
 *     the call returns.
 * The call itself does not wait for the device.  The entry points that do: vslam_ctx_synchronize, vslam_ctx_wait,
 * vslam_ctx_set_stream (for the stream it leaves), vslam_ctx_destroy, vslam_corner_stats, vslam_prof_count / _enable / _reset
 * (when timed launches are pending), vslam_copy_h2d, vslam_copy_d2h, vslam_upload_wait (the copy stream only), vslam_dev_free,
 * vslam_host_free, vslam_map_destroy, vslam_world_destroy, vslam_pipeline_acquire / _submit_* (for the slot's previous batch),
 * vslam_pipeline_wait / _drain / _destroy -- and any entry point on its first call at a larger shape, when a workspace of the
 * context has to grow.  vslam_upload_async is the one exception to the first rule: it runs on the copy stream, beside what
 * is queued, and vslam_upload_fence orders later work behind it.  tests/test_gpu_stream_order.py holds every entry point to
 * this behind a stalled stream: deterministically where work could start too early, and as far as timing shows it where a
 * wait for the library's own streams could come too late (they cannot be held back from outside).         */
int vslam_ctx_set_stream(vslam_ctx *ctx, void *hip_stream);
/* Waits for the context's stream, then reads AND CLEARS the device-side error word (VSLAM_ERR_CAPACITY if a bounded list
 * overflowed since the last call).  Not for a context that a vslam_pipeline owns: there the word belongs to the ticket in
 * flight (vslam_pipeline_commit files it under the batch), and clearing it out of band would take that batch's status away --
 * use vslam_ctx_wait / vslam_pipeline_wait on those.                                                                       */
int vslam_ctx_synchronize(vslam_ctx *ctx);
/* Waits for the context's stream and nothing else (vslam_ctx_synchronize also fetches the device-side error word). */
int vslam_ctx_wait(vslam_ctx *ctx);
const char *vslam_last_error(vslam_ctx *ctx);
/* Diagnostics of the corner detector's LAST batch on this context (vslam_extract_features / vslam_frontend_* /
 * vslam_good_features); waits for the context's stream.  h_stats[0] = frames, [1] = pixels per frame, [2] = pixels the certified
 * cheap tier listed as possible corners, summed over the frames (the reference's exact arithmetic runs on these only),
 * [3] = frames whose bounded list overflowed and were redone from whole-image scratch, [4] = scratch sets in the pool (more
 * overflowing frames than this in one call: VSLAM_ERR_CAPACITY).  What bench.py reports per data regime.                   */
int vslam_corner_stats(vslam_ctx *ctx, uint64_t h_stats[5]);
/* Device memory the context's grow-only workspaces hold at the moment (bytes; what a batch shape costs beside its own
 * inputs and outputs).                                                                                    */
int vslam_ctx_workspace_bytes(vslam_ctx *ctx, size_t *bytes_out);
/* Diagnostics of those workspaces.  The rule every entry point is held to (tests/test_gpu_workspace.py): what a
 * call writes is a function of its arguments and of the resident state it is handed (maps, worlds), never of what an earlier
 * call left in a workspace.  The named slots whose name begins with "ctx." are the only ones that carry anything from one call
 * to the next (the default rBRIEF table, the sticky error word, a calibration target).
 *   vslam_ctx_workspace_fill   queues one memset of `byte` (0 .. 255) per slot on the context's stream, stream-ordered like any
 *       other call, no synchronisation; the "ctx." slots are left alone.  The next call of every entry point must give the bits it
 *       gives on any other workspace contents.  vslam_corner_stats and the vslam_debug_* read-backs report a workspace's
 *       contents and so report the fill when they are read behind it.
 *   vslam_ctx_workspace_slots  the slots as text, one line "name bytes\n" per slot in name order, NUL-terminated, cut to `cap`
 *       bytes when it is longer; *needed = the bytes the whole text takes, the NUL included.  buf may be NULL when cap is 0.  */
int vslam_ctx_workspace_fill(vslam_ctx *ctx, int byte);
int vslam_ctx_workspace_slots(vslam_ctx *ctx, char *buf, size_t cap, size_t *needed);
const char *vslam_version(void);
/* ORB's learned rBRIEF test pairs (OpenCV `bit_pattern_31_`, the table behind cv::ORB::compute, src/Frame.cpp:57,68):
 * HOST pointer to 256 x (x0, y0, x1, y1) int8, static storage.  Every d_pattern argument below accepts NULL for a
 * device copy of this table that the context keeps; other tables (tests, wider patches) are passed explicitly.       */
const int8_t *vslam_brief_pattern_31(void);
/* Context options.
 *   VSLAM_OPT_RANSAC_ALL_SUMS  0 (default): vslam_ransac_* compute what find_fundamental's accept rule can observe
 *       (src/RansacFilter.cpp:59: a hypothesis matters only if its inlier count is the pair's maximum, and its
 *       residual sum only breaks ties among those).  Every hypothesis that reaches the maximum count is counted in
 *       full and exactly; a hypothesis is abandoned as soon as it can no longer reach a count already verified for
 *       the pair -- or (round 4) can at best TIE such a count while a certified bound puts its residual sum below
 *       that of a hypothesis verified to reach it: among equal counts the rule keeps the larger sum, so it can neither
 *       win nor tie.  d_hyp_count holds the maximum for the hypotheses that reach it -- except for those abandoned on
 *       the sum -- and -1 for all others; d_hyp_sum holds the exact sum where it can still decide the winner, -inf for
 *       maximum-count hypotheses a certified bound places below the winner's, NaN where the count is -1.  Winner,
 *       mask, F and matches are the reference's either way.
 *       1: the count and the residual sum of EVERY hypothesis are computed as the reference does (:105-140) — what
 *       the per-hypothesis parity tests ask for; about 3x the scoring time.
 *   VSLAM_OPT_RANSAC_MIN_MATCHES  8 (default) .. 1: vslam_ransac_evaluate skips items with fewer matches than this
 *       (no model: winner -1).  find_fundamental needs 8 to draw a set (src/RansacFilter.cpp:24), but
 *       compute_fundamental_residual scores a GIVEN F on any number of matches (:105-140): its adapter sets 1.
 *   VSLAM_OPT_RANSAC_SOLVER  0 (default): compute_fundamental as the reference computes it (OpenCV's Jacobi SVD replayed
 *       operation by operation; bit-exact with the oracle).  1: opt-in APPROXIMATE solver for throughput experiments
 *       (BASELINE.json configs[4]): conditioned 9x9 normal matrix on the matrix cores (v_mfma_f32_16x16x4_f32) +
 *       inverse iteration.  NOT bit-exact: F equals the exact solver's up to sign and about 1e-4 (unit-norm F) on
 *       well-conditioned samples; inlier masks may differ.  Never used unless set.
 *   VSLAM_OPT_MATCH_SHAPE  0 (default, and the only value the product library accepts: 8 waves x 32 query rows).
 *       EXPERIMENTS build (libvslam_amd_exp.so, -DVSLAM_EXPERIMENTS) only: 1 the same, 2: 4 waves x 64 query rows.  Same
 *       results bit for bit; kept there so that the choice can be re-measured (tools/ab_match.sh).                 */
#define VSLAM_OPT_RANSAC_ALL_SUMS 1
#define VSLAM_OPT_RANSAC_MIN_MATCHES 2
#define VSLAM_OPT_RANSAC_SOLVER 3
#define VSLAM_OPT_MATCH_SHAPE 4
/*   VSLAM_OPT_CORNER_WINDOW_PCT  135 (default): how many of the detector's possible corners get the exact arithmetic
 *       at once, in percent of max_corners (+ 128).  The selection ranks about 1.3 x max_corners candidates; a frame
 *       whose selection needs more than were evaluated is redone with all of them, so the value changes speed, never
 *       results (0 = always everything; a small value forces the redo: a test knob).                              */
#define VSLAM_OPT_CORNER_WINDOW_PCT 5
/*   VSLAM_OPT_RANSAC_MIN_ITEMS  8 (default) .. 0: RansacFilter::min_items.  initialize_sets draws min_items indices
 *       without replacement into sets that are 8 wide whatever min_items is (src/RansacFilter.cpp:17,22): entries
 *       min_items .. 7 stay 0 and find_fundamental uses all 8 (:49-53).  Values above 8 overrun the set in the
 *       reference and are rejected here.                                                                          */
#define VSLAM_OPT_RANSAC_MIN_ITEMS 6
/*   VSLAM_OPT_CORNER_LIST_CAP  0 (default): the corner detector's per-frame lists hold 16 x max_corners + 4096 entries
 *       (image data lists about 10 x max_corners).  A frame that needs more (response plateaus, pure noise) is redone
 *       from whole-image scratch taken from a pool of max(4, frames / 16) (at most 64) sets: the results never depend on
 *       the bound.  Only if more frames of ONE call overflow than the pool has sets do those frames come back without
 *       corners, and vslam_ctx_synchronize returns VSLAM_ERR_CAPACITY.  n > 0: n entries per frame (a test knob);
 *       -1: every list sized for the whole image, as before round 4 (nothing can overflow; 16 bytes per pixel and frame). */
#define VSLAM_OPT_CORNER_LIST_CAP 7
/*   VSLAM_OPT_MATCH_FORM  0 (default) / 1: the matcher forms Hamming distances as FP4 (+-1) dot products on the matrix
 *       cores (v_mfma_scale_f32_32x32x64_f8f6f4).  EXPERIMENTS build only: 2 = as int8 (0 / 1) dot products
 *       (v_mfma_i32_32x32x32_i8); the product library carries the FP4 kernel alone and answers 2 with VSLAM_ERR_INVALID.
 *       Exact either way, same results bit for bit.                                                                */
#define VSLAM_OPT_MATCH_FORM 8
/*   VSLAM_OPT_TREE_FORK  where vslam_frontend_pairs / _sequence start the k-d build (an output of the path that no later
 *       stage reads) on the auxiliary stream: -1 (default) by size (behind the matcher up to 2048 keypoint slots, in front
 *       of it above), 0 in front of the matcher, 1 behind it, 2 behind the set mapping, 3 behind the 8-point solves,
 *       4 behind the screen, 5 not forked at all (in line on the main stream, at the end of extraction).  The call's last
 *       kernel waits for it.  Same results; a tuning knob.                                                             */
#define VSLAM_OPT_TREE_FORK 9
/*   VSLAM_OPT_POSE_REFIT  0 (default): nothing changes.  1: vslam_frontend_pairs_pose (and so vslam_pipeline_submit_pairs_pose)
 *       and vslam_track_sequences run vslam_refit_fundamental on d_F, in place, between RANSAC and extract_Rt / the map steps:
 *       the pose, triangulation, filter and map stages get the refitted F, d_F holds it (so do records packed from it);
 *       d_best, d_matches and the inlier set are what they are without the option.                                       */
#define VSLAM_OPT_POSE_REFIT 10
/*   VSLAM_OPT_POSE_REFINE  0 (default): nothing changes, no launch is added.  1: vslam_frontend_pairs_pose (and so
 *       vslam_pipeline_submit_pairs_pose) runs vslam_refine_pairs in place on d_R / d_t / d_c2 / d_points4d between the
 *       triangulation and the reprojection filter, with gate_sq = 4 x reproj_threshold_sq and 20 iterations: the filter and the
 *       caller get the adjusted pose and points.  vslam_map_step / vslam_track_sequences triangulate directly after extract_Rt
 *       and run the same adjustment there, so the pose entered into the map, the association, the filter and the appended points
 *       all use the adjusted values.  Comes after VSLAM_OPT_POSE_REFIT when both are on.  Any other value: VSLAM_ERR_INVALID. */
#define VSLAM_OPT_POSE_REFINE 11
int vslam_ctx_set_option(vslam_ctx *ctx, int option, int value);

/* device memory + copies for hosts that have no other allocator (the C++ adapters) */
int vslam_dev_alloc(vslam_ctx *ctx, size_t bytes, void **d_out);
int vslam_dev_free(vslam_ctx *ctx, void *d_ptr);
int vslam_copy_h2d(vslam_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int vslam_copy_d2h(vslam_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* Frame ingest (what replaces cv::VideoCapture's per-frame host Mat, src/vslam.cpp:54-60).
 * Page-locked host buffers and uploads that run on the context's copy stream beside the kernels:
 *   vslam_host_alloc / vslam_host_free   page-locked host memory (hipHostMalloc)
 *   vslam_upload_async                   enqueue host -> device on the copy stream (returns at once)
 *   vslam_upload_fence                   later work on the compute stream waits for every upload enqueued so far
 *   vslam_upload_wait                    the calling thread waits for them (before a host buffer is refilled)  */
int vslam_host_alloc(vslam_ctx *ctx, size_t bytes, void **h_out);
int vslam_host_free(vslam_ctx *ctx, void *h_ptr);
int vslam_upload_async(vslam_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int vslam_upload_fence(vslam_ctx *ctx);
int vslam_upload_wait(vslam_ctx *ctx);
/* The way back: device -> host on the context's COMPUTE stream, behind everything queued on it so far (the result copy that
 * closes a batch).  Returns at once; the bytes are there when the stream has been waited for (vslam_ctx_wait /
 * vslam_ctx_synchronize / vslam_pipeline_wait).  Page-locked h_dst keeps the copy asynchronous.                          */
int vslam_download_async(vslam_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* per-kernel timing with HIP events on the context's stream (bench.py's roofline leg) */
int vslam_prof_enable(vslam_ctx *ctx, int on);
int vslam_prof_reset(vslam_ctx *ctx);
int vslam_prof_count(vslam_ctx *ctx);   /* synchronises, folds pending events, returns #kernels */
int vslam_prof_get(vslam_ctx *ctx, int i, char *name, int name_cap, double *total_ms, int64_t *launches);

/* profiling aid: a plain streaming copy of `bytes` (multiple of 16) with 4 or 16 bytes per lane, so
 * rocprofv3's FETCH_SIZE / WRITE_SIZE can be calibrated on a known byte count per access width */
/* d_src, d_dst: 16-byte aligned (VSLAM_ERR_INVALID otherwise). */
int vslam_debug_stream_copy(vslam_ctx *ctx, const void *d_src, void *d_dst, size_t bytes, int bytes_per_lane);
/* profiling aid: a kernel that keeps every SIMD's vector pipe busy for its whole duration (8 waves per SIMD of independent
 * v_fma_f32), so that rocprofv3's SQ_ACTIVE_INST_VALU / GRBM_GUI_ACTIVE ratio that means "vector pipe 100 % busy" is measured
 * rather than assumed (tools/sq_summary.py) */
int vslam_debug_valu_calib(vslam_ctx *ctx);

/* ----------------------------------------------------------------- matching */
/* Replaces match_features' front half, src/Frame.cpp:83-94:
 *   BFMatcher(NORM_HAMMING)->knnMatch(desc1, desc2, k=2) + `m[0].distance < m[1].distance*0.7`.
 * d_desc1/d_desc2: [batch][kp_stride][32] u8; d_n1/d_n2: [batch] int32.
 * d_pairs: [batch][kp_stride][2] int32 (queryIdx, trainIdx) in query order; d_m: [batch].
 * Optional d_knn (may be NULL): [batch][kp_stride][4] int32 = idx0, dist0, idx1, dist1.
 * Items with fewer than 2 train rows produce m = 0 (the reference reads m[1] regardless).
 * Alignment: d_desc1, d_desc2, d_knn 16 bytes, d_pairs 8, the counts 4 (VSLAM_ERR_INVALID otherwise).    */
int vslam_match_knn2_ratio(vslam_ctx *ctx, const uint8_t *d_desc1, const int32_t *d_n1,
                           const uint8_t *d_desc2, const int32_t *d_n2, int batch, int kp_stride,
                           int32_t *d_pairs, int32_t *d_m, int32_t *d_knn);

/* ------------------------------------------------------------------- RANSAC */
/* Replaces RansacFilter::initialize_sets, src/RansacFilter.cpp:6-34, with the seed injected
 * (std::mt19937(seed) + libstdc++ uniform_int_distribution, draws without replacement).
 * d_seeds: [batch] u32; d_m: [batch] matches per item; d_sets: [batch][hyp][8] int32.
 * d_draw_scratch: [batch][hyp*8] u32 workspace.  Items with m < 8 get all-zero sets.
 * Alignment: 4 bytes for all four arrays.                                                     */
int vslam_ransac_sets(vslam_ctx *ctx, const uint32_t *d_seeds, const int32_t *d_m, int batch,
                      int hyp, int32_t *d_sets, uint32_t *d_draw_scratch);

/* Replaces RansacFilter::find_fundamental (+ compute_fundamental, compute_fundamental_residual),
 * src/RansacFilter.cpp:36-140, for pre-drawn sets, and match_features' back half
 * (src/Frame.cpp:96-102: keep the winner's inlier matches).
 * d_xy1/d_xy2: [batch][kp_stride][2] f32; d_pairs/d_m as produced by vslam_match_knn2_ratio.
 * Outputs: d_F [batch][9] f32 (row-major 3x3, untouched when no hypothesis is accepted),
 *          d_mask [batch][kp_stride] u8, d_best [batch][4] int32 = winner, count, bits(sum), n_out,
 *          d_matches [batch][kp_stride][2] int32 compacted inlier matches (n_out of them).
 * Workspaces: d_hypF [batch][hyp][9] f32, d_hyp_count [batch][hyp] int32, d_hyp_sum [batch][hyp] f32
 * (also the per-hypothesis outputs the parity tests read: every F always; every count and sum
 * with VSLAM_OPT_RANSAC_ALL_SUMS, otherwise those of the maximum-count hypotheses, see above).
 * Alignment (here and for vslam_ransac_solve / _evaluate): d_xy1, d_xy2, d_pairs, d_matches 8 bytes, d_mask any address,
 * every other array 4 (VSLAM_ERR_INVALID otherwise).                                           */
int vslam_ransac_fundamental(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2,
                             const int32_t *d_pairs, const int32_t *d_m, const int32_t *d_sets,
                             int batch, int kp_stride, int hyp, float threshold, float *d_F,
                             uint8_t *d_mask, int32_t *d_best, int32_t *d_matches, float *d_hypF,
                             int32_t *d_hyp_count, float *d_hyp_sum);

/* The two halves of vslam_ransac_fundamental, exposed because RansacFilter's public surface has
 * them as separate methods:
 *   vslam_ransac_solve     = compute_fundamental for every set (src/RansacFilter.cpp:69-103)
 *   vslam_ransac_evaluate  = compute_fundamental_residual for every given hypothesis (:105-140) +
 *                            the accept rule of find_fundamental (:59) + the winner's mask/matches.
 * With hyp = 1 they are the single-call forms of those methods.                               */
int vslam_ransac_solve(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const int32_t *d_pairs,
                       const int32_t *d_m, const int32_t *d_sets, int batch, int kp_stride, int hyp,
                       float *d_hypF);
int vslam_ransac_evaluate(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2,
                          const int32_t *d_pairs, const int32_t *d_m, const float *d_hypF, int batch,
                          int kp_stride, int hyp, float threshold, float *d_F, uint8_t *d_mask,
                          int32_t *d_best, int32_t *d_matches, int32_t *d_hyp_count, float *d_hyp_sum);

/* The step find_fundamental leaves undone (src/RansacFilter.cpp:36-67 returns the winner as fitted to its 8 sampled,
 * un-normalised points; `//TODO: normalize` at :40): the winning F refitted over ALL its inliers.  THIS TEXT and
 * tests/ref_refit.py are the contract.
 * Inputs per item b: the compacted inlier matches d_matches[b][0 .. n), n = d_best[b][3] (clamped to 0 .. kp_stride), as
 * vslam_ransac_evaluate / vslam_match_features write them, into d_xy1 / d_xy2 [batch][kp_stride][2]; d_F_in [batch][9].  A match
 * with an index outside 0 .. kp_stride - 1 is skipped and not counted.  Every f32 input is widened to f64 and ALL arithmetic
 * is f64, never fused:
 *   1. Hartley normalisation per image: c = centroid, d = mean Euclidean distance to c, s = sqrt(2) / d,
 *      T = [[s, 0, -s c.x], [0, s, -s c.y], [0, 0, 1]];
 *   2. M = A^t A (9 x 9) over the normalised correspondences, the rows of A as in src/RansacFilter.cpp:81-89:
 *      u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1;
 *   3. f = the eigenvector of M's smallest eigenvalue by cyclic Jacobi (rows (0,1), (0,2) .. (7,8)), until
 *      sqrt(sum of the squared off-diagonal entries) <= 2^-52 * trace or 30 sweeps; Fh = f as a row-major 3 x 3;
 *   4. rank 2: the SVD of Fh (one-sided Jacobi), the smallest singular value set to 0, recomposed;
 *   5. F = T2^t Fh T1, divided by its Frobenius norm;
 *   6. negated if sum F_ij * F_in_ij < 0 (F_in is the RANSAC winner: the refit continues it);
 *   7. rounded once to f32 into d_F_out [batch][9] (may be d_F_in itself).
 * An item is LEFT ALONE -- d_F_out[b] = d_F_in[b] bit for bit, written by the same kernel -- when there is no winner
 * (d_best[b][0] < 0), when fewer than 8 correspondences are counted, when d == 0 in either image, or when an entry of the
 * result is not finite.  None of this raises the error word.
 * d_stats (may be NULL) [batch][4] f64: [0] correspondences used; [1] the mean TRUE Sampson distance
 * e^2 / (Fx1_0^2 + Fx1_1^2 + Ftx2_0^2 + Ftx2_1^2), e = x2^t F x1, of those correspondences under F_in (not the expression of
 * src/RansacFilter.cpp:126); [2] the same under F_out as written (the f32 values); [3] lambda_9 / lambda_8 of M, smallest over
 * second smallest eigenvalue (near 1: the null vector is not isolated).  For an item left alone [0] is the count that was
 * found and [1..3] are NaN.
 * Deterministic: no floating-point atomics; every sum is a strided partial sum per lane (256 lanes), a butterfly inside the
 * wave, then the wave sums in wave order -- the order depends on n alone, so a pair gives the same bits in every run, in any
 * batch, at any position.  One workgroup per item, any n up to kp_stride.
 * Stream-ordered on the context; allocates nothing and does not synchronise.  VSLAM_ERR_INVALID, before anything is queued,
 * for a null pointer (d_stats excepted), batch <= 0 or kp_stride <= 0, or an argument off its alignment: d_xy1, d_xy2,
 * d_matches, d_stats 8 bytes, the others 4.                                                                               */
int vslam_refit_fundamental(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const int32_t *d_matches,
                            const int32_t *d_best, int batch, int kp_stride, const float *d_F_in,
                            float *d_F_out /* may alias d_F_in */, double *d_stats /* [batch][4], may be NULL */);

/* Two-view bundle adjustment of each pair's pose and points: the step the reference left as an empty `struct optimizer`
 * (src/optimzer.cpp).  Within one pair there is one fixed camera [K | 0], one free camera K [R | t] and the pair's own points;
 * the sum of the squared reprojection errors in both images is minimised over R, t (|t| = 1) and the points by
 * Levenberg-Marquardt on the Schur-reduced 5 x 5 system.  THIS TEXT and tests/ref_refine.py are the contract.
 * Inputs per item b: the compacted inlier matches d_matches[b][0 .. n), n = d_best[b][3] clamped to 0 .. kp_stride, into
 * d_xy1 / d_xy2 [batch][kp_stride][2]; d_R [batch][9] (row-major), d_t [batch][3] as vslam_extract_Rt wrote them;
 * d_points4d [batch][kp_stride][4] as vslam_triangulate wrote them (x, y, z, 1 in match slot i; the fourth entry is not read);
 * h_K: 9 floats on the host, row-major.  Every f32 input is widened to f64 and ALL arithmetic is f64, never fused.  A match with
 * an index outside 0 .. kp_stride - 1 is skipped.
 * Projection of a point Y in camera coordinates: q_r = (K_r0 Y_0 + K_r1 Y_1) + K_r2 Y_2, (u, v) = (q_0 / q_2, q_1 / q_2).  In the
 * first image Y = X; in the second Y = RX + t with (RX)_r = (R_r0 X_0 + R_r1 X_1) + R_r2 X_2.  The error of a match in an image
 * is (u - x)^2 + (v - y)^2 against its keypoint (x, y).
 *   1. PARTICIPATING matches, fixed once: X finite, X_2 > 0, (RX + t)_2 > 0 and the error <= gate_sq in each image separately,
 *      all under the inputs as given.  The objective is the sum of both errors over the participating matches.
 *   2. Start: R0 = R (3 I - R^t R) / 2 (one Newton step of the polar iteration: R comes from f32), t0 = t / |t|, the points as
 *      given; lambda = 1e-3.
 *   3. One iteration at (R, t, X), residual r = projection - keypoint.  Per point, with A(Y) = d(u, v)/dY =
 *      [K_0. - u K_2. ; K_1. - v K_2.] / q_2:  J1x = A(X);  J2x = A(Y) R;  Jc = A(Y) [ -[RX]x | b1 | b2 ] (2 x 5), where e_k is the
 *      axis of the smallest |t_k| (the lowest k on a tie), b1 = normalize(t x e_k), b2 = t x b1;
 *      V = J1x^t J1x + J2x^t J2x, W = Jc^t J2x (5 x 3), g_x = J1x^t r_1 + J2x^t r_2, g_c = Jc^t r_2;
 *      damping (Marquardt): V*_kk = V_kk + lambda max(V_kk, 2^-40), and the diagonal of Jc^t Jc times (1 + lambda) (no floor:
 *      a reduced system that is not positive definite refuses the step);  V* = L L^t by Cholesky, Yv = V*^-1 W^t, z = V*^-1 g_x;
 *      S = sum (Jc^t Jc, damped) - W Yv  (15 sums), rhs = sum g_c - W z (5 sums);  S dc = -rhs by Cholesky;
 *      dX = -(z + Yv dc) per point.  A pivot that is not > 0 in any V* or in S, or a dc that is not finite, refuses the step.
 *   4. Candidate: R' = exp([w]x) R with w = dc[0..3): theta^2 = w.w; below 2^-26: a = 1 - theta^2 / 6, b = 1/2 - theta^2 / 24,
 *      otherwise a = sin(theta) / theta, b = 2 sin^2(theta / 2) / theta^2; exp = I + a [w]x + b (w w^t - theta^2 I).
 *      t' = normalize(t + dc[3] b1 + dc[4] b2);  X' = X + dX.
 *   5. Accepted iff every participating point has X'_2 > 0 and (R'X' + t')_2 > 0 and the objective at the candidate is strictly
 *      lower (a NaN never is).  Accepted: lambda = max(lambda / 10, 1e-15), and the run ends when (old - new) / old < 2^-40.
 *      Refused: lambda = 10 lambda, and the run ends when lambda > 1e12.  At most max_iterations iterations.
 *   6. Rounded once to f32: d_R, d_t; d_c2[r][c] = (K_r0 M_0c + K_r1 M_1c) + K_r2 M_2c with M = [R | t] in f64; (x, y, z, 1) in
 *      the participating matches' slots of d_points4d.  Every other slot keeps its bits.
 * An item is LEFT ALONE -- d_R, d_t and d_points4d keep their bits, d_c2 is the formula of 6 on the inputs, all written by the
 * same kernel -- when there is no winner (d_best[b][0] < 0), when fewer than 8 matches participate, when t has an entry that is
 * not finite or |t| = 0, when no step was accepted, or when an output entry is not finite.  None of this raises the error word.
 * d_stats (may be NULL) [batch][4] f64: [0] participating matches; [1] their mean squared reprojection error under the inputs
 * (the objective over twice the count); [2] the same under the outputs as written (the f32 values); [3] accepted steps.  For an
 * item left alone [0] is the count that was found and [1..3] are NaN.
 * Deterministic: no floating-point atomics; every sum (the 15 + 5 entries of the reduced system, the objective) is a strided
 * partial sum per lane (256 lanes, lane l takes the matches i = l mod 256 in rising order), a butterfly inside the wave, then
 * the four wave sums in wave order: a pair gives the same bits in every run, in any batch, at any position.  A point's f64
 * coordinates stay in f64 between iterations (in LDS, or in a workspace of the context's grow-only arena when n is above 3200).
 * Stream-ordered on the context; does not synchronise.  VSLAM_ERR_INVALID, before anything is queued, for a null pointer
 * (d_stats excepted), batch <= 0, kp_stride <= 0, max_iterations outside 1 .. 64, gate_sq not finite or <= 0, or an argument
 * off its alignment: d_points4d 16 bytes, d_xy1, d_xy2, d_matches, d_stats 8, the others 4.                                  */
int vslam_refine_pairs(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const int32_t *d_matches, const int32_t *d_best,
                       int batch, int kp_stride, const float *h_K, float gate_sq, int max_iterations,
                       float *d_R /* [batch][9] in/out */, float *d_t /* [batch][3] in/out */, float *d_c2 /* [batch][12] out */,
                       float *d_points4d /* [batch][kp_stride][4] in/out */, double *d_stats /* [batch][4], may be NULL */);

/* ------------------------------------------------------------------ k-d tree */
/* Replaces construct_kdtree(frame_kdtree&, points), src/KDTree.cpp:107-143.  The tree is the
 * reference's pre-order node array reduced to its pt_index column: d_nodes [batch][kp_stride].
 * Child positions are implicit (left subtree len/2 nodes, right len - len/2 - 1).  Tie placement
 * reproduces libstdc++'s std::nth_element (introselect) exactly.  A tree is built in one workgroup's
 * LDS, 14 bytes per slot (two float coordinates, a 16-bit index, two 16-bit partition lists) and 4 more,
 * rounded up to 16, within 160 KB less 512 bytes: 14 * kp_stride + 4 <= 163328, that is
 * kp_stride <= VSLAM_KDTREE_MAX_KP = 11666, VSLAM_ERR_CAPACITY beyond — which is also the limit of
 * vslam_extract_features / vslam_frontend_* when they are asked for the trees (d_nodes != NULL).
 * Alignment, for all four k-d entry points: d_xy and d_queries 8 bytes, every other array 4.      */
#define VSLAM_KDTREE_MAX_KP 11666
int vslam_kdtree_build(vslam_ctx *ctx, const float *d_xy, const int32_t *d_n, int batch,
                       int kp_stride, int32_t *d_nodes);
/* Replaces radius_search(frame_kdtree, points, query, radius), src/KDTree.cpp:145-171.
 * d_queries [batch][q_stride][2], d_nq [batch]; hits in the reference's visit (pre-order) order:
 * d_hits [batch][q_stride][hit_cap] (first hit_cap only), d_counts [batch][q_stride] (true count). */
int vslam_kdtree_radius(vslam_ctx *ctx, const int32_t *d_nodes, const float *d_xy,
                        const int32_t *d_n, int batch, int kp_stride, const float *d_queries,
                        const int32_t *d_nq, int q_stride, float radius, int32_t *d_hits,
                        int32_t *d_counts, int hit_cap);

/* Replaces nearest(KDTree, query, max_distance_sq), src/KDTree.cpp:37-71, on the same pre-order
 * array: d_best_idx [batch][q_stride] = index of the nearest point, or -1 when none is closer than
 * max_distance_sq (the reference then returns a default-constructed {0,0} point).             */
int vslam_kdtree_nearest(vslam_ctx *ctx, const int32_t *d_nodes, const float *d_xy,
                         const int32_t *d_n, int batch, int kp_stride, const float *d_queries,
                         const int32_t *d_nq, int q_stride, float max_distance_sq,
                         int32_t *d_best_idx);

/* The points of a tree filed by integer pixel cell, for callers that ask ONE radius query at a time
 * (radius_search(frame.kdtree, frame.points, q, 2) once per in-view map point, src/vslam.cpp:146-160): a device round
 * trip per query costs 200 x the reference's pointer chase, a probe of this table on the host does not.
 * d_table [batch][slots][2] uint32 = {cell key ((floor(y) + 32768) << 16 | (floor(x) + 32768)), pre-order position},
 * 0xFFFFFFFF = empty; open addressing from ((key * 2654435761) >> 7) & (slots - 1), linear; every point owns a slot;
 * slots a power of two >= 2 * kp_stride.  d_ok [batch] = 0 when a coordinate does not fit the key (table unusable).
 * Hits of a radius query = the points of the cells floor(q - r) .. floor(q + r) with dx * dx + dy * dy < r * r, in
 * ascending pre-order position: exactly the reference's result and order (src/KDTree.cpp:151-171).              */
int vslam_kdtree_cell_table(vslam_ctx *ctx, const int32_t *d_nodes, const float *d_xy, const int32_t *d_n, int batch,
                            int kp_stride, int slots, uint32_t *d_table, int32_t *d_ok);

/* ---------------------------------------------------------------- extraction */
typedef struct vslam_extract_params {
    int32_t max_corners;     /* goodFeaturesToTrack maxCorners (3000 in src/Frame.cpp:61)      */
    double quality;          /* 0.01                                                           */
    double min_distance;     /* 3                                                              */
    float cos_a, sin_a;      /* steered-BRIEF rotation; KeyPoint(p,20) has angle -1 deg        */
    const int8_t *d_pattern; /* DEVICE [256][4] int8 (x0,y0,x1,y1) rBRIEF test pairs; NULL = ORB's
                                learned table (vslam_brief_pattern_31), what cv::ORB::compute
                                samples (src/Frame.cpp:57,68)                                  */
} vslam_extract_params;

/* Replaces extract_features(Frame&), src/Frame.cpp:53-80, for a batch of BGR frames:
 * cvtColor -> goodFeaturesToTrack -> ORB::compute (border filter, 7x7 blur, rBRIEF) -> kd-tree.
 * d_bgr: [frames][height][row_stride] u8 (3 bytes per pixel).
 * Outputs per frame: d_xy [frames][kp_stride][2], d_desc [frames][kp_stride][32],
 * d_nodes [frames][kp_stride] (may be NULL), d_n [frames] kept keypoints, d_n_detected [frames]
 * (the pre-filter count that sizes map_point_ids, src/Frame.cpp:73).
 * Alignment: d_bgr and params->d_pattern any address (any row_stride >= 3 * width as well); d_desc 16 bytes, d_xy 8,
 * d_nodes, d_n, d_n_detected 4 -- all tested before the first stage is queued.               */
int vslam_extract_features(vslam_ctx *ctx, const uint8_t *d_bgr, int frames, int width, int height,
                           int row_stride, const vslam_extract_params *params, int kp_stride,
                           float *d_xy, uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n,
                           int32_t *d_n_detected);

/* Replaces extract_features(Frame&, nrows, ncols), src/Frame.cpp:16-51 (the grid ORB/FAST extractor;
 * dead in the reference: its call at src/vslam.cpp:63 is commented out).  Per grid cell: black outline
 * drawn INTO d_bgr (:32), ORB(500, 1.2, 8, 31, 0, 2, HARRIS, 31, fastThreshold 20)->detect, replaced by
 * the fastThreshold-5 detector's result when fewer than 500 keypoints were found (:33-36); then
 * ORB::compute on the whole outlined image (:43).  Like the reference it builds no k-d tree and does
 * not touch map_point_ids.  Outputs per frame: d_xy [frames][kp_stride][2] (ORB::compute's order:
 * grouped by pyramid level), d_desc [frames][kp_stride][32], optional d_angle_octave
 * [frames][kp_stride][2] (degrees, level), d_n [frames].
 * Alignment: d_bgr any address; d_pattern any address (a table off a 16-byte boundary is copied to an aligned one first);
 * d_desc 16 bytes, d_xy 8, d_angle_octave and d_n 4.                                                   */
int vslam_extract_features_grid(vslam_ctx *ctx, uint8_t *d_bgr, int frames, int width, int height,
                                int row_stride, int nrows, int ncols, const int8_t *d_pattern,
                                int kp_stride, float *d_xy, uint8_t *d_desc, float *d_angle_octave,
                                int32_t *d_n);

/* stage-level entry points (parity tests; each is one step of vslam_extract_features).  Alignment: every image plane
 * (d_bgr, d_gray, d_out, d_blurred) and d_pattern at any address -- a plane whose base and width allow it gets the dword or
 * 16-byte kernel, any other the byte kernel, with the same bits; d_desc 16 bytes, d_xy / d_xy_in / d_xy_out 8, d_eig and the
 * counts 4 (d_eig on a 16-byte boundary gets float4 stores).                                           */
int vslam_bgr2gray(vslam_ctx *ctx, const uint8_t *d_bgr, int frames, int width, int height,
                   int row_stride, uint8_t *d_gray);
int vslam_min_eigen(vslam_ctx *ctx, const uint8_t *d_gray, int frames, int width, int height,
                    float *d_eig);
int vslam_good_features(vslam_ctx *ctx, const uint8_t *d_gray, int frames, int width, int height,
                        int max_corners, double quality, double min_distance, int kp_stride,
                        float *d_xy, int32_t *d_n);
int vslam_gaussian7(vslam_ctx *ctx, const uint8_t *d_gray, int frames, int width, int height,
                    uint8_t *d_out);
int vslam_orb_describe(vslam_ctx *ctx, const uint8_t *d_blurred, int frames, int width, int height,
                       const float *d_xy_in, const int32_t *d_n_in, int kp_stride, float cos_a,
                       float sin_a, const int8_t *d_pattern, float *d_xy_out, uint8_t *d_desc,
                       int32_t *d_n_out);

/* ------------------------------------------------------- pose (SURVEY.md 8f "next" rows) */
/* Replaces extract_Rt(fundamental, K, rotation, translation), src/helpers.cpp:3-35, for a batch of
 * fundamental matrices, plus the camera matrix c2 = K * [R | t] of src/vslam.cpp:83-85,125.
 * d_F [batch][9]; d_best [batch][4] as written by vslam_ransac_* (items with winner < 0 are skipped;
 * may be NULL); h_K: HOST 3x3 intrinsics (row-major).  d_R [batch][9], d_t [batch][3], d_c2 [batch][12].
 * Alignment of the pose entry points (this one, vslam_triangulate, _triangulate_points, _reprojection_filter): d_points4d 16
 * bytes, d_xy1, d_xy2, d_p1, d_p2, d_matches, d_error 8, every other device array 4.               */
int vslam_extract_Rt(vslam_ctx *ctx, const float *d_F, const int32_t *d_best, int batch, const float *h_K,
                     float *d_R, float *d_t, float *d_c2);
/* Replaces triangulate(p1, p2, c1, c2, points_4d), src/helpers.cpp:37-80, with c1 = [K | 0]
 * (src/vslam.cpp:123-124): one 4x4 SVD per inlier match (d_matches / d_best[.][3] from RANSAC).
 * d_points4d [batch][kp_stride][4] (x, y, z, 1).                                                    */
int vslam_triangulate(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const int32_t *d_matches,
                      const int32_t *d_best, int batch, int kp_stride, const float *h_K,
                      const float *d_c2, float *d_points4d);

/* triangulate(p1, p2, c1, c2, points_4d) exactly as the reference declares it (include/helpers.h:19, src/helpers.cpp:37-80):
 * n point pairs (d_p1, d_p2: [n][2] f32 on the device), any two 3 x 4 camera matrices (HOST, row-major) -> d_points4d [n][4]
 * (x, y, z, 1).  What the C++ drop-in triangulate() of include/vslam/helpers.h calls.                                       */
int vslam_triangulate_points(vslam_ctx *ctx, const float *d_p1, const float *d_p2, int n, const float *h_c1,
                             const float *h_c2, float *d_points4d);

/* Replaces the reprojection-error filter of src/vslam.cpp:192-251, reproducing the reference exactly,
 * including its two indexing quirks (the de-homogenise loop strides the flat N x 3 array by 3 up to N, and
 * map_point_ids is tested at the MATCH index).  d_points4d from vslam_triangulate; d_map_point_ids
 * [batch][kp_stride] of the current frame; threshold_sq = 4 in the reference (src/vslam.cpp:50).
 * d_inlier_idx [batch][kp_stride] kept match indices (ascending), d_n_inliers [batch], d_error [batch] f64. */
int vslam_reprojection_filter(vslam_ctx *ctx, const float *d_points4d, const float *d_xy1, const float *d_xy2,
                              const int32_t *d_matches, const int32_t *d_best, int batch, int kp_stride,
                              const float *h_K, const float *d_c2, const int32_t *d_map_point_ids,
                              float threshold_sq, int32_t *d_inlier_idx, int32_t *d_n_inliers,
                              double *d_error);

/* Replaces the map-association loop of src/vslam.cpp:129-161 and orb_distance (src/PointMap.cpp:36-46):
 * project each map point with c2, radius_search (r = 2 in the reference) in the frame's k-d tree, and
 * give it the first hit that is unassigned and within `dist_threshold` (64) Hamming of the map point's
 * observations.  Sequential semantics preserved: lower map indices claim first.
 * d_map_points [batch][map_stride][4] (x,y,z,1), d_n_map [batch]; d_c2 [batch][12];
 * d_nodes/d_xy/d_desc/d_n: the frame's features as written by vslam_extract_features;
 * observations in CSR form: d_obs_offsets [batch][map_stride+1], d_obs_desc [batch][obs_stride][32];
 * d_map_point_ids [batch][kp_stride] in/out (-1 = free); d_claim [batch][map_stride] = keypoint or -1.
 * At most 16 acceptable hits per map point are kept; more sets a sticky flag that
 * vslam_ctx_synchronize reports as VSLAM_ERR_CAPACITY.
 * Alignment: d_map_points, d_desc, d_obs_desc 16 bytes, d_xy 8, every other array 4.                */
int vslam_associate_map_points(vslam_ctx *ctx, const float *d_map_points, const int32_t *d_n_map, int batch,
                               int map_stride, const float *d_c2, int img_w, int img_h,
                               const int32_t *d_nodes, const float *d_xy, const uint8_t *d_desc,
                               const int32_t *d_n, int kp_stride, const int32_t *d_obs_offsets,
                               const uint8_t *d_obs_desc, int obs_stride, float radius,
                               uint32_t dist_threshold, int32_t *d_map_point_ids, int32_t *d_claim);

/* ------------------------------------------------------------ the map, resident (PointMap + the loop between pairs)
 * What src/vslam.cpp:60-270 carries from frame to frame, for `tracks` independent sequences advanced in lockstep (one frame
 * step = one batch of `tracks` pairs), entirely in device memory with capacities fixed at creation (the reference's doubling
 * `capacity` is not observable and is not copied):
 *   pm.points / pm.size / pm.colors                 d_points [tracks][map_capacity][4] (x, y, z, 1), d_sizes [tracks],
 *                                                   d_colors [tracks][map_capacity][3] u8
 *   pm.frame_ids[i] / pm.frame_point_ids[i]         an observation log; vslam_map_observations writes it out as CSR lists in
 *                                                   the reference's push order
 *   frame.map_point_ids of every frame              d_map_point_ids [tracks][max_frames][kp_stride], -1 = none (src/Frame.cpp:73)
 *   frame.R_t, frame.pose                           d_R_t, d_pose [tracks][max_frames][16], frame 0 = identity
 * A map belongs to the context it was made on and is destroyed BEFORE it (vslam_map_destroy waits for the context's stream);
 * every call is stream-ordered on that context.  vslam_map_reset / _step / _view / _observations allocate nothing;
 * vslam_track_sequences takes its flattened seed row and the front-end's workspaces from the context's grow-only arena, like
 * vslam_frontend_sequence.  Descriptor arrays handed to a map call are 16-byte aligned, matches and points 8-byte aligned,
 * other int32 / float arrays 4-byte aligned (VSLAM_ERR_INVALID otherwise, before anything is queued); images (d_bgr, d_bgr_cur) at any address; match indices outside the frames' keypoint counts are ignored.  Frame ids count from 0 per track; `frames` = frames recorded so far (1 after create / reset: frame 0). */
typedef struct vslam_map vslam_map;
typedef struct vslam_map_arrays {
    int32_t tracks, max_frames, kp_stride, map_capacity, obs_capacity;
    int32_t frames;                  /* frames recorded so far, frame 0 included (host-side counter)                 */
    float *d_points;                 /* [tracks][map_capacity][4]                                                     */
    uint8_t *d_colors;               /* [tracks][map_capacity][3]                                                     */
    int32_t *d_sizes;                /* [tracks]                                                                      */
    int32_t *d_map_point_ids;        /* [tracks][max_frames][kp_stride]                                               */
    float *d_R_t;                    /* [tracks][max_frames][16]                                                      */
    float *d_pose;                   /* [tracks][max_frames][16]                                                      */
    int32_t *d_obs_counts;           /* [tracks][map_capacity] observations per map point                             */
    int32_t *d_n_obs;                /* [tracks] observations in all                                                  */
} vslam_map_arrays;
int vslam_map_create(vslam_ctx *ctx, int tracks, int max_frames, int kp_stride, int map_capacity, int obs_capacity,
                     vslam_map **out);
int vslam_map_destroy(vslam_map *map);
/* Back to empty (frame 0 recorded, identity poses, no ids, no points); no reallocation. */
int vslam_map_reset(vslam_ctx *ctx, vslam_map *map);
/* One iteration of src/vslam.cpp:60-270 for every track, nothing leaving the device.  Inputs, all [tracks][...] batches:
 * the features of the last and the current frame as vslam_extract_features writes them, the pair's d_matches / d_best / d_F as
 * vslam_match_features writes them, the current frames' images d_bgr_cur [tracks][height][row_stride]; h_K HOST 3 x 3;
 * radius 2, dist_threshold 64, reproj_threshold_sq 4 in the reference.  In stream order:
 *   1. extract_Rt, c2 = K [R | t], R_t, pose = last.pose * R_t (:83-88; the 4 x 4 product in exact double products summed
 *      left to right, one rounding);
 *   2. propagation (:105-118): match (first, second) with id = last.map_point_ids[first] > 0 -- map point 0 is never
 *      propagated, as in the reference -- sets cur.map_point_ids[second] = id (of two matches onto one `second` the later
 *      wins) and pushes the observation (frame, second) onto map point id (both do);
 *   3. association (:126-161) = vslam_associate_map_points over the map as it stands before this frame's new points, its
 *      observations including those of step 2; every claim pushes an observation;
 *   4. vslam_triangulate (c1 = [K | 0]) and vslam_reprojection_filter against the UPDATED map_point_ids;
 *   5. add_reprojection_inliers (src/PointMap.cpp:3-34): the kept matches, ascending, become map points size .. size + k - 1
 *      with w = 1, the observations (last frame, first), (frame, second) in that order and the colour
 *      image.at(int(x2), int(y2)): ROW int(x), COLUMN int(y), as the reference writes it (:247).  Where that row is >= height
 *      (or the column >= width) the reference reads outside the image or the row; (0, 0, 0) is written here.  map_point_ids are
 *      not set for new points (the reference does not).
 * A pair without a RANSAC winner (d_best[.][0] < 0, the items vslam_extract_Rt skips) leaves its track's map untouched for the
 * step: R_t = identity, pose carried over, no ids (the reference would go on with an empty F: undefined).  A track for which
 * map_capacity or obs_capacity does not suffice anywhere in the step is left the same way -- nothing partial -- and a step
 * beyond max_frames does nothing at all; both raise the context's sticky error word (VSLAM_ERR_CAPACITY from
 * vslam_ctx_synchronize / the pipeline ticket), as does the 16-candidate cap of the association.                            */
int vslam_map_step(vslam_ctx *ctx, vslam_map *map, const float *d_xy_last, const uint8_t *d_desc_last, const int32_t *d_n_last,
                   const float *d_xy_cur, const uint8_t *d_desc_cur, const int32_t *d_nodes_cur, const int32_t *d_n_cur,
                   const int32_t *d_matches, const int32_t *d_best, const float *d_F, const uint8_t *d_bgr_cur, int width,
                   int height, int row_stride, const float *h_K, float radius, uint32_t dist_threshold,
                   float reproj_threshold_sq);
/* Device pointers of the state (valid until vslam_map_destroy; contents as of the work queued so far). */
int vslam_map_view(vslam_map *map, vslam_map_arrays *out);
/* pm.frame_ids / pm.frame_point_ids as CSR, stream-ordered: d_offsets [tracks][map_capacity + 1] (entries past a track's size
 * repeat its total), d_frame_ids / d_point_ids [tracks][obs_capacity]: map point i of track b observed by
 * (d_frame_ids[b][o], d_point_ids[b][o]) for o in [d_offsets[b][i], d_offsets[b][i + 1]), in the reference's push order.
 * Slots past a track's total are not written.                                                                            */
int vslam_map_observations(vslam_ctx *ctx, vslam_map *map, int32_t *d_offsets, int32_t *d_frame_ids, int32_t *d_point_ids);
/* The loop for resident video: d_bgr [tracks][frames][height][row_stride]; d_seeds [tracks][frames - 1].  Resets the map,
 * extracts all tracks * frames frames once and matches every consecutive pair as one batch -- vslam_frontend_sequence over the
 * flattened frames (index track * frames + f), so that no existing translation unit changes; the tracks - 1 pairs that
 * straddle two tracks are computed and ignored (1 / frames of the matching time) -- then frames - 1 map steps.  Per-frame
 * outputs [tracks * frames] slots and per-pair outputs [tracks * frames - 1] slots are the caller's, as in
 * vslam_frontend_sequence with frames = tracks * frames: pair (track, f -> f + 1) is slot track * frames + f, so the records
 * path keeps working.  kp_stride is the map's (<= VSLAM_KDTREE_MAX_KP: the trees are needed).  Steps beyond max_frames do nothing and raise the
 * error word, like vslam_map_step.                                                                                        */
int vslam_track_sequences(vslam_ctx *ctx, vslam_map *map, const uint8_t *d_bgr, int frames, int width, int height,
                          int row_stride, const vslam_extract_params *params, const uint32_t *d_seeds, int hyp, float threshold,
                          const float *h_K, float radius, uint32_t dist_threshold, float reproj_threshold_sq, float *d_xy,
                          uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n, int32_t *d_matches, int32_t *d_best, float *d_F);

/* ------------------------------------------------------------ the view of the map (Display, headless)
 * What the reference shows in its Pangolin window (include/Display.h, src/display.cpp; fed from src/vslam.cpp:264-276), as
 * images in device memory: one image per track, from any viewpoint, the map points as squares of their stored colour and one
 * wire frustum per recorded frame (draw_box, src/display.cpp:118-152).  THIS TEXT and tests/ref_render.py are the contract;
 * OpenGL is not (no claim is made that Pangolin lights the same pixels).
 *
 * Eye space: x right, y down, z forward -- the convention of the project's cameras (c1 = [K | 0]).
 * Arithmetic: every f32 input (coordinates, poses, the view) is widened to f64; products and sums run left to right in f64,
 * never fused; division, floor and ceil are IEEE; one rounding to f32 where a depth becomes a key.  xf(M, p) below is
 *     r_i = ((M[i][0] * p.x + M[i][1] * p.y) + M[i][2] * p.z) + M[i][3]        i = 0, 1, 2   (rows 0..2 of a row-major 4 x 4)
 * and mix(a, b, t) = a * (1 - t) + b * t  (so that t = 0 gives a and t = 1 gives b exactly).
 *
 * Primitives of a track, in order; the ORDER INDEX breaks depth ties (the lower index wins):
 *   1. its map points 0 .. n - 1, n = d_sizes[track] clamped to 0 .. map_stride  (AS_REFERENCE: n = ceil(size / 4), below);
 *   2. with VSLAM_RENDER_FRUSTA, for frames 0 .. frames - 1 the eight segments of draw_box in the order of
 *      src/display.cpp:129-148: order index n + 8 * frame + s.  With O = (0, 0, 0), w = box_w, h = w * box_h_ratio,
 *      z = w * box_z_ratio (both products in f32, as draw_box forms them):
 *        s = 0..3  O -> (w, h, z), O -> (w, -h, z), O -> (-w, -h, z), O -> (-w, h, z)
 *        s = 4..7  (w, h, z) -> (w, -h, z), (-w, h, z) -> (-w, -h, z), (-w, h, z) -> (w, h, z), (-w, -h, z) -> (w, -h, z)
 * A map point: e = xf(mv, (x, y, z)) -- the stored w is ignored, as glVertex3d ignores it.  Drawn iff the three of e are
 *   finite and z_near <= e.z <= z_far.  px = floor(fu * e.x / e.z + u0), py = floor(fv * e.y / e.z + v0) (the product first,
 *   then the quotient, then the sum); a point with |px| or |py| above 2^30 is not drawn.  It covers the pixels
 *   px - (s - 1) / 2 .. px + s / 2 by py - (s - 1) / 2 .. py + s / 2 (s = point_size, integer division), clipped to the image,
 *   each with depth (float) e.z.
 * A frustum segment A -> B (camera coordinates): a = xf(mv, xf(pose, A)), b likewise, nothing rounded in between
 *   (glMultTransposeMatrixf(pose) of a row-major pose is pose * p).  Dropped if a coordinate is not finite.
 *   (i)   z clip: dropped if both a.z, b.z < z_near or both > z_far.  An endpoint p with p.z < z_near is replaced by
 *         (mix(a.x, b.x, t), mix(a.y, b.y, t), z_near) with t = (z_near - a.z) / (b.z - a.z); with p.z > z_far likewise with
 *         z_far.  Both replacements are computed from the ORIGINAL a and b.
 *   (ii)  projection of both ends: U = fu * x / z + u0, V = fv * y / z + v0, iz = 1 / z; dropped if one is not finite.
 *   (iii) Liang-Barsky against the rectangle [-0.5, width + 0.5] x [-0.5, height + 0.5] (half pixels: a run cut at two
 *         opposite borders then steps from pixel centre to pixel centre, where floor is safe from the last bit of a sum),
 *         s0 = 0, s1 = 1, dU = Ub - Ua, dV = Vb - Va,
 *         for (p, q) in (-dU, Ua + 0.5), (dU, (width + 0.5) - Ua), (-dV, Va + 0.5), (dV, (height + 0.5) - Va):
 *             p == 0: dropped if q < 0;   p < 0: r = q / p, dropped if r > s1, s0 = max(s0, r);
 *             p > 0: r = q / p, dropped if r < s0, s1 = min(s1, r);
 *         the ends become mix(., ., s0) and mix(., ., s1) of U, V and iz (from the unclipped ends).  An end inside the image is
 *         therefore never moved, and the work per segment is O(width + height) whatever the pose.
 *   (iv)  m = max(|Ub - Ua|, |Vb - Va|) of the clipped ends; dropped unless m <= 65536; n = max(1, ceil(m)); the samples
 *         k = 0 .. n at t = k / n: pixel (floor(mix(Ua, Ub, t)), floor(mix(Va, Vb, t))), kept if inside the image, with depth
 *         (float)(1 / mix(iza, izb, t)): 1 / z is linear on the screen, so the depth is perspective-correct.
 * Winner per pixel: the smallest 64-bit key (bits of the f32 depth) << 32 | order index (positive floats order as their bit
 * patterns; an integer minimum does not depend on arrival order, so the image is bitwise reproducible).  The pixel gets the
 * winner's colour -- a point's stored (b, g, r) as is, frustum_bgr for a segment -- or background_bgr without a winner.
 * VSLAM_RENDER_AS_REFERENCE reproduces what draw_points_colors actually submits (src/display.cpp:97-116): its loop runs
 *   `i < size; i += 4` over a FLAT float index, so only points 0 .. ceil(size / 4) - 1 are drawn, and the colour goes through
 *   glColor3b(colors.x, colors.y, colors.z): the stored B, G, R taken as SIGNED bytes and as red, green, blue.
 *   [OpenGL, from memory] unpinned: a signed byte c maps to (2c + 1) / 255, negative values clamp to 0, so a stored channel c
 *   becomes 2c + 1 for c < 128 and 0 otherwise; output R comes from stored B, output G from stored G, output B from stored R.
 *
 * d_points [tracks][map_stride][4] f32, d_colors [tracks][map_stride][3] u8, d_sizes [tracks] int32; d_pose
 * [tracks][pose_stride][16] f32 (row-major 4 x 4; may be NULL when frames == 0 or VSLAM_RENDER_FRUSTA is not set),
 * 0 <= frames <= pose_stride; d_points is 16-byte, d_sizes, d_pose and d_depth_out are 4-byte aligned (VSLAM_ERR_INVALID otherwise), d_colors and d_bgr_out may sit at any address.  d_bgr_out [tracks][height][row_stride] u8, row_stride >= 3 * width; bytes past 3 * width in a
 * row are not written.  d_depth_out (may be NULL) [tracks][height][width] f32: the winner's depth, +inf where nothing was drawn.
 * Both calls are stream-ordered on the context, take their key plane ([tracks][height][width] u64) from the context's grow-only
 * arena, do not synchronise (except when that plane has to grow: the arena then waits for the stream before it frees the old
 * block, as for every workspace) and do not write to the map.  VSLAM_ERR_INVALID, before anything is queued, for: a null pointer,
 * a non-positive size (tracks, map_stride, width, height; frames < 0; pose_stride < frames), row_stride < 3 * width,
 * point_size outside 1..15, z_near <= 0 (or not finite), z_far < z_near, a track range outside the map.  VSLAM_ERR_CAPACITY for
 * width or height above 16384, more than 65535 tracks or more than 2^20 frames.                                                                                      */
#define VSLAM_RENDER_FRUSTA 1
#define VSLAM_RENDER_AS_REFERENCE 2
typedef struct vslam_view {
    float mv[16];              /* world -> eye, row-major 4 x 4, rows 0..2 used (affine)            */
    float fu, fv, u0, v0;      /* pinhole of the viewer                                              */
    float z_near, z_far;       /* a primitive sample is drawn iff z_near <= eye z <= z_far           */
    int32_t point_size;        /* side of the square a map point covers, 1..15                       */
    int32_t flags;             /* VSLAM_RENDER_FRUSTA | VSLAM_RENDER_AS_REFERENCE                     */
    float box_w, box_h_ratio, box_z_ratio;   /* draw_box: 1.0, 0.75, 0.6 (include/Display.h:34)      */
    uint8_t background_bgr[3], frustum_bgr[3];   /* (0,0,0) and blue = (255,0,0), src/display.cpp:52 */
} vslam_view;
/* Host only, no context.  The numbers of src/display.cpp:25-26: look_at from eye (-2, 2, -2) to (0, 0, 0) with up (0, 1, 0),
 * focal 420 / 420, centre (width / 2, height / 2) in integer division, near 0.2, far 10000; point size 1, VSLAM_RENDER_FRUSTA,
 * the draw_box defaults, black background, blue frusta.                                                                    */
int vslam_view_default(int width, int height, vslam_view *out);
/* In double on the host: f = normalize(target - eye), r = normalize(cross(f, up)), d = cross(f, r); the rows of the rotation
 * R are r, d, f, the translation is -(R * eye); rounded once to f32; row 3 = (0, 0, 0, 1).  normalize(v) = v / sqrt((v.x * v.x
 * + v.y * v.y) + v.z * v.z), cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x), a row of
 * R * eye = (R0 * eye.x + R1 * eye.y) + R2 * eye.z.  VSLAM_ERR_DEGENERATE when eye == target or up is parallel to the
 * viewing direction (mv_out is then untouched).                                                                            */
int vslam_view_look_at(const double eye[3], const double target[3], const double up[3], float mv_out[16]);
int vslam_render_points(vslam_ctx *ctx, const float *d_points, const uint8_t *d_colors, const int32_t *d_sizes,
                        int tracks, int map_stride, const float *d_pose, int frames, int pose_stride,
                        const vslam_view *h_view, int width, int height, int row_stride,
                        uint8_t *d_bgr_out, float *d_depth_out /* may be NULL */);
/* vslam_render_points over the map's own arrays (vslam_map_view) for tracks track_lo .. track_lo + track_count - 1 and the
 * frames recorded so far; the output arrays have track_count slots.                                                       */
int vslam_map_render(vslam_ctx *ctx, vslam_map *map, int track_lo, int track_count, const vslam_view *h_view,
                     int width, int height, int row_stride, uint8_t *d_bgr_out, float *d_depth_out);

/* ------------------------------------------------------------ the world frame (a second, opt-in view beside the map)
 * The map above is the reference's, bit for bit: every pair's t has length 1 (extract_Rt), so every pair's points have a unit of
 * their own; they are in the LAST frame's camera coordinates (c1 = [K | 0]); and `pose` chains last -> current transforms.  A
 * vslam_world puts the same tracks into ONE coordinate system per track -- that of the track's frame 0, in the unit of its first
 * pair with a model -- without touching what the map holds.  THIS TEXT and tests/ref_world.py are the contract.
 *
 * Per track and step (f - 1 -> f), from the step's R [9], t [3] (f32, as vslam_extract_Rt / vslam_refine_pairs leave them), the
 * compacted inlier matches m = 0 .. n - 1, n = d_best[.][3] clamped to 0 .. kp_stride, and their triangulated points X_m
 * (d_points4d slot m; the fourth entry is not read).  ALL arithmetic is f64, never fused, sums left to right; f32 inputs are
 * widened first.  |v|^2 = (x x + y y) + z z.
 *   carry   [kp_stride] per track: an f64 3-vector and a validity per keypoint of the LAST frame: that keypoint's point in the
 *           last frame's camera coordinates, in world units, as the previous step left it.
 *   in range: 0 <= first < min(d_n_last, kp_stride) and 0 <= second < min(d_n_cur, kp_stride); any other match is ignored.
 *   usable: Y_m = R X_m + t, row r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r; X_m and Y_m finite, X_m.z > 0 and Y_m.z > 0.
 *   link:   in range, usable, carry[first] valid, and q = |carry[first]|^2 / |X_m|^2 finite (it is unless a square overflows
 *           or |X_m|^2 underflows to 0; such a match still carries on, it does not vote).
 *   scale:  with L links and L >= min_links, s_f = sqrt(q_(k)), the element of rank k = (L - 1) / 2 (integer division) among the
 *           q in ascending order -- a value, so arrival order cannot show.  Otherwise s_f = s_(f-1); s_0 = 1.  d_links[.][f] = L.
 *   pose:   camera -> world.  Twc_0 = I;  Twc_f = Twc_(f-1) * [R^t | -(s_f (R^t t))] with (R^t t)_i = ((R_0i t_0 + R_1i t_1) +
 *           R_2i t_2); the 4 x 4 product is P_rc = ((A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c) + A_r3 B_3c, all four terms, row 3
 *           included.  NOTHING IS RE-ORTHONORMALISED: the rotation block is a product of f32-rounded rotations and drifts from
 *           orthogonality by about 2^-24 per frame.
 *   lift:   a point X of this pair becomes xf(Twc_(f-1), (s_f x, s_f y, s_f z)) rounded once to f32, w = 1 (xf as for the
 *           renderer above).
 *   new carry: keyed by `second`: s_f Y_m for every in-range usable match; of two matches onto one `second` the HIGHER match
 *           index wins; every other entry is invalid.
 *   a pair without a winner (d_best[.][0] < 0): Twc_f = Twc_(f-1), s_f = s_(f-1), d_links = -1, the carry all invalid.
 * The f64 square root is the device library's, which is correctly rounded on gfx950 (tests/test_gpu_world.py holds it to the
 * host's on thousands of values), so every output is held bit for bit.  The selection is a radix select over the u64 bit patterns
 * (non-negative doubles order as their bits) with integer histograms in LDS: no sort, no floating-point atomics, the same bits in
 * every batch slot and run.
 *
 * A world belongs to the context it was made on and is destroyed before it; capacities are fixed at creation and
 * vslam_world_reset / _step / _lift / _view / _render allocate nothing (vslam_map_attach_world allocates d_world_points, once).
 * Every call is stream-ordered on the context and does not synchronise.  kp_stride <= VSLAM_MAX_KP (VSLAM_ERR_CAPACITY),
 * min_links >= 1 (8 is the default of the Python and C++ surfaces).                                                          */
typedef struct vslam_world vslam_world;
typedef struct vslam_world_arrays {
    int32_t tracks, max_frames, kp_stride, min_links;
    int32_t map_capacity;            /* 0 until attached to a map                                                     */
    int32_t frames;                  /* frames recorded so far, frame 0 included (host-side counter)                  */
    double *d_Twc;                   /* [tracks][max_frames][16] camera -> world, row-major 4 x 4                     */
    float *d_pose;                   /* [tracks][max_frames][16] the same rounded once: what vslam_render_points takes */
    double *d_scale;                 /* [tracks][max_frames]                                                           */
    int32_t *d_links;                /* [tracks][max_frames] L; -1: no winner; 0 for frame 0                           */
    double *d_carry;                 /* [tracks][kp_stride][3]                                                         */
    int32_t *d_carry_index;          /* [tracks][kp_stride] the match that wrote the entry, -1 = invalid               */
    float *d_world_points;           /* [tracks][map_capacity][4], NULL until attached                                 */
} vslam_world_arrays;
int vslam_world_create(vslam_ctx *ctx, int tracks, int max_frames, int kp_stride, int min_links, vslam_world **out);
/* Waits for the context's stream.  A world that is attached to a map is destroyed after that map, or detached first. */
int vslam_world_destroy(vslam_world *world);
/* Back to frame 0: identity poses, scale 1, links 0, no carry, d_world_points zero. */
int vslam_world_reset(vslam_ctx *ctx, vslam_world *world);
/* Advances every track by one frame ([tracks][...] batches: d_matches [.][kp_stride][2], d_best [.][4], d_points4d
 * [.][kp_stride][4], d_R [.][9], d_t [.][3], d_n_last / d_n_cur [.]).  d_matches is 8-byte and d_points4d 16-byte aligned.
 * A step beyond max_frames does nothing and raises the context's sticky error word, as vslam_map_step does.              */
int vslam_world_step(vslam_ctx *ctx, vslam_world *world, const int32_t *d_matches, const int32_t *d_best,
                     const float *d_points4d, const float *d_R, const float *d_t, const int32_t *d_n_last,
                     const int32_t *d_n_cur);
/* Lifts rows [d_lo[track], d_hi[track]) (clamped to 0 .. stride) of d_points [tracks][stride][4], points of pair
 * (frame - 1 -> frame), 1 <= frame < frames recorded, into d_out [tracks][stride][4]; rows outside the range keep their bits.
 * d_out may be d_points.  Both are 16-byte aligned, d_lo and d_hi 4-byte (VSLAM_ERR_INVALID otherwise).                      */
int vslam_world_lift(vslam_ctx *ctx, vslam_world *world, int frame, const float *d_points, int stride, const int32_t *d_lo,
                     const int32_t *d_hi, float *d_out);
int vslam_world_view(vslam_world *world, vslam_world_arrays *out);
/* From now on vslam_map_step and vslam_track_sequences run the world step behind each map step, on the step's own R, t and
 * points4d (the adjusted ones under VSLAM_OPT_POSE_REFINE), and lift the points appended in that step -- rows [size before, size
 * after) of d_points -- into d_world_points.  A track the map leaves untouched for a step (capacity, or no winner) appends
 * nothing; its world still advances as specified.  vslam_map_reset resets the world too.  tracks, max_frames, kp_stride and the
 * frames recorded so far must agree and both must belong to one context (VSLAM_ERR_INVALID otherwise).  world = NULL detaches.
 * Without an attached world no launch is added to a map step and every output of the map keeps its bits; with one, the map's own
 * arrays keep their bits as well.                                                                                           */
int vslam_map_attach_world(vslam_map *map, vslam_world *world);
/* vslam_render_points over d_world_points, the map's colours and sizes and the world's f32 poses, for the frames recorded so
 * far; `map` is the map the world is attached to.  Arguments as for vslam_map_render.                                      */
int vslam_world_render(vslam_ctx *ctx, vslam_world *world, vslam_map *map, int track_lo, int track_count,
                       const vslam_view *h_view, int width, int height, int row_stride, uint8_t *d_bgr_out,
                       float *d_depth_out);

/* ------------------------------------------------------------------ pipeline */
/* match_features(frame1, frame2, rf, matches, F), src/Frame.cpp:82-105, for a batch of pairs
 * whose features are already on the device: match -> sets -> RANSAC -> inlier matches.
 * Workspaces are owned by the context and sized on first use.
 * Alignment: d_desc1, d_desc2 16 bytes, d_xy1, d_xy2, d_matches 8, every other array 4, tested up front. */
int vslam_match_features(vslam_ctx *ctx, const float *d_xy1, const uint8_t *d_desc1,
                         const int32_t *d_n1, const float *d_xy2, const uint8_t *d_desc2,
                         const int32_t *d_n2, int batch, int kp_stride, const uint32_t *d_seeds,
                         int hyp, float threshold, int32_t *d_matches, int32_t *d_best, float *d_F,
                         int32_t *d_prelim_m);

/* The whole front-end for a batch of independent frame pairs: frames [0, pairs) are the "last"
 * frames, frames [pairs, 2*pairs) the "current" ones; pair p = (frame p, frame pairs + p).
 * Extract all 2*pairs frames, match last->current, RANSAC.  This is what bench.py times.
 * d_xy / d_desc / d_nodes / d_n are the per-frame outputs of vslam_extract_features for all
 * 2*pairs frames; d_matches / d_best / d_F are per pair as in vslam_match_features.
 * Alignment as for vslam_extract_features and vslam_match_features, all of it tested before the first stage is queued
 * (the same holds for vslam_frontend_pairs_pose, with pose->d_points4d 16 bytes and pose->d_error 8, and for
 * vslam_frontend_sequence).                                                                   */
int vslam_frontend_pairs(vslam_ctx *ctx, const uint8_t *d_bgr, int pairs, int width, int height,
                         int row_stride, const vslam_extract_params *params, int kp_stride,
                         const uint32_t *d_seeds, int hyp, float threshold,
                         float *d_xy, uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n,
                         int32_t *d_matches, int32_t *d_best, float *d_F);

/* The capture loop's whole per-pair chain in one call, nothing leaving the device in between (src/vslam.cpp:60-88: extract,
 * match_features, extract_Rt, R_t; :120-125 the camera matrices; :186 triangulate; :192-251 the reprojection filter):
 * vslam_frontend_pairs, then vslam_extract_Rt, vslam_triangulate (c1 = [K | 0]) and vslam_reprojection_filter on its matches.
 * h_K: HOST 3 x 3 intrinsics.  d_map_point_ids [pairs][kp_stride] of the current frames, or NULL for "none assigned" (-1
 * everywhere).  Outputs as the four entry points write them; every pointer of `pose` is required.  Usable on a context of a
 * vslam_pipeline like every other entry point.                                                                              */
typedef struct vslam_pose_outputs {
    float *d_R;             /* [pairs][9]  */
    float *d_t;             /* [pairs][3]  */
    float *d_c2;            /* [pairs][12] */
    float *d_points4d;      /* [pairs][kp_stride][4] */
    int32_t *d_inlier_idx;  /* [pairs][kp_stride] match indices that pass the reprojection filter, ascending */
    int32_t *d_n_inliers;   /* [pairs] */
    double *d_error;        /* [pairs] summed reprojection error of the kept matches */
} vslam_pose_outputs;
int vslam_frontend_pairs_pose(vslam_ctx *ctx, const uint8_t *d_bgr, int pairs, int width, int height, int row_stride,
                              const vslam_extract_params *params, int kp_stride, const uint32_t *d_seeds, int hyp,
                              float threshold, float *d_xy, uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n,
                              int32_t *d_matches, int32_t *d_best, float *d_F, const float *h_K,
                              const int32_t *d_map_point_ids, float reproj_threshold_sq, const vslam_pose_outputs *pose);

/* Fixed-size per-pair result records for the one exchange of the multi-GPU path: per pair
 * 13 + kp_stride int32 words = F (9 words, bit-preserving), d_best's 4 words, then one word per match slot,
 * query index | train index << 16 (keypoint indices are below VSLAM_MAX_KP).  d_records: [pairs][13 + kp_stride].
 * Alignment: d_matches 8 bytes, the others 4.                                                                     */
int vslam_pack_records(vslam_ctx *ctx, const float *d_F, const int32_t *d_best, const int32_t *d_matches,
                       int pairs, int kp_stride, int32_t *d_records);

/* The same path for a run of consecutive video frames, the shape of the reference's main loop
 * (src/vslam.cpp:60-77: every new frame is matched against the previous one): extract each of the `frames`
 * frames ONCE, then pair i = (frame i, frame i + 1) for i in [0, frames - 1).
 * Per-frame outputs as in vslam_extract_features ([frames] slots); d_seeds, d_matches, d_best, d_F have
 * frames - 1 slots.  frames >= 2.                                                              */
int vslam_frontend_sequence(vslam_ctx *ctx, const uint8_t *d_bgr, int frames, int width, int height,
                            int row_stride, const vslam_extract_params *params, int kp_stride,
                            const uint32_t *d_seeds, int hyp, float threshold, float *d_xy,
                            uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n, int32_t *d_matches,
                            int32_t *d_best, float *d_F);

/* ------------------------------------------------------------ batches in flight on one device
 * The reference's capture loop (src/vslam.cpp:53-77) finishes one frame pair before it looks at the next.  On the device
 * a batch runs through stages that fill the chip and stages of one workgroup per frame or pair that leave most of it
 * idle; the entry points are stream-ordered and a context owns its streams and workspaces, so a caller with a queue of
 * batches keeps k of them in flight on k contexts and the idle parts of one are filled by another (2.90 -> 2.61 ms per
 * batch at the headline shape with k = 4; contexts made here are arranged for company: DESIGN.md 6).  A TICKET is one batch:
 *   vslam_pipeline_acquire   next context, round-robin; waits for the batch that used it k tickets ago (at most k batches
 *                            are ever queued) and files that batch's status.  Enqueue the batch on the context returned --
 *                            any entry points of this header, uploads and vslam_gather_records included;
 *   vslam_pipeline_commit    closes the batch (its status = the context's device-side error word at this point of the
 *                            stream: copied and cleared in stream order, so one batch's overflow is reported for that
 *                            ticket only and does not reach the next batch of the same context);
 *   vslam_pipeline_submit_pairs / _sequence   acquire + vslam_frontend_pairs / _sequence (+ vslam_pack_records when
 *                            d_records is not NULL) + commit.  Output buffers are the caller's, one set per batch in flight.
 *                            An error of the wrapped call is returned at once, *ticket_out = -1, the slot stays usable
 *                            (an argument off its alignment is such an error: nothing of the batch is queued, nothing is
 *                            filed under a ticket; d_records: 4 bytes);
 *   vslam_pipeline_wait      blocks until that batch is complete; returns its status (VSLAM_OK, VSLAM_ERR_CAPACITY, ...).
 *                            Statuses of failed batches nobody asked about are kept (the last 256);
 *   vslam_pipeline_poll      1 = complete, 0 = not yet (never blocks);
 *   vslam_pipeline_drain     waits for everything; the first failure not yet collected by vslam_pipeline_wait, else VSLAM_OK.
 * Inputs of a batch must be ordered before it: resident, or uploaded through the acquired context (vslam_upload_async +
 * vslam_upload_fence).  One submitting thread at a time (calls are serialised by a mutex).  n_ctx: 1 .. 16.           */
typedef struct vslam_pipeline vslam_pipeline;
int vslam_pipeline_create(int device, int n_ctx, vslam_pipeline **out);
int vslam_pipeline_destroy(vslam_pipeline *p);
int vslam_pipeline_size(const vslam_pipeline *p);
vslam_ctx *vslam_pipeline_ctx(vslam_pipeline *p, int slot);   /* ticket t runs on slot t % size */
const char *vslam_pipeline_last_error(vslam_pipeline *p);
int vslam_pipeline_set_option(vslam_pipeline *p, int option, int value);   /* vslam_ctx_set_option on every context */
int vslam_pipeline_acquire(vslam_pipeline *p, vslam_ctx **ctx_out, int64_t *ticket_out);
int vslam_pipeline_commit(vslam_pipeline *p, int64_t ticket);
int vslam_pipeline_submit_pairs(vslam_pipeline *p, const uint8_t *d_bgr, int pairs, int width, int height, int row_stride,
                                const vslam_extract_params *params, int kp_stride, const uint32_t *d_seeds, int hyp,
                                float threshold, float *d_xy, uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n,
                                int32_t *d_matches, int32_t *d_best, float *d_F, int32_t *d_records, int64_t *ticket_out);
/* vslam_frontend_pairs_pose as a ticket (h_K is copied; *pose is copied, the arrays it names are the caller's until the
 * ticket has been waited for).  A batch that exhausts the corner pool is queued once more, pose stages included. */
int vslam_pipeline_submit_pairs_pose(vslam_pipeline *p, const uint8_t *d_bgr, int pairs, int width, int height, int row_stride,
                                     const vslam_extract_params *params, int kp_stride, const uint32_t *d_seeds, int hyp,
                                     float threshold, float *d_xy, uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n,
                                     int32_t *d_matches, int32_t *d_best, float *d_F, const float *h_K,
                                     const int32_t *d_map_point_ids, float reproj_threshold_sq, const vslam_pose_outputs *pose,
                                     int32_t *d_records, int64_t *ticket_out);
int vslam_pipeline_submit_sequence(vslam_pipeline *p, const uint8_t *d_bgr, int frames, int width, int height, int row_stride,
                                   const vslam_extract_params *params, int kp_stride, const uint32_t *d_seeds, int hyp,
                                   float threshold, float *d_xy, uint8_t *d_desc, int32_t *d_nodes, int32_t *d_n,
                                   int32_t *d_matches, int32_t *d_best, float *d_F, int32_t *d_records, int64_t *ticket_out);
int vslam_pipeline_poll(vslam_pipeline *p, int64_t ticket);
int vslam_pipeline_wait(vslam_pipeline *p, int64_t ticket);
int vslam_pipeline_drain(vslam_pipeline *p);
/* Batches that vslam_pipeline_submit_pairs / _sequence queued and the pipeline then queued a SECOND time by itself: a batch in
 * which more frames needed the corner detector's whole-image fallback than its pool holds (VSLAM_OPT_CORNER_LIST_CAP; pure
 * noise, response plateaus) is done again, when its status is collected, with every list sized for the whole image; its
 * outputs are then complete and the ticket reports VSLAM_OK.  (A ticket built with acquire / commit cannot be queued again --
 * the pipeline does not know what was enqueued -- and reports VSLAM_ERR_CAPACITY as before.)                                */
int64_t vslam_pipeline_batches_redone(vslam_pipeline *p);

/* ------------------------------------------------------------ several devices
 * Frame pairs are independent (src/RansacFilter.cpp:38: all state is per call), so a batch shards by contiguous slices,
 * one slice per device, with per-pair seeds base ^ GLOBAL pair index -- a pair's result does not depend on the split --
 * and the only exchange is the final gather of fixed-size result records (vslam_pack_records' layout).
 * vslam_shard_range: the slice [lo, hi) of `items` that `rank` of `world` owns (the first items % world ranks get one more). */
int vslam_shard_range(int items, int rank, int world, int *lo, int *hi);

/* (i) One process that owns the devices: one context + one host thread per entry of `devices` (an entry may repeat: several
 * contexts on one device).  vslam_multi_frontend_pairs = vslam_frontend_pairs + vslam_pack_records on every slice at once.
 *   h_bgr_last / h_bgr_cur: HOST, [pairs][height][row_stride] each (page-locked memory from vslam_host_alloc uploads faster);
 *   params->d_pattern must be NULL; h_pattern: HOST [256][4] int8 or NULL for ORB's learned table;
 *   h_records: HOST [pairs][13 + kp_stride] int32, pair order; h_n_keypoints: HOST [2 * pairs] (last frames, then current)
 *   or NULL.  Blocking: returns when every slice is done.  Options are per context: vslam_multi_ctx(m, i).            */
typedef struct vslam_multi vslam_multi;
int vslam_multi_create(const int *devices, int n_devices, vslam_multi **out);
int vslam_multi_destroy(vslam_multi *m);
int vslam_multi_size(const vslam_multi *m);
vslam_ctx *vslam_multi_ctx(vslam_multi *m, int i);
const char *vslam_multi_last_error(vslam_multi *m);
int vslam_multi_frontend_pairs(vslam_multi *m, const uint8_t *h_bgr_last, const uint8_t *h_bgr_cur, int pairs, int width,
                               int height, int row_stride, const vslam_extract_params *params, const int8_t *h_pattern,
                               int kp_stride, uint32_t base_seed, int hyp, float threshold, int32_t *h_records,
                               int32_t *h_n_keypoints);
/* Host frames reach each device in chunks of 64 pairs, chunk k + 1 uploading while chunk k computes; all the same a slot is
 * bound by its host link (57 GB/s page-locked = about 20 k pairs/s at 1280x720 against 90 k for the kernels).  When the
 * frames are ALREADY on the devices (decoded there, produced by an earlier stage, uploaded ahead of time):
 * d_bgr[r] = slot r's slice on slot r's device in vslam_frontend_pairs' layout -- the slice's `last` frames, then its
 * `current` frames, (hi - lo) of each for [lo, hi) = vslam_shard_range(pairs, r, size) -- NULL allowed for an empty slice.
 * Everything else as above: records and counts come back to host memory in pair order.  The images: any address.           */
int vslam_multi_frontend_pairs_resident(vslam_multi *m, const uint8_t *const *d_bgr, int pairs, int width, int height,
                                        int row_stride, const vslam_extract_params *params, const int8_t *h_pattern,
                                        int kp_stride, uint32_t base_seed, int hyp, float threshold, int32_t *h_records,
                                        int32_t *h_n_keypoints);

/* (ii) One process per device (any launcher): every rank runs its slice on its own context; the records are exchanged once,
 * all-gather over RCCL (xGMI inside a node) on the context's stream.  RCCL is loaded when the first of these is called.
 *   vslam_comm_unique_id: rank 0 makes the 128-byte id and hands it to the other ranks by whatever channel the launcher
 *   has (a file, a socket, an environment variable, MPI); vslam_comm_create: collective over all ranks.
 *   vslam_gather_records: every rank contributes words_per_rank int32 (equal on all ranks: pad the last slice);
 *   d_all receives world x words_per_rank in rank order = pair order.  Asynchronous on the context's stream.
 *   d_records and d_all (here and in vslam_gather_records_v): 4-byte aligned.                                          */
#define VSLAM_COMM_ID_BYTES 128
typedef struct vslam_comm vslam_comm;
int vslam_comm_unique_id(void *id_out);
int vslam_comm_create(vslam_ctx *ctx, const void *id, int world, int rank, vslam_comm **out);
int vslam_comm_destroy(vslam_comm *comm);
int vslam_gather_records(vslam_ctx *ctx, vslam_comm *comm, const int32_t *d_records, size_t words_per_rank,
                         int32_t *d_all);
/* What RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank), not what vslam_comm_create was told.  */
int vslam_comm_info(vslam_comm *comm, int *world_out, int *rank_out);
/* Uneven slices and the rooted form.  Rank r contributes h_words[r] int32 words (HOST array of `world` counts, the same on
 * every rank; 0 allowed); d_all receives them in rank order = pair order.  root < 0: every rank receives everything (an
 * all-gather with counts); root >= 0: only that rank does -- each peer sends its block once, straight to the root, over its
 * own xGMI link (d_all may be NULL on the others).  One group of ncclSend / ncclRecv on the context's stream. */
int vslam_gather_records_v(vslam_ctx *ctx, vslam_comm *comm, const int32_t *d_records, const size_t *h_words, int root,
                           int32_t *d_all);

#ifdef __cplusplus
}
#endif
#endif
