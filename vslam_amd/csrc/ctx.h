// Context, error plumbing, workspace arena and per-kernel event timing shared by the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/vslam_amd.h"
#include "../../include/vslam_resect.h"

struct vslam_prof_pending {
    int slot;
    hipEvent_t start, stop;
};

struct vslam_prof_slot {
    std::string name;
    double total_ms = 0;
    int64_t launches = 0;
};

struct vslam_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // second stream + fork/join events: independent stages (the k-d tree build is not an input of
    // match/RANSAC) run beside the main stream inside vslam_frontend_pairs
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // uploads (frame ingest) run on their own stream; ev_upload marks the last one enqueued
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_upload = nullptr;
    // recorded behind the raw mt19937 outputs produced ahead of time on the auxiliary stream (vslam_frontend_pairs / _sequence)
    hipEvent_t ev_raw = nullptr;
    // An independent stage (the k-d build: an output of the path, nobody's input) that vslam_frontend_pairs / _sequence hand
    // to the matching stages to be forked onto the auxiliary stream at the point where it disturbs them least:
    // aux_job_at = 1 after the matcher, 2 after the set mapping, 3 after the solves, 4 after the screen (0: at once / none).  vs_aux_job_point(ctx, k)
    // launches it when k is that point; the caller joins on ev_join.
    std::function<int()> aux_job;
    int aux_job_at = 0;
    int tree_fork = -1;   // VSLAM_OPT_TREE_FORK: where the batched front-end forks the k-d build (-1: by size; 0 in front of the matcher)
    int overlap_blur = 2;       // VSLAM_OVERLAP_BLUR: 0 blur on the main stream, otherwise on the auxiliary stream from min_eigen (where the gray image is complete) on
    // One of several contexts with batches in flight on this device (vs_ctx_create): blur on the main stream, the auxiliary
    // stream at the main stream's priority, streams it may never use made on first use.
    bool shared_chip = false;
    bool lazy_streams = false;   // the copy stream is made on first use
    int solve_split = 0;        // VSLAM_RANSAC_SOLVE_SPLIT (read when the context is made): 0 one solve kernel, 4 / 5 sweeps + closing kernel
    bool sets_prefetch = true;  // VSLAM_SETS_PREFETCH: the raw mt19937 outputs generated ahead of time on the auxiliary stream
    int ransac_min_matches = VSLAM_SET_SIZE;   // VSLAM_OPT_RANSAC_MIN_MATCHES
    int ransac_min_items = VSLAM_SET_SIZE;     // VSLAM_OPT_RANSAC_MIN_ITEMS: indices drawn per 8-wide set
    int ransac_solver = 0;                      // VSLAM_OPT_RANSAC_SOLVER: 0 exact Jacobi replay, 1 Gram / MFMA (not bit-exact)
    int match_shape = 0;                        // VSLAM_OPT_MATCH_SHAPE: 0 by size, 1 = 8 waves x 32 rows, 2 = 4 waves x 64 rows
    int match_form = 0;                         // VSLAM_OPT_MATCH_FORM: 0 default (FP4), 1 FP4, 2 int8
    int corner_window_pct = 135;                // VSLAM_OPT_CORNER_WINDOW_PCT
    int corner_list_cap = 0;                    // VSLAM_OPT_CORNER_LIST_CAP: 0 = 16 x max_corners + 4096, -1 = whole image
    bool pose_refit = false;        // VSLAM_OPT_POSE_REFIT: the pose chain and the tracking loop refit F over its inliers (refit.hip)
    bool pose_refine = false;       // VSLAM_OPT_POSE_REFINE: two-view bundle adjustment of each pair's pose and points (refine.hip)
    bool ransac_all_sums = false;   // VSLAM_OPT_RANSAC_ALL_SUMS: exact residual sum of every hypothesis (ransac_score_kernel)
    // where the corner detector's last batch left its per-frame counters (vslam_corner_stats reads them after a stream wait)
    const uint32_t *stat_counts = nullptr;
    const int32_t *stat_pool_count = nullptr;
    int stat_frames = 0, stat_pool_slots = 0;
    size_t stat_px = 0;
    std::string err;

    // named, grow-only device buffers (never allocated inside a timed loop after warm-up)
    struct Buf {
        void *ptr = nullptr;
        size_t bytes = 0;
    };
    std::map<std::string, Buf> arena;
    std::map<std::string, bool> attr_done;   // hipFuncSetAttribute is per device: remembered per context

    bool prof = false;
    std::vector<vslam_prof_slot> prof_slots;
    std::map<std::string, int> prof_index;
    std::vector<vslam_prof_pending> prof_pending;
    std::vector<hipEvent_t> event_pool;
};

#define VS_HIP(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e__ = (call);                                                            \
        if (e__ != hipSuccess) {                                                            \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                \
            return VSLAM_ERR_HIP;                                                           \
        }                                                                                   \
    } while (0)

#define VS_REQUIRE(ctx, cond, code)                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            if (ctx) (ctx)->err = std::string("requirement failed: ") + #cond;              \
            return (code);                                                                  \
        }                                                                                   \
    } while (0)

// The pointer-alignment contract of include/vslam_amd.h ("Alignment of device pointers"): a caller's device pointer on a
// multiple of `bytes`, checked on the host in front of the entry point's first launch and before it touches the arena.  The
// message names the argument.  A null pointer passes: whether an argument may be null is the entry point's own question.
#define VS_ALIGNED(ctx, ptr, bytes) VS_REQUIRE(ctx, reinterpret_cast<uintptr_t>(ptr) % (bytes) == 0, VSLAM_ERR_INVALID)
// the int32 / float / f64 arrays, whose requirement is their element's own: VS_REQUIRE(ctx, vs_ptr_bits(a, b, c) % 4 == 0, ...)
template <typename... P>
static inline uintptr_t vs_ptr_bits(const P *...p) {
    return (uintptr_t(0) | ... | reinterpret_cast<uintptr_t>(p));
}
// what every batched front-end call is handed (vslam_extract_features, vslam_frontend_*, vslam_track_sequences, the pipeline's
// submit forms): all of it checked before the first stage is queued, so that no call fails half-way through a batch.  Every
// per-frame and per-pair slice starts a multiple of kp_stride x 8 / 32 bytes (or whole int32s) behind its base, so the base
// decides for all of them.  The image (d_bgr) and the pattern are taken at any address.
static inline int vs_frontend_aligned(vslam_ctx *ctx, const uint32_t *d_seeds, const float *d_xy, const uint8_t *d_desc,
                                      const int32_t *d_nodes, const int32_t *d_n, const int32_t *d_matches,
                                      const int32_t *d_best, const float *d_F) {
    VS_ALIGNED(ctx, d_desc, 16);
    VS_ALIGNED(ctx, d_xy, 8);
    VS_ALIGNED(ctx, d_matches, 8);
    VS_REQUIRE(ctx, vs_ptr_bits(d_seeds, d_nodes, d_n, d_best, d_F) % 4 == 0, VSLAM_ERR_INVALID);
    return VSLAM_OK;
}

// sticky device-side error word (bit 0: a fixed-size candidate list overflowed); vslam_ctx_synchronize
// reads and clears it and reports VSLAM_ERR_CAPACITY
int vs_device_errflag(vslam_ctx *ctx, int32_t **out);
int vs_ctx_create(int device, bool shared_chip, vslam_ctx **out);   // vslam_ctx_create = (device, false, out)
std::string vs_errflag_message(int32_t flag);

// fork the pending auxiliary job (if it was asked for at `point`) onto the auxiliary stream behind everything queued so far
int vs_aux_job_point(vslam_ctx *ctx, int point);

// grow-only named workspace
int vs_arena_get(vslam_ctx *ctx, const char *name, size_t bytes, void **out);

// event bracket around one kernel launch when profiling is on
struct VsProfScope {
    vslam_ctx *ctx;
    vslam_prof_pending p;
    bool active;
    VsProfScope(vslam_ctx *c, const char *name);
    ~VsProfScope();
};

// Launchers queue on ctx->stream: this points it at another stream (the auxiliary one) until the end of the scope, on every
// return path.  Forking onto that stream and joining it again stay the caller's job.
struct VsStreamScope {
    vslam_ctx *ctx;
    hipStream_t saved;
    VsStreamScope(vslam_ctx *c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
    ~VsStreamScope() { ctx->stream = saved; }
};

static inline int vs_div_up(int a, int b) { return (a + b - 1) / b; }

// the caller's camera matrix (h_K, row-major f32) as a kernel argument
struct VsK {
    float v[9];
};
static inline VsK vs_pack_K(const float *h_K) {
    VsK K;
    for (int i = 0; i < 9; i++) K.v[i] = h_K[i];
    return K;
}

// Let `kernel` be launched with up to `bytes` of dynamic LDS; beyond the default limit a launch fails without this.  The
// attribute is per device, so it is set once per context and remembered under `key`.  When a launch needs it (the limit
// differs with the kernel's static LDS) is the caller's condition.
template <typename K>
int vs_allow_dynamic_lds(vslam_ctx *ctx, K kernel, const char *key, size_t bytes) {
    bool &done = ctx->attr_done[key];
    if (!done) {
        VS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        done = true;
    }
    return VSLAM_OK;
}

// A/B switches (slower kernel variants, stream arrangements, tile shapes measured and not chosen) exist only in the
// EXPERIMENTS build of the library (-DVSLAM_EXPERIMENTS -> libvslam_amd_exp.so, which tools/ab_*.py and the variant tests load
// through VSLAM_AMD_LIB / capi.load_library): the default build reads no environment variable and carries one kernel per stage.
#ifdef VSLAM_EXPERIMENTS
#include <cstdlib>
#define VS_EXPERIMENT_ENV(name) getenv(name)
#else
#define VS_EXPERIMENT_ENV(name) (static_cast<const char *>(nullptr))
#endif

#ifdef __HIPCC__
// Workgroups are dealt round-robin over the 8 XCDs (linear id L lands on XCD L % 8 — observed, used
// for speed only, never for correctness).  Remap a 1-D grid of ceil(items/8)*8*per_item blocks so that
// all `per_item` blocks of one item (frame / pair) share an XCD and therefore its 4 MiB L2.
__device__ __forceinline__ void vs_xcd_item_block(int linear, int per_item, int &item, int &blk) {
    const int xcd = linear & 7, slot = linear >> 3;
    item = ((slot / per_item) << 3) + xcd;
    blk = slot - (slot / per_item) * per_item;
}
#endif
static inline int vs_xcd_grid(int items, int per_item) { return vs_div_up(items, 8) * 8 * per_item; }

// Row segments per column strip for the streaming image kernels: about 90 rows per wave (6 warm-up rows each,
// 7 %), more and shorter segments (down to 24 rows) when the batch alone would leave the 1024 SIMDs with fewer
// than four waves each.
static inline int vs_stream_segments(int h, int frames, int strips) {
    int segs = h >= 135 ? (h + 45) / 90 : 1;
    const long long waves = (long long)frames * strips * segs;
    if (waves < 4096) {
        const long long want = (4096 + (long long)frames * strips - 1) / ((long long)frames * strips);
        const int most = h / 24 > 1 ? h / 24 : 1;
        segs = (int)(want < most ? want : most);
        if (segs < 1) segs = 1;
    }
    return segs;
}

// ---- stage launchers implemented in the .hip files (all async on ctx->stream) ----
// `pitch` (the image stages): bytes per row of the gray / blurred planes, >= w.  Packed rows pass w; a width that is no multiple
// of 4 may get rows of a multiple of 16 bytes whose tail holds the row's BORDER_REFLECT_101 continuation, so that the dword
// kernels take them (vs_padded_pitch in capi.hip).
int vs_launch_match(vslam_ctx *ctx, const uint8_t *d1, const int32_t *n1, const uint8_t *d2,
                    const int32_t *n2, int batch, int kp_stride, int32_t *pairs, int32_t *m,
                    int32_t *knn);
int vs_launch_ransac_sets(vslam_ctx *ctx, const uint32_t *seeds, const int32_t *m, int batch, int hyp,
                          int32_t *sets, uint32_t *draws);
// the same sets in two steps: raw mt19937 outputs (seed only; can run ahead on another stream), then the mapping
size_t vs_ransac_raw_words(int hyp);   // uint32 words of raw outputs per item
int vs_launch_ransac_mt(vslam_ctx *ctx, const uint32_t *seeds, int batch, int hyp, uint32_t *raw);
int vs_launch_ransac_map(vslam_ctx *ctx, const int32_t *m, int batch, int hyp, const uint32_t *raw, int32_t *sets,
                         uint32_t *draws);
int vs_launch_ransac(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs,
                     const int32_t *m, const int32_t *sets, int batch, int kp_stride, int hyp,
                     float threshold, float *F, uint8_t *mask, int32_t *best, int32_t *matches,
                     float *hypF, int32_t *hyp_count, float *hyp_sum);
int vs_launch_ransac_solve(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs,
                           const int32_t *m, const int32_t *sets, int batch, int kp_stride, int hyp,
                           float *hypF);
int vs_launch_ransac_evaluate(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *pairs,
                              const int32_t *m, const float *hypF, int batch, int kp_stride, int hyp,
                              float threshold, float *F, uint8_t *mask, int32_t *best, int32_t *matches,
                              int32_t *hyp_count, float *hyp_sum);
// the winner refitted over its inliers (refit.hip); F_out may be F_in
int vs_launch_refit(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *matches, const int32_t *best, int batch,
                    int kp_stride, const float *F_in, float *F_out, double *stats);
// two-view bundle adjustment of R, t and the points, in place (refine.hip); c2 = K [R | t] of what it leaves in R and t
int vs_launch_refine_pairs(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *matches, const int32_t *best, int batch,
                           int kp_stride, const float *h_K, float gate_sq, int max_iterations, float *R, float *t, float *c2,
                           float *points4d, double *stats);
constexpr int kVsPoseRefineIterations = 20;   // what VSLAM_OPT_POSE_REFINE runs with; its gate is 4 x the filter's threshold_sq
int vs_launch_kdtree_build(vslam_ctx *ctx, const float *xy, const int32_t *n, int batch, int kp_stride,
                           int32_t *nodes);
int vs_launch_kdtree_radius(vslam_ctx *ctx, const int32_t *nodes, const float *xy, const int32_t *n,
                            int batch, int kp_stride, const float *queries, const int32_t *nq,
                            int q_stride, float radius, int32_t *hits, int32_t *counts, int hit_cap);
int vs_launch_kdtree_nearest(vslam_ctx *ctx, const int32_t *nodes, const float *xy, const int32_t *n,
                             int batch, int kp_stride, const float *queries, const int32_t *nq,
                             int q_stride, float max_distance_sq, int32_t *best_idx);
int vs_launch_kdtree_cell_table(vslam_ctx *ctx, const int32_t *nodes, const float *xy, const int32_t *n, int batch,
                                int kp_stride, int slots, uint32_t *table, int32_t *ok);
int vs_launch_bgr2gray(vslam_ctx *ctx, const uint8_t *bgr, int frames, int w, int h, int stride,
                       uint8_t *gray, int pitch);
int vs_launch_min_eigen(vslam_ctx *ctx, const uint8_t *gray, int frames, int w, int h, int pitch, float *eig,
                        uint32_t *frame_max_bits);
// per-frame counters of the corner pipeline: one zero-initialised block (select.hip lays it out)
struct VsCornerCounters {
    uint32_t *counts;    // entries in the detector's list
    uint32_t *fmax;      // ordered exact maximum response
    uint32_t *low;       // two-tier detector: certified lower bound of maximum / c0 (ordered)
    uint32_t *count2;    // exact keys above the cut
    uint32_t *count3;    // exact keys of the rerun (flagged frames, nothing cut)
    uint32_t *need;      // the selection ran out of candidates above the cut: rerun this frame with everything
    uint32_t *cutkey;    // ordered response below which keys2 is incomplete (0: complete)
    uint32_t *hist;      // two-tier detector: the listed upper bounds by magnitude
};
// Whole-image scratch for the few frames the bounded two-tier path cannot finish (see vs_launch_good_features): `slots`
// sets of (keys, response image, per-pixel state).  A frame claims a slot by a ticket on `count`; everything per slot.
struct VsCornerPool {
    int32_t *count = nullptr;      // tickets handed out (may exceed slots: the excess frames raise bit 2 of the error word)
    int32_t *frame = nullptr;      // [slots] the frame filed under each slot
    uint32_t *counts = nullptr;    // [slots] candidates found
    uint32_t *fmax = nullptr;      // [slots] ordered exact maximum response
    unsigned long long *keys = nullptr;   // [slots][key_cap]
    float *eig = nullptr;          // [slots][w * h]
    uint8_t *state = nullptr;      // [slots][w * h]
    size_t key_cap = 0;
    int slots = 0;
    // the frames' gray rows, for the selection's test of a frame that overflowed its list: a constant image has no corner and
    // needs no slot (select.hip)
    const uint8_t *gray = nullptr;
    int pitch = 0;
};
#ifdef __HIPCC__
__device__ __forceinline__ int vs_pool_used(const VsCornerPool &p) {
    const int used = *p.count;
    return used < p.slots ? used : p.slots;
}
#endif
int vs_launch_pool_candidates(vslam_ctx *ctx, const uint8_t *gray, int w, int h, int pitch, double quality,
                              const VsCornerPool &pool);
size_t vs_response_hist_words(int frames);
// `gray` still to be formed from a 3-byte image (cvtColor is then the detector's job: fused into its first kernel when
// the layout allows, a launch of its own otherwise)
struct VsBgrSource {
    const uint8_t *data;
    int stride;   // bytes per row
};
int vs_launch_response_candidates(vslam_ctx *ctx, const uint8_t *gray, int frames, int w, int h, int pitch, double quality,
                                  float *eig, const VsCornerCounters &c, unsigned long long *keys,
                                  unsigned long long *keys2, size_t key_cap, uint32_t n_safe, int *raw_list,
                                  const VsBgrSource *bgr = nullptr);
int vs_launch_corner_exact(vslam_ctx *ctx, const uint8_t *gray, int frames, int w, int h, int pitch, const VsCornerCounters &c,
                           const unsigned long long *keys, unsigned long long *keys2, size_t key_cap, uint32_t n_safe,
                           int mode);
// fork_aux: record ev_fork and make the auxiliary stream wait on it once the response kernels are queued (the caller runs an
// independent stage there beside the selection)
int vs_launch_good_features(vslam_ctx *ctx, const uint8_t *gray, int frames, int w, int h, int pitch,
                            int max_corners, double quality, double min_distance, int kp_stride,
                            float *xy, int32_t *n, const VsBgrSource *bgr = nullptr, bool fork_aux = false);
int vs_launch_gaussian7(vslam_ctx *ctx, const uint8_t *gray, int frames, int w, int h, int pitch, uint8_t *out);
int vs_launch_gray_pad(vslam_ctx *ctx, const uint8_t *src, int frames, int w, int h, uint8_t *dst, int pitch);
int vs_launch_gray_unpad(vslam_ctx *ctx, const uint8_t *src, int frames, int w, int h, int pitch, uint8_t *dst);
int vs_launch_gaussian7_rows(vslam_ctx *ctx, const uint8_t *src, uint8_t *dst, int frames, size_t frame_pitch, int w, int h,
                             int y_begin, int y_end);
// the rotated rBRIEF table (513 words) queued ahead of a describe call; rotated_table: that table, nullptr to rotate it there
int vs_launch_rbrief_rotate(vslam_ctx *ctx, const int8_t *pattern, float ca, float sa, const int32_t **table);
int vs_launch_orb_describe(vslam_ctx *ctx, const uint8_t *blurred, int frames, int w, int h, int pitch,
                           const float *xy_in, const int32_t *n_in, int kp_stride, float ca, float sa,
                           const int8_t *pattern, const int32_t *rotated_table, float *xy_out, uint8_t *desc,
                           int32_t *n_out);
int vs_launch_extract_grid(vslam_ctx *ctx, uint8_t *bgr, int frames, int w, int h, int stride, int nrows, int ncols,
                           const int8_t *pattern, int kp_cap, float *xy, uint8_t *desc, float *angle_octave,
                           int32_t *n_out);
int vs_launch_extract_Rt(vslam_ctx *ctx, const float *F, const int32_t *best, int batch, const float *h_K, float *R,
                         float *t, float *c2);
int vs_launch_triangulate(vslam_ctx *ctx, const float *xy1, const float *xy2, const int32_t *matches,
                          const int32_t *best, int batch, int kp_stride, const float *h_K, const float *c2,
                          float *points4d);
int vs_launch_triangulate_points(vslam_ctx *ctx, const float *p1, const float *p2, int n, const float *h_c1, const float *h_c2,
                                 float *points4d);
int vs_launch_associate(vslam_ctx *ctx, const float *map_points, const int32_t *n_map, int batch, int map_stride,
                        const float *c2, int img_w, int img_h, const int32_t *nodes, const float *xy, const uint8_t *desc,
                        const int32_t *n_kp, int kp_stride, const int32_t *obs_offsets, const uint8_t *obs_desc,
                        int obs_stride, float radius, uint32_t dist_threshold, int32_t *map_point_ids, int32_t *claim);
int vs_launch_reproj_filter(vslam_ctx *ctx, const float *points4d, const float *xy1, const float *xy2, const int32_t *matches,
                            const int32_t *best, int batch, int kp_stride, const float *h_K, const float *c2,
                            const int32_t *map_point_ids, float threshold_sq, int32_t *out_idx, int32_t *out_n,
                            double *out_err);

// ---- the world frame (world.hip); map.hip drives it behind a map step when one is attached ----
struct vslam_world {
    vslam_ctx *ctx = nullptr;
    int tracks = 0, max_frames = 0, kp_stride = 0, min_links = 0;
    int frames = 1;
    double *Twc = nullptr;          // [tracks][max_frames][16]
    float *pose = nullptr;          // [tracks][max_frames][16]
    double *scale = nullptr;        // [tracks][max_frames]
    int32_t *links = nullptr;       // [tracks][max_frames]
    double *carry = nullptr;        // [tracks][kp_stride][3]
    int32_t *carry_idx = nullptr;   // [tracks][kp_stride]
    // made by vs_world_bind when a map takes the world on
    int map_capacity = 0;
    float *world_points = nullptr;  // [tracks][map_capacity][4]
    int32_t *size_before = nullptr; // [tracks] the map's sizes ahead of the step
    // vslam_world_set_resection (include/vslam_resect.h): the table the step writes the new carry into (the two change places
    // after every step) and the per-step statistics; allocated once, when resection is first set
    bool resect = false;
    vslam_resect_params resect_params{};
    double *carry_next = nullptr;        // [tracks][kp_stride][3]
    int32_t *carry_idx_next = nullptr;   // [tracks][kp_stride]
    double *resect_stats = nullptr;      // [tracks][max_frames][4]
    // include/vslam_fuse.h: made by the first vslam_world_fuse / vslam_world_cull.  fusion: bit 0 a fusion exists, bit 1 a cull has run;
    // 0 = "no fusion", d_fuse_to (if made) the identity
    int32_t *fuse_to = nullptr;          // [tracks][map_capacity]
    int fusion = 0;
    // include/vslam_fuse_project.h: the extra log, made by the first vslam_world_fuse_project; fusion bit 2: extras exist
    int32_t *extra_point = nullptr, *extra_frame = nullptr, *extra_kp = nullptr;   // [tracks][extra_capacity]
    uint8_t *extra_desc = nullptr;       // [tracks][extra_capacity][32]
    int32_t *n_extra = nullptr;          // [tracks]
    int extra_capacity = 0;              // the map's obs_capacity when the log was made
    std::vector<void *> owned;
};
int vs_world_bind(vslam_ctx *ctx, vslam_world *w, int map_capacity);
// around one map step: the sizes ahead of it; then the world step and the lift of rows [size before, size after)
int vs_world_before_map_step(vslam_ctx *ctx, vslam_world *w, const int32_t *sizes);
int vs_world_after_map_step(vslam_ctx *ctx, vslam_world *w, const int32_t *matches, const int32_t *best, const float *points4d,
                            const float *R, const float *t, const int32_t *n_last, const int32_t *n_cur, const float *map_points,
                            const int32_t *sizes, const float *xy_cur, const float *h_K);
// resect.hip: the resection behind a plain step that wrote frame `fid` and the new carry (carry_next / carry_idx_next)
int vs_launch_world_resect(vslam_ctx *ctx, vslam_world *w, int fid, const int32_t *matches, const int32_t *best, const float *points4d,
                           const float *R, const float *t, const int32_t *n_last, const int32_t *n_cur, const float *xy_cur,
                           const float *h_K);
int vs_world_resect_reset(vslam_ctx *ctx, vslam_world *w);
bool vs_resect_params_ok(const vslam_resect_params &p);

// ---- a world attached to a map, for the calls that read both (adjust.hip, search.hip, pnp.hip) ----
vslam_world *vs_map_world(vslam_map *map);   // map.hip: the world the map has attached, or null
// `world` is this context's, the one attached to `map`, and lifted
static inline bool vs_world_of_map(vslam_ctx *ctx, vslam_world *world, vslam_map *map) {
    return world->ctx == ctx && vs_map_world(map) == world && world->world_points;
}
// search.hip: vs_world_of_map, and the world has as many frames as the map, whose view is *m
int vs_world_map_view(vslam_ctx *ctx, vslam_world *world, vslam_map *map, vslam_map_arrays *m);
// What vslam_world_search and vslam_world_relocalise open with (search.hip): vs_world_map_view, the alignment of the current frame's
// arrays, and the arena workspace of both calls, with the map's CSR and its observation descriptors queued into it.
struct VsWorldCorr {
    vslam_map_arrays m;
    int32_t *off, *kp_of_point, *dist;   // [tracks][map_capacity + 1], [tracks][map_capacity] twice
    uint8_t *obs_desc;                   // [tracks][obs_capacity][32]
    double *R, *T, *mark;                // [tracks][9], [tracks][3], [tracks][4]: a pose and what vs_world_search_writeback reads
    double *corr_points;                 // [tracks][kp_stride][3]
    float *corr_xy;                      // [tracks][kp_stride][2]
};
int vs_world_corr_begin(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur,
                        const double *d_stats, VsWorldCorr *c);
// vslam_world_search's write-back (search.hip): frame f1 of every track whose mark[4 b + 3] is a number gets (R, T) [tracks][9] /
// [tracks][3] written as d_Twc / d_pose and the latest carry re-expressed
int vs_world_search_writeback(vslam_ctx *ctx, vslam_world *world, int f1, double *R, double *T, double *mark);
// fuse.hip.  The CSR of the map's observations as the world sees it, which every world call that reads observations obtains here:
// off [tracks][map_capacity + 1]; frame and kp [tracks][obs_capacity] (both or neither); desc [tracks][obs_capacity][32] or null.
// Without a fusion exactly the launches of vslam_map_observations (frame, kp given) and vslam_map_observation_descriptors (desc
// given); with one, the map's lists fused with d_mask = d_fuse_to (include/vslam_fuse.h) and the descriptors gathered through
// d_out_src.
int vs_world_csr(vslam_ctx *ctx, vslam_world *world, vslam_map *map, int32_t *off, int32_t *frame, int32_t *kp, uint8_t *desc);
// camera f = recorded frame f of every track, from d_Twc as include/vslam_adjust.h forms "camera c" (fuse.hip's world_cameras_kernel):
// R [tracks][max_frames][9], T [tracks][max_frames][3], n_cams [tracks] = frames
int vs_world_cameras(vslam_ctx *ctx, vslam_world *world, int max_frames, int frames, double *R, double *T, int32_t *n_cams);
int vs_world_fusion_reset(vslam_ctx *ctx, vslam_world *world);   // "no fusion": d_fuse_to (if made) the identity, the extra log empty
// d_fuse_to made if the world has none yet (a vs_world_fusion_reset then: so ahead of anything that vslam_world_fuse is to keep)
int vs_world_fusion_make(vslam_ctx *ctx, vslam_world *world);
// fuse_project.hip, for a world whose extras exist (include/vslam_fuse_project.h, "The world's CSR once extras exist").  The map's
// log (log_off [tracks][P + 1], log_frame / log_kp [tracks][O], sizes [tracks]) with every point's admitted extras appended to its
// row: off [tracks][P + 1], frame / kp / src [tracks][O] (src: the map's row, or O + e for extra e); work [tracks][2 P].
int vs_world_extras_merge(vslam_ctx *ctx, vslam_world *world, const int32_t *sizes, int P, int O, const int32_t *log_off, const int32_t *log_frame,
                          const int32_t *log_kp, int32_t *off, int32_t *frame, int32_t *kp, int32_t *src, int32_t *work);
// the descriptors of a fusion's merged rows over such lists: row o is the map's row or the extra that src[out_src[o]] names
int vs_world_extras_gather_desc(vslam_ctx *ctx, vslam_world *world, int P, int O, const int32_t *out_off, const int32_t *out_src, const int32_t *src,
                                const uint8_t *log_desc, uint8_t *desc);
struct vslam_match_params;   // include/vslam_pnp.h
bool vs_match_params_ok(const vslam_match_params &p);   // search.hip
