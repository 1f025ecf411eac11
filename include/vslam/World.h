// The world frame of the resident map as a C++ object: a vslam_world (include/vslam_amd.h, "the world frame") with the
// lifetime of the object.  The reference has nothing like it -- its map keeps every pair's points in the last frame's camera
// coordinates and in the pair's own unit -- so this is no drop-in; it is what a consumer of include/vslam/*.h uses to get
// camera -> world poses and points in one coordinate system per track.  Header-only over the C ABI; arrays are device pointers.
// For the one-track PointMap of include/vslam/PointMap.h see vslam::map_attach_world there.
#pragma once
#include <stdexcept>
#include <string>

#include "../vslam_amd.h"
#include "../vslam_resect.h"
#include "../vslam_adjust.h"
#include "../vslam_search.h"
#include "../vslam_pnp.h"
#include "../vslam_sim3.h"
#include "../vslam_graph.h"
#include "../vslam_fuse.h"
#include "../vslam_fuse_project.h"
#include "../vslam_tracks.h"

namespace vslam {

class World {
public:
    // Capacities are fixed here; nothing is allocated afterwards.  Destroy it before the context, and after a map it is
    // attached to.  min_links: links a pair needs to set its own scale (otherwise it keeps the previous one).
    World(vslam_ctx *ctx, int tracks, int max_frames, int kp_stride, int min_links = 8) : ctx_(ctx) {
        check(vslam_world_create(ctx, tracks, max_frames, kp_stride, min_links, &world_), "vslam_world_create");
    }
    ~World() {
        if (world_) vslam_world_destroy(world_);
    }
    World(const World &) = delete;
    World &operator=(const World &) = delete;

    void reset() { check(vslam_world_reset(ctx_, world_), "vslam_world_reset"); }
    // one frame for every track, stream-ordered: [tracks][...] device arrays as vslam_world_step takes them
    void step(const int32_t *d_matches, const int32_t *d_best, const float *d_points4d, const float *d_R, const float *d_t,
              const int32_t *d_n_last, const int32_t *d_n_cur) {
        check(vslam_world_step(ctx_, world_, d_matches, d_best, d_points4d, d_R, d_t, d_n_last, d_n_cur), "vslam_world_step");
    }
    // Tracking against the map (include/vslam_resect.h), at frame 0 only: from now on the world is stepped with step_resect, which
    // resects each frame's pose against the carried points.  params: nullptr for the defaults.  clear_resection() undoes it.
    void set_resection(const vslam_resect_params *params = nullptr) {
        vslam_resect_params p;
        check(vslam_resect_params_default(&p), "vslam_resect_params_default");
        check(vslam_world_set_resection(world_, params ? params : &p), "vslam_world_set_resection");
    }
    void clear_resection() { check(vslam_world_set_resection(world_, nullptr), "vslam_world_set_resection"); }
    // step's arrays, the current frame's keypoints d_xy_cur [tracks][kp_stride][2] and the camera matrix h_K [9] (host, row-major)
    void step_resect(const int32_t *d_matches, const int32_t *d_best, const float *d_points4d, const float *d_R, const float *d_t,
                     const int32_t *d_n_last, const int32_t *d_n_cur, const float *d_xy_cur, const float *h_K) {
        check(vslam_world_step_resect(ctx_, world_, d_matches, d_best, d_points4d, d_R, d_t, d_n_last, d_n_cur, d_xy_cur, h_K),
              "vslam_world_step_resect");
    }
    // [tracks][max_frames][4] f64 on the device: each step's participants, mean rho before / after, accepted steps; nullptr while
    // resection has never been set
    double *resection_stats() const {
        double *d = nullptr;
        check(vslam_world_resection_view(world_, &d), "vslam_world_resection_view");
        return d;
    }
    // rows [d_lo, d_hi) per track of the points of pair (frame - 1 -> frame) into d_out; other rows keep their bits
    void lift(int frame, const float *d_points, int stride, const int32_t *d_lo, const int32_t *d_hi, float *d_out) {
        check(vslam_world_lift(ctx_, world_, frame, d_points, stride, d_lo, d_hi, d_out), "vslam_world_lift");
    }
    vslam_world_arrays view() const {
        vslam_world_arrays a;
        check(vslam_world_view(world_, &a), "vslam_world_view");
        return a;
    }
    void attach_to(vslam_map *map) { check(vslam_map_attach_world(map, world_), "vslam_map_attach_world"); }
    void render(vslam_map *map, int track_lo, int track_count, const vslam_view &view, int width, int height, int row_stride,
                uint8_t *d_bgr_out, float *d_depth_out = nullptr) {
        check(vslam_world_render(ctx_, world_, map, track_lo, track_count, &view, width, height, row_stride, d_bgr_out, d_depth_out),
              "vslam_world_render");
    }
    // The last `window` frames of every track and the map points they observe adjusted together, in place (vslam_world_adjust,
    // include/vslam_adjust.h).  The world must be the one attached to `map`; d_xy [tracks * xy_frames][kp_stride][2] as
    // vslam_track_sequences leaves it; params: nullptr for the defaults; d_stats [tracks][4] f64 or nullptr.
    void adjust(vslam_map *map, const float *d_xy, int xy_frames, const float *h_K, int window = 8,
                const vslam_adjust_params *params = nullptr, double *d_stats = nullptr) {
        check(vslam_world_adjust(ctx_, world_, map, d_xy, xy_frames, h_K, window, params, d_stats), "vslam_world_adjust");
    }
    // Every track's world points searched by projection in the caller's latest frame, from the pose of the last frame recorded
    // (vslam_world_search, include/vslam_search.h).  The world must be the one attached to `map`; d_xy_cur / d_desc_cur / d_n_cur
    // [tracks][kp_stride]; search: nullptr for the defaults; resect: nullptr to search only, otherwise the frame's pose is
    // resected against what was found and written back where that moved it.  d_corr_point / d_corr_kp [tracks][kp_stride],
    // d_n_corr [tracks]; d_stats [tracks][4] f64 (the resection's) or nullptr.
    void search(vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur, const int32_t *d_n_cur, const float *h_K, int width,
                int height, int32_t *d_corr_point, int32_t *d_corr_kp, int32_t *d_n_corr, const vslam_search_params *search = nullptr,
                const vslam_resect_params *resect = nullptr, double *d_stats = nullptr) {
        check(vslam_world_search(ctx_, world_, map, d_xy_cur, d_desc_cur, d_n_cur, h_K, width, height, search, resect, d_corr_point,
                                 d_corr_kp, d_n_corr, d_stats),
              "vslam_world_search");
    }
    // The pose of the caller's latest frame found from the map alone, for every track (vslam_world_relocalise, include/vslam_pnp.h):
    // the world's points matched to the keypoints by descriptor, P3P RANSAC over the matches, the polish (nullptr: none), and for
    // the tracks that were found the write-back of search().  The last recorded pose is not read.  The world must be the one
    // attached to `map`; d_seeds [tracks]; match / pnp: nullptr for the defaults; d_found, d_winner, d_n_inliers, d_n_corr [tracks];
    // d_corr_point / d_corr_kp [tracks][kp_stride]; d_stats [tracks][4] f64 (the polish's) or nullptr.
    void relocalise(vslam_map *map, const float *d_xy_cur, const uint8_t *d_desc_cur, const int32_t *d_n_cur, const float *h_K,
                    const uint32_t *d_seeds, int32_t *d_found, int32_t *d_winner, int32_t *d_n_inliers, int32_t *d_corr_point,
                    int32_t *d_corr_kp, int32_t *d_n_corr, const vslam_resect_params *polish = nullptr, const vslam_pnp_params *pnp = nullptr,
                    const vslam_match_params *match = nullptr, double *d_stats = nullptr) {
        check(vslam_world_relocalise(ctx_, world_, map, d_xy_cur, d_desc_cur, d_n_cur, h_K, d_seeds, match, pnp, polish, d_found, d_winner,
                                     d_n_inliers, d_corr_point, d_corr_kp, d_n_corr, d_stats),
              "vslam_world_relocalise");
    }
    // The similarity between two recorded frames' maps for `items` pairs (track_a, frame_a, track_b, frame_b) (vslam_world_sim3,
    // include/vslam_sim3.h: every array is that call's): the camera-to-camera model in d_scale / d_R / d_T and the world-to-world
    // similarity X_a = s_w R_w X_b + t_w in d_s_w / d_R_w / d_t_w, both written where an item is found.  The world must be the one
    // attached to `map`; nothing is written into either.  params / polish: nullptr for the defaults / no polish; d_point_a,
    // d_point_b and d_stats may be nullptr.
    void sim3(vslam_map *map, const int32_t *d_track_a, const int32_t *d_frame_a, const int32_t *d_track_b, const int32_t *d_frame_b, int items,
              const int32_t *d_matches, const int32_t *d_n_matches, const float *d_xy_a, const float *d_xy_b, const float *h_K,
              const uint32_t *d_seeds, double *d_scale, double *d_R, double *d_T, double *d_s_w, double *d_R_w, double *d_t_w, int32_t *d_found,
              int32_t *d_n_corr, int32_t *d_n_inliers, int32_t *d_winner, int32_t *d_point_a = nullptr, int32_t *d_point_b = nullptr,
              const vslam_resect_params *polish = nullptr, const vslam_sim3_params *params = nullptr, double *d_stats = nullptr) {
        check(vslam_world_sim3(ctx_, world_, map, d_track_a, d_frame_a, d_track_b, d_frame_b, items, d_matches, d_n_matches, d_xy_a, d_xy_b, h_K,
                               d_seeds, params, polish, d_scale, d_R, d_T, d_s_w, d_R_w, d_t_w, d_found, d_n_corr, d_n_inliers, d_winner,
                               d_point_a, d_point_b, d_stats),
              "vslam_world_sim3");
    }
    // Every listed track's world carried through X' = s R X + t (vslam_world_apply_sim3): h_track [items] on the HOST, distinct;
    // d_s [items], d_R [items][9], d_t [items][3], d_apply [items] on the device.
    void apply_sim3(vslam_map *map, const int32_t *h_track, const double *d_s, const double *d_R, const double *d_t, const int32_t *d_apply,
                    int items) {
        check(vslam_world_apply_sim3(ctx_, world_, map, h_track, d_s, d_R, d_t, d_apply, items), "vslam_world_apply_sim3");
    }
    // The loops inside each track closed and their error spread over the frames in between (vslam_world_close_loops,
    // include/vslam_graph.h: every array is that call's): d_track, d_frame_a, d_frame_b, d_use [loops] and the camera a -> camera b
    // model d_scale / d_R / d_T of each on the device; seq_weight / loop_weight: three host numbers or nullptr (1 1 1); params:
    // nullptr for the defaults; d_stats [tracks][4] or nullptr.
    void close_loops(vslam_map *map, const int32_t *d_track, const int32_t *d_frame_a, const int32_t *d_frame_b, const int32_t *d_use,
                     const double *d_scale, const double *d_R, const double *d_T, int loops, const double *seq_weight = nullptr,
                     const double *loop_weight = nullptr, const vslam_graph_params *params = nullptr, double *d_stats = nullptr) {
        check(vslam_world_close_loops(ctx_, world_, map, d_track, d_frame_a, d_frame_b, d_use, d_scale, d_R, d_T, loops, seq_weight, loop_weight,
                                      params, d_stats),
              "vslam_world_close_loops");
    }
    // The map points of every track that share an observation fused into groups (vslam_world_fuse, include/vslam_fuse.h): the
    // world's d_fuse_to written, the rows of the newly absorbed points in d_world_points set to NaN.  The world must be the one
    // attached to `map`; d_stats [tracks][4] int32 or nullptr.
    void fuse(vslam_map *map, int32_t *d_stats = nullptr) { check(vslam_world_fuse(ctx_, world_, map, d_stats), "vslam_world_fuse"); }
    // The world points their observations do not support culled (vslam_world_cull, include/vslam_fuse.h); d_xy as adjust() takes it;
    // params: nullptr for the defaults; d_stats [tracks][4] int32 or nullptr.
    void cull(vslam_map *map, const float *d_xy, int xy_frames, const float *h_K, const vslam_cull_params *params = nullptr,
              int32_t *d_stats = nullptr) {
        check(vslam_world_cull(ctx_, world_, map, d_xy, xy_frames, h_K, params, d_stats), "vslam_world_cull");
    }
    // Geometric fusing (vslam_world_fuse_project, include/vslam_fuse_project.h): every world point searched by projection in the
    // recorded frames frame_lo <= f < frame_hi that do not see it yet, the found pairs appended to the world's extra log, then what
    // fuse() does over the lists with the extras in them.  d_xy / d_desc / d_n_kp: the keypoints of every frame,
    // [tracks][xy_frames][kp_stride]; search: nullptr for the defaults; d_stats [tracks][8] int32 or nullptr.
    void fuse_project(vslam_map *map, const float *d_xy, const uint8_t *d_desc, const int32_t *d_n_kp, int xy_frames, const float *h_K, int width,
                      int height, int frame_lo, int frame_hi, const vslam_search_params *search = nullptr, int32_t *d_stats = nullptr) {
        check(vslam_world_fuse_project(ctx_, world_, map, d_xy, d_desc, d_n_kp, xy_frames, h_K, width, height, frame_lo, frame_hi, search, d_stats),
              "vslam_world_fuse_project");
    }
    // Every world point triangulated anew from all the observations of its row of the world's CSR, in place; only the rows that come
    // out with status 0 are written (vslam_world_retriangulate, include/vslam_tracks.h).  d_xy as adjust() takes it; params: nullptr
    // for the defaults; d_status [tracks][map_capacity] int32 or nullptr; d_stats [tracks][4] int32 or nullptr.
    void retriangulate(vslam_map *map, const float *d_xy, int xy_frames, const float *h_K, const vslam_track_params *params = nullptr,
                       int32_t *d_status = nullptr, int32_t *d_stats = nullptr) {
        check(vslam_world_retriangulate(ctx_, world_, map, d_xy, xy_frames, h_K, params, d_status, d_stats), "vslam_world_retriangulate");
    }
    // The CSR of the map's observations as this world sees it -- merged once a fusion exists, the map's own otherwise
    // (vslam_world_observations, include/vslam_fuse.h): d_offsets [tracks][map_capacity + 1], d_frame_ids / d_point_ids
    // [tracks][obs_capacity], d_desc [tracks][obs_capacity][32] or nullptr.
    void observations(vslam_map *map, int32_t *d_offsets, int32_t *d_frame_ids, int32_t *d_point_ids, uint8_t *d_desc = nullptr) {
        check(vslam_world_observations(ctx_, world_, map, d_offsets, d_frame_ids, d_point_ids, d_desc), "vslam_world_observations");
    }
    // [tracks][map_capacity] int32 on the device, nullptr while there is no fusion; *state: bit 0 fused, bit 1 culled
    int32_t *fuse_to(int32_t *state = nullptr) const {
        int32_t *d = nullptr;
        check(vslam_world_fusion_view(world_, &d, state), "vslam_world_fusion_view");
        return d;
    }
    vslam_world *handle() const { return world_; }

private:
    void check(int rc, const char *what) const {
        if (rc != VSLAM_OK) throw std::runtime_error(std::string(what) + ": " + vslam_last_error(ctx_));
    }
    vslam_ctx *ctx_ = nullptr;
    vslam_world *world_ = nullptr;
};

}  // namespace vslam
