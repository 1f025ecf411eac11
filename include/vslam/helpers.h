// Drop-in for the reference's include/helpers.h: the same two free functions and the two inline matrix helpers, computed on
// the MI355X through include/vslam_amd.h (vslam_extract_Rt / vslam_triangulate_points), plus the batch form of the capture
// loop's map-association block.  With this header src/vslam.cpp:82,186 reach the device versions unchanged.
#pragma once
#include <iostream>
#include <vector>

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
#include "../vslam_places.h"
#include "Frame.h"
#include "cvlite.h"
#include "vslam_internal.h"

#ifndef VSLAM_HAVE_OPENCV
// cv::Mat's stream output in OpenCV's default format ("[a, b;\n c, d]"), for print_matrix on builds without OpenCV
inline std::ostream &operator<<(std::ostream &os, const cv::Mat &m) {
    os << '[';
    for (int r = 0; r < m.rows; r++) {
        for (int c = 0; c < m.cols * m.channels(); c++) {
            if (c) os << ", ";
            if (m.depth() == CV_32F) os << m.ptr<float>(r)[c];
            else os << (int)m.ptr<unsigned char>(r)[c];
        }
        if (r + 1 < m.rows) os << ";\n ";
    }
    return os << ']';
}
#endif

// reference: include/helpers.h:9-11
inline void print_matrix(const cv::Mat &mat, const char *name) {
    std::cout << name << '\n' << mat << '\n' << '\n';
}

#ifdef VSLAM_HAVE_OPENCV
// reference: include/helpers.h:13-15 (cv::FileStorage exists only where OpenCV is installed)
inline void write_matrix(const cv::Mat &mat, const char *name, cv::FileStorage &fs) {
    fs << name << mat;
}
#endif

// reference: include/helpers.h:17, src/helpers.cpp:3-35.  fundamental, K: 3 x 3 CV_32F; rotation 3 x 3, translation 3 x 1.
void extract_Rt(const cv::Mat &fundamental, const cv::Mat &K, cv::Mat &rotation, cv::Mat &translation);

// reference: include/helpers.h:19, src/helpers.cpp:37-80.  p1, p2: N x 2 CV_32F (continuous, as the reference reads them);
// c1, c2: 3 x 4 CV_32F; points_4d: N x 4 CV_32F rows (x, y, z, 1).
void triangulate(const cv::Mat &p1, const cv::Mat &p2, const cv::Mat &c1, const cv::Mat &c2, cv::Mat &points_4d);

namespace vslam {
// For callers whose features and RANSAC results are already on the device (vslam_match_features / vslam_frontend_*): the
// winners d_F [batch][9] refitted in place over their inlier matches, stream-ordered on `ctx` -- vslam_refit_fundamental with
// d_F_out = d_F_in; throws std::runtime_error with vslam_last_error on failure.  d_stats [batch][4] f64 or nullptr.
// RansacFilter::refit_fundamental is the host-vector form.
void refit_fundamental(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const s32 *d_matches, const s32 *d_best, int batch,
                       int kp_stride, float *d_F, f64 *d_stats = nullptr);

// Two-view bundle adjustment of each pair's pose and points (vslam_refine_pairs, include/vslam_amd.h), in place on the device
// arrays d_R [batch][9], d_t [batch][3], d_points4d [batch][kp_stride][4] as vslam_extract_Rt / vslam_triangulate wrote them;
// d_c2 [batch][12] receives K [R | t].  K: 3 x 3 CV_32F.  Stream-ordered on `ctx`; throws std::runtime_error with
// vslam_last_error on failure.  d_stats [batch][4] f64 or nullptr.
void refine_pairs(vslam_ctx *ctx, const float *d_xy1, const float *d_xy2, const s32 *d_matches, const s32 *d_best, int batch,
                  int kp_stride, const cv::Mat &K, float gate_sq, int max_iterations, float *d_R, float *d_t, float *d_c2,
                  float *d_points4d, f64 *d_stats = nullptr);

// Tracking against the map: the pose-only adjustment of each item's d_R [batch][9] / d_T [batch][3] (f64, in place) from its
// d_n [batch] correspondences d_points [batch][stride][3] f64 seen at d_xy [batch][stride][2] f32 (vslam_resect_poses,
// include/vslam_resect.h).  K: 3 x 3 CV_32F; params: nullptr for the defaults.  Stream-ordered on `ctx`; throws
// std::runtime_error with vslam_last_error on failure.  d_stats [batch][4] f64 or nullptr.
void resect_poses(vslam_ctx *ctx, const f64 *d_points, const float *d_xy, const s32 *d_n, int batch, int stride, const cv::Mat &K,
                  f64 *d_R, f64 *d_T, f64 *d_stats = nullptr, const vslam_resect_params *params = nullptr);

// A window of cameras and the points they share adjusted together, for a batch of items the caller holds on the device
// (vslam_adjust_windows, include/vslam_adjust.h: the arrays and strides are that call's).  K: 3 x 3 CV_32F; params: nullptr for
// the defaults; d_stats [batch][4] f64 or nullptr.  Stream-ordered on `ctx`; throws std::runtime_error with vslam_last_error.
void adjust_windows(vslam_ctx *ctx, f64 *d_R, f64 *d_T, const s32 *d_n_cams, int cam_stride, f64 *d_points, const s32 *d_n_points,
                    int pt_stride, const s32 *d_obs_offsets, const s32 *d_obs_cam, const float *d_obs_xy, int obs_stride, int batch,
                    const cv::Mat &K, f64 *d_stats = nullptr, const vslam_adjust_params *params = nullptr);

// Search by projection for a batch of items the caller holds on the device (vslam_search_projection, include/vslam_search.h: the
// arrays and strides are that call's): each item's points projected with its pose and matched to the frame's keypoints by
// descriptor inside a pixel window, one-to-one, compacted into the layout resect_poses reads.  K: 3 x 3 CV_32F; params:
// nullptr for the defaults; d_kp_taken, d_corr_point, d_corr_kp, d_stats may be nullptr.  Stream-ordered on `ctx`; throws
// std::runtime_error with vslam_last_error.
void search_projection(vslam_ctx *ctx, const float *d_points, const s32 *d_n_points, int pt_stride, const s32 *d_obs_offsets,
                       const unsigned char *d_obs_desc, int obs_stride, const f64 *d_R, const f64 *d_T, const cv::Mat &K, int width, int height,
                       const float *d_xy, const unsigned char *d_desc, const s32 *d_n_kp, int kp_stride, const s32 *d_kp_taken, int batch,
                       s32 *d_kp_of_point, s32 *d_dist, f64 *d_corr_points, float *d_corr_xy, s32 *d_corr_point, s32 *d_corr_kp,
                       s32 *d_n_corr, s32 *d_stats = nullptr, const vslam_search_params *params = nullptr);

// A pose without a prior for a batch of items the caller holds on the device (vslam_pnp_ransac, include/vslam_pnp.h: the arrays
// and strides are that call's): P3P RANSAC over each item's 3-D / 2-D correspondences, d_R / d_T written where an item is found,
// the winner's inliers compacted into the layout resect_poses reads.  K: 3 x 3 CV_32F; params: nullptr for the defaults; polish:
// nullptr for none; d_corr_index, d_counts, d_stats may be nullptr.  Stream-ordered on `ctx`; throws std::runtime_error with
// vslam_last_error.
void pnp_ransac(vslam_ctx *ctx, const f64 *d_points, const float *d_xy, const s32 *d_n, int batch, int stride, const cv::Mat &K,
                const unsigned int *d_seeds, f64 *d_R, f64 *d_T, s32 *d_inlier, f64 *d_corr_points, float *d_corr_xy, s32 *d_corr_index,
                s32 *d_n_inliers, s32 *d_winner, s32 *d_counts = nullptr, f64 *d_stats = nullptr, const vslam_pnp_params *params = nullptr,
                const vslam_resect_params *polish = nullptr);

// The similarity B = s R A + t between two views for a batch of items the caller holds on the device (vslam_sim3_ransac,
// include/vslam_sim3.h: the arrays and strides are that call's): 3-point RANSAC over each item's 3-D / 3-D correspondences with
// their keypoints in both images, d_scale / d_R / d_T written where an item is found.  K: 3 x 3 CV_32F, for both images; params:
// nullptr for the defaults; polish: nullptr for none; d_corr_index, d_counts, d_stats may be nullptr.  Stream-ordered on `ctx`;
// throws std::runtime_error with vslam_last_error.
void sim3_ransac(vslam_ctx *ctx, const f64 *d_A, const float *d_xa, const f64 *d_B, const float *d_xb, const s32 *d_n, int batch, int stride,
                 const cv::Mat &K, const unsigned int *d_seeds, f64 *d_scale, f64 *d_R, f64 *d_T, s32 *d_inlier, s32 *d_corr_index,
                 s32 *d_n_inliers, s32 *d_winner, s32 *d_counts = nullptr, f64 *d_stats = nullptr, const vslam_sim3_params *params = nullptr,
                 const vslam_resect_params *polish = nullptr);
// The 7-parameter polish alone (vslam_sim3_refine), d_scale / d_R / d_T in place over the correspondences i < n with d_mask[i] != 0
// (nullptr: all of them); params: nullptr for the defaults; d_stats may be nullptr.
void sim3_refine(vslam_ctx *ctx, const f64 *d_A, const float *d_xa, const f64 *d_B, const float *d_xb, const s32 *d_n, int batch, int stride,
                 const s32 *d_mask, const cv::Mat &K, f64 *d_scale, f64 *d_R, f64 *d_T, f64 *d_stats = nullptr,
                 const vslam_resect_params *params = nullptr);

// Pose graphs over Sim(3) for a batch of items the caller holds on the device (vslam_graph_optimize, include/vslam_graph.h: the
// arrays and strides are that call's), d_scale / d_R / d_T in place; params: nullptr for the defaults; d_stats may be nullptr.
// Stream-ordered on `ctx`; throws std::runtime_error with vslam_last_error.
void graph_optimize(vslam_ctx *ctx, f64 *d_scale, f64 *d_R, f64 *d_T, const s32 *d_fixed, const s32 *d_n_nodes, int batch, int node_stride,
                    const s32 *d_edge_ab, const f64 *d_edge_scale, const f64 *d_edge_R, const f64 *d_edge_T, const f64 *d_edge_weight,
                    const s32 *d_n_edges, int edge_stride, f64 *d_stats = nullptr, const vslam_graph_params *params = nullptr);

// Map points that share an observation grouped, their observation lists merged, for a batch of items the caller holds on the
// device (vslam_fuse_points, include/vslam_fuse.h: the arrays and strides are that call's).  d_mask, d_out_src and d_stats may be
// nullptr.  Stream-ordered on `ctx`; throws std::runtime_error with vslam_last_error.
void fuse_points(vslam_ctx *ctx, const s32 *d_n_points, int pt_stride, const s32 *d_obs_offsets, const s32 *d_obs_cam, const s32 *d_obs_kp,
                 int obs_stride, int cam_stride, int kp_stride, const s32 *d_mask, int batch, s32 *d_fuse_to, s32 *d_out_offsets,
                 s32 *d_out_cam, s32 *d_out_kp, s32 *d_out_src = nullptr, s32 *d_stats = nullptr);

// Which points of each item their observations support (vslam_cull_points, include/vslam_fuse.h: the arrays and strides are that
// call's).  K: 3 x 3 CV_32F; params: nullptr for the defaults; d_counts may be nullptr.  Stream-ordered on `ctx`; throws
// std::runtime_error with vslam_last_error.
void cull_points(vslam_ctx *ctx, const float *d_points, const s32 *d_n_points, int pt_stride, const s32 *d_obs_offsets, const s32 *d_obs_cam,
                 const s32 *d_obs_kp, int obs_stride, const f64 *d_R, const f64 *d_T, const s32 *d_n_cams, int cam_stride, const float *d_xy,
                 int kp_stride, const cv::Mat &K, int batch, s32 *d_keep, s32 *d_stats, s32 *d_counts = nullptr,
                 const vslam_cull_params *params = nullptr);

// Geometric fusing: every point of each item searched by projection in every camera that does not see it yet, one-to-one per
// keypoint, with the point that already holds the keypoint (vslam_fuse_project, include/vslam_fuse_project.h: the arrays and strides
// are that call's).  K: 3 x 3 CV_32F; params: nullptr for the defaults; d_cam_mask and d_stats may be nullptr.  Stream-ordered on
// `ctx`; throws std::runtime_error with vslam_last_error.
void fuse_project(vslam_ctx *ctx, const float *d_points, const s32 *d_n_points, int pt_stride, const s32 *d_obs_offsets, const s32 *d_obs_cam,
                  const s32 *d_obs_kp, const u8 *d_obs_desc, int obs_stride, const f64 *d_R, const f64 *d_T, const s32 *d_n_cams, int cam_stride,
                  const float *d_xy, const u8 *d_desc, const s32 *d_n_kp, int kp_stride, const s32 *d_cam_mask, const cv::Mat &K, int width,
                  int height, int batch, s32 *d_found_point, s32 *d_found_cam, s32 *d_found_kp, s32 *d_found_dist, s32 *d_found_holder,
                  int found_stride, s32 *d_n_found, s32 *d_stats = nullptr, const vslam_search_params *params = nullptr);

// Each point of each item triangulated from all its observations (vslam_triangulate_tracks, include/vslam_tracks.h: the arrays and
// strides are that call's; d_out_points may be d_points).  K: 3 x 3 CV_32F; params: nullptr for the defaults; d_counts and d_info may
// be nullptr.  Stream-ordered on `ctx`; throws std::runtime_error with vslam_last_error.
void triangulate_tracks(vslam_ctx *ctx, const float *d_points, const s32 *d_n_points, int pt_stride, const s32 *d_obs_offsets,
                        const s32 *d_obs_cam, const s32 *d_obs_kp, int obs_stride, const f64 *d_R, const f64 *d_T, const s32 *d_n_cams,
                        int cam_stride, const float *d_xy, int kp_stride, const cv::Mat &K, int batch, float *d_out_points, s32 *d_status,
                        s32 *d_stats, s32 *d_counts = nullptr, f64 *d_info = nullptr, const vslam_track_params *params = nullptr);

// The nearest word of a vocabulary for every descriptor of a batch of frames the caller holds on the device (vslam_places_assign,
// include/vslam_places.h: the arrays and strides are that call's).  d_dist may be nullptr.  Stream-ordered on `ctx`; throws
// std::runtime_error with vslam_last_error.
void places_assign(vslam_ctx *ctx, const unsigned char *d_desc, const s32 *d_n, int kp_stride, int frames, const unsigned char *d_vocab,
                   int n_words, s32 *d_word, s32 *d_dist = nullptr);

// A vocabulary of n_words words by k-majority from n descriptors (vslam_places_train, include/vslam_places.h).  Stream-ordered on
// `ctx`; throws std::runtime_error with vslam_last_error.
void places_train(vslam_ctx *ctx, const unsigned char *d_desc, int n, int n_words, int iterations, unsigned char *d_vocab, s32 *d_sizes);

// A vslam_places (include/vslam_places.h: an index of frames as bags of binary words) held for a scope: made by the constructor,
// destroyed with the object, which must go before its context.  Every member is that header's call of the same name on device
// arrays, stream-ordered on the context, and throws std::runtime_error with vslam_last_error.  Not copyable.
class Places {
public:
    Places(vslam_ctx *ctx, int n_words, int capacity, int max_kp);
    ~Places();
    Places(const Places &) = delete;
    Places &operator=(const Places &) = delete;
    void reset();
    void set_vocabulary(const unsigned char *d_vocab, const s32 *d_weights = nullptr);
    void set_weights(const s32 *d_weights);
    void add(const unsigned char *d_desc, const s32 *d_n, int kp_stride, int frames, const s32 *d_tags, s32 *d_ids);
    void query(const unsigned char *d_desc, const s32 *d_n, int kp_stride, int queries, const s32 *d_below, int top_k, s32 *d_best_id,
               s32 *d_best_score, s32 *d_best_den, s32 *d_q_norm);
    vslam_places_arrays view();
    vslam_places *handle() const { return idx_; }

private:
    vslam_ctx *ctx_;
    vslam_places *idx_ = nullptr;
};

// The map-association block of the capture loop (src/vslam.cpp:129-161 with orb_distance, src/PointMap.cpp:36-46) in one
// device call -- what radius_search_batch is to a single radius_search.  map_points: N x 4 CV_32F rows (x, y, z, 1)
// (pm.points.rowRange(0, pm.size)); c2: 3 x 4.  Map point i is projected, dropped unless it lands inside [0, W) x [0, H),
// searched for in frame.kdtree with `radius` (2 in the reference), and given the FIRST hit in radius_search's order whose
// map_point_ids entry is still < 0 and whose descriptor is closer than dist_threshold (DISTANCE_THRESHOLD, 64) to one of the
// map point's observations; lower map indices claim first, as in the sequential loop.  The observations of map point i are
// rows obs_offsets[i] .. obs_offsets[i + 1] - 1 of obs_desc (M x 32 CV_8U): the descriptors
// pm.frames[pm.frame_ids[i][k]].descriptors.row(pm.frame_point_ids[i][k]) in k order.
// frame.map_point_ids is updated in place (:155); the return value holds, per map point, the keypoint it claimed or -1 -- the
// caller appends frame.id / that index to pm.frame_ids[i] / pm.frame_point_ids[i] (:156-157).
std::vector<s32> associate_map_points(Frame &frame, const cv::Mat &map_points, const cv::Mat &c2, int W, int H,
                                      const std::vector<u32> &obs_offsets, const cv::Mat &obs_desc, float radius = 2.f,
                                      u32 dist_threshold = 64);
}  // namespace vslam
