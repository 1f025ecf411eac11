// Drop-in for the reference's include/PointMap.h: the same struct and the same two free functions, with the map itself kept
// on the MI355X -- a one-track vslam_map (include/vslam_amd.h) behind the struct, advanced by vslam::map_step and copied into
// the host-side members by sync_to_host().
#pragma once
#include <memory>
#include <utility>
#include <vector>

#include "Frame.h"
#include "cvlite.h"
#include "vslam_internal.h"

#ifndef VSLAM_HAVE_OPENCV
namespace cv {
template <typename T>
struct Point3_ {
    T x, y, z;
    Point3_() : x(0), y(0), z(0) {}
    Point3_(T x_, T y_, T z_) : x(x_), y(y_), z(z_) {}
    bool operator==(const Point3_ &o) const { return x == o.x && y == o.y && z == o.z; }
};
}  // namespace cv
#endif

namespace vslam {
struct DeviceMap;   // the vslam_map and its staging buffers
}

struct PointMap {   // reference: include/PointMap.h:10-21
    usize size = 0;
    usize capacity = 0;

    cv::Mat points;   // size x 4 CV_32F rows (x, y, z, 1)
    std::vector<std::vector<usize>> frame_ids;
    std::vector<std::vector<usize>> frame_point_ids;
    std::vector<cv::Point3_<u8>> colors;

    std::vector<Frame> frames;

    // The device map behind the struct (vslam::map_create).  sync_to_host() waits for the device and fills size, capacity,
    // points, frame_ids, frame_point_ids (the reference's push order), colors and every recorded frame's map_point_ids,
    // R_t and pose from it.
    std::shared_ptr<vslam::DeviceMap> device;
    void sync_to_host();

    // The world frame beside the map (vslam::map_attach_world; include/vslam_amd.h, "the world frame"), as of the last
    // sync_to_host(): the map's points in the coordinates of frame 0 (size x 4 CV_32F rows (x, y, z, 1), row i = points row i
    // lifted) and one camera -> world pose per recorded frame (4 x 4 CV_32F).  Empty without an attached world.
    const cv::Mat &world_points() const { return world_points_; }
    const std::vector<cv::Mat> &world_poses() const { return world_poses_; }
    cv::Mat world_points_;
    std::vector<cv::Mat> world_poses_;
};

// reference: include/PointMap.h:23, src/PointMap.cpp:3-34 -- on the host-side members, as the reference writes it (a caller
// that keeps the loop on the host; the device map is advanced by vslam::map_step instead, which appends the same points).
void add_reprojection_inliers(PointMap &pm, const cv::Mat &points_4d, const std::vector<usize> &reprojection_inliers,
                              const std::vector<cv::Point3_<u8>> &colors, u64 last_frame_id, u64 frame_id,
                              const std::vector<std::pair<int, int>> &matches);
// reference: include/PointMap.h:24, src/PointMap.cpp:36-46 -- min Hamming distance over the map point's observations, on the
// host-side members (valid after sync_to_host()).
u32 orb_distance(const PointMap &pm, usize map_point_id, const Frame &frame, usize frame_point_id);

namespace vslam {
// Gives pm its device map: room for max_frames frames of up to kp_stride keypoints, map_capacity points, obs_capacity
// observations (fixed; exceeding one makes map_step throw and leaves the map as it was).
void map_create(PointMap &pm, int max_frames, int kp_stride, int map_capacity, int obs_capacity);
// One iteration of src/vslam.cpp:69-262 on the device for frame = pm.frames.back() against the frame before it (both with
// features extracted), given match_features' outputs: R_t / pose, propagation of map_point_ids, association (radius,
// dist_threshold), triangulation, the reprojection filter (threshold_sq) and the new map points with their colours.
// An empty `fundamental` (RANSAC accepted nothing) leaves the map untouched, as vslam_map_step documents.
void map_step(PointMap &pm, const std::vector<std::pair<int, int>> &matches, const cv::Mat &fundamental, const cv::Mat &K,
              float radius = 2.f, u32 dist_threshold = 64, float threshold_sq = 4.f);
// Gives pm's device map a world frame (a vslam::World of its shape, include/vslam/World.h): every map_step from now on advances
// it and lifts the new points; sync_to_host() fills world_points() / world_poses().  Before the first map_step.
void map_attach_world(PointMap &pm, int min_links = 8);
}  // namespace vslam
