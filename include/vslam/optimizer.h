// The header src/optimzer.cpp includes and the reference never wrote: its `struct optimizer` is three empty members,
// initial_poses, landmark_priors, measurements, the inputs of a bundle adjustment.  Here they hold the two-view problem that is
// consistent in the reference's own frames (one fixed camera [K | 0], one free camera K [R | t], the pair's points in the first
// camera's coordinates), and optimize() runs it on the device (vslam_refine_pairs, include/vslam_amd.h).
#pragma once

#include <utility>
#include <vector>

#include "cvlite.h"
#include "vslam_internal.h"

struct optimizer {
    // [0] the fixed camera, [I | 0] (3 x 4 CV_32F; not read: the first camera is the frame of the landmarks);
    // [1] the free camera [R | t] as extract_Rt left it
    std::vector<cv::Mat> initial_poses;
    // n x 4 CV_32F rows (x, y, z, 1) as triangulate() returns them, landmark i seen in measurements[i]
    cv::Mat landmark_priors;
    // landmark i's keypoint in the first and in the second image
    std::vector<std::pair<cv::Point2f, cv::Point2f>> measurements;

    // addition (the reference declares no method): the two-view bundle adjustment of initial_poses[1] and landmark_priors
    // over `measurements`, written back IN PLACE; K 3 x 3 CV_32F.  Landmarks that do not take part (not finite, behind a camera,
    // reprojection error above gate_sq in an image) keep their values, and so does everything when the problem is left alone
    // (fewer than 8 landmarks take part, no step lowers the error).  stats: nullptr or 4 doubles as d_stats holds them.
    // Throws std::invalid_argument on shapes that do not fit, std::runtime_error on a device error.
    void optimize(const cv::Mat &K, float gate_sq = 16.f, int max_iterations = 20, f64 *stats = nullptr);
};
