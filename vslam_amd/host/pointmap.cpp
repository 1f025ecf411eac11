// include/vslam/PointMap.h over the C ABI's resident map (vslam_map_*), one track.
#include <cstring>
#include <stdexcept>

#include "../../include/vslam/PointMap.h"
#include "../../include/vslam/World.h"
#include "host_internal.h"

using vslam::detail::check;
using vslam::detail::context;

namespace vslam {
struct DeviceMap {
    vslam_map *map = nullptr;
    std::unique_ptr<World> world;   // vslam::map_attach_world; destroyed after the map
    int max_frames = 0, kp_stride = 0, map_capacity = 0, obs_capacity = 0;
    int recorded = 0;   // id of the last frame stepped (0: only the first frame so far)
    // one frame step's inputs: features of two frames (ping-pong), the pair's outputs, the image
    float *xy[2] = {nullptr, nullptr};
    uint8_t *desc[2] = {nullptr, nullptr};
    int32_t *n[2] = {nullptr, nullptr};
    int32_t *nodes = nullptr, *matches = nullptr, *best = nullptr;
    float *F = nullptr;
    uint8_t *image = nullptr;
    size_t image_bytes = 0;
    int32_t *offsets = nullptr, *obs_frames = nullptr, *obs_points = nullptr;
    std::vector<void *> owned;

    template <typename T>
    void alloc(T **p, size_t count) {
        void *d = nullptr;
        check(vslam_dev_alloc(context(), sizeof(T) * (count ? count : 1), &d), "PointMap: device memory");
        owned.push_back(d);
        *p = static_cast<T *>(d);
    }
    ~DeviceMap() {
        if (map) vslam_map_destroy(map);
        world.reset();
        for (void *d : owned) vslam_dev_free(context(), d);
        if (image) vslam_dev_free(context(), image);
    }
    void upload_frame(const Frame &fr, int slot, bool with_tree) {
        const int cnt = (int)fr.points.size();
        if (cnt > kp_stride) throw std::invalid_argument("PointMap: a frame has more keypoints than the map's kp_stride");
        if (fr.descriptors.rows < cnt || (cnt > 0 && fr.descriptors.cols != VSLAM_DESC_BYTES))
            throw std::invalid_argument("PointMap: frame.descriptors does not cover frame.points");
        std::vector<float> pts(2 * (size_t)kp_stride, 0.f);
        std::vector<uint8_t> d((size_t)kp_stride * VSLAM_DESC_BYTES, 0);
        for (int i = 0; i < cnt; i++) {
            pts[2 * i] = fr.points[i].x;
            pts[2 * i + 1] = fr.points[i].y;
            std::memcpy(d.data() + (size_t)i * VSLAM_DESC_BYTES, fr.descriptors.ptr<uint8_t>(i), VSLAM_DESC_BYTES);
        }
        const int32_t c = cnt;
        check(vslam_copy_h2d(context(), xy[slot], pts.data(), sizeof(float) * pts.size()), "PointMap: upload");
        check(vslam_copy_h2d(context(), desc[slot], d.data(), d.size()), "PointMap: upload");
        check(vslam_copy_h2d(context(), n[slot], &c, sizeof(c)), "PointMap: upload");
        if (with_tree) {
            std::vector<int32_t> pre((size_t)kp_stride, -1);
            if (cnt > 0 && fr.kdtree.root == nullptr) throw std::invalid_argument("PointMap: the frame has no k-d tree");
            for (int i = 0; i < cnt; i++) pre[i] = (int32_t)fr.kdtree.root[i].pt_index;   // the node array is in pre-order
            check(vslam_copy_h2d(context(), nodes, pre.data(), sizeof(int32_t) * pre.size()), "PointMap: upload");
        }
    }
};

void map_create(PointMap &pm, int max_frames, int kp_stride, int map_capacity, int obs_capacity) {
    auto d = std::make_shared<DeviceMap>();
    d->max_frames = max_frames; d->kp_stride = kp_stride; d->map_capacity = map_capacity; d->obs_capacity = obs_capacity;
    check(vslam_map_create(context(), 1, max_frames, kp_stride, map_capacity, obs_capacity, &d->map), "vslam_map_create");
    const size_t K = (size_t)kp_stride;
    for (int s = 0; s < 2; s++) {
        d->alloc(&d->xy[s], 2 * K);
        d->alloc(&d->desc[s], K * VSLAM_DESC_BYTES);
        d->alloc(&d->n[s], 1);
    }
    d->alloc(&d->nodes, K);
    d->alloc(&d->matches, 2 * K);
    d->alloc(&d->best, 4);
    d->alloc(&d->F, 9);
    d->alloc(&d->offsets, (size_t)map_capacity + 1);
    d->alloc(&d->obs_frames, (size_t)obs_capacity);
    d->alloc(&d->obs_points, (size_t)obs_capacity);
    pm.device = d;
    pm.capacity = (usize)map_capacity;
}

void map_step(PointMap &pm, const std::vector<std::pair<int, int>> &matches, const cv::Mat &fundamental, const cv::Mat &K,
              float radius, u32 dist_threshold, float threshold_sq) {
    if (!pm.device) throw std::logic_error("PointMap: vslam::map_create first");
    DeviceMap &d = *pm.device;
    const int fid = (int)pm.frames.size() - 1;
    if (fid < 1) throw std::logic_error("PointMap: map_step needs two frames in pm.frames");
    if (d.recorded != fid - 1) throw std::logic_error("PointMap: one map_step per frame, in order");
    if (fid == 1) d.upload_frame(pm.frames[0], 0, false);   // later steps find the last frame's features where its own step left them
    const Frame &frame = pm.frames[fid];
    d.upload_frame(frame, fid & 1, true);
    const int k = (int)matches.size();
    if (k > d.kp_stride) throw std::invalid_argument("PointMap: more matches than the map's kp_stride");
    std::vector<int32_t> m(2 * (size_t)d.kp_stride, 0);
    for (int i = 0; i < k; i++) {
        m[2 * i] = matches[i].first;
        m[2 * i + 1] = matches[i].second;
    }
    const bool has_model = !fundamental.empty();
    const int32_t best[4] = {has_model ? 0 : -1, k, 0, k};
    float Fh[9] = {0}, Kh[9];
    for (int i = 0; i < 9; i++) {
        if (has_model) Fh[i] = fundamental.ptr<float>(i / 3)[i % 3];
        Kh[i] = K.ptr<float>(i / 3)[i % 3];
    }
    check(vslam_copy_h2d(context(), d.matches, m.data(), sizeof(int32_t) * m.size()), "PointMap: upload");
    check(vslam_copy_h2d(context(), d.best, best, sizeof(best)), "PointMap: upload");
    check(vslam_copy_h2d(context(), d.F, Fh, sizeof(Fh)), "PointMap: upload");
    const cv::Mat &img = frame.image;
    if (img.empty() || img.type() != CV_8UC3) throw std::invalid_argument("PointMap: frame.image must be CV_8UC3");
    const size_t row = (size_t)img.cols * 3, bytes = row * img.rows;
    if (bytes > d.image_bytes) {
        if (d.image) vslam_dev_free(context(), d.image);
        void *p = nullptr;
        check(vslam_dev_alloc(context(), bytes, &p), "PointMap: device memory");
        d.image = static_cast<uint8_t *>(p);
        d.image_bytes = bytes;
    }
    std::vector<uint8_t> packed(bytes);
    for (int r = 0; r < img.rows; r++) std::memcpy(packed.data() + row * r, img.ptr<uint8_t>(r), row);
    check(vslam_copy_h2d(context(), d.image, packed.data(), bytes), "PointMap: upload");
    const int cur = fid & 1, last = cur ^ 1;
    check(vslam_map_step(context(), d.map, d.xy[last], d.desc[last], d.n[last], d.xy[cur], d.desc[cur], d.nodes, d.n[cur],
                         d.matches, d.best, d.F, d.image, img.cols, img.rows, (int)row, Kh, radius, dist_threshold, threshold_sq),
          "vslam_map_step");
    d.recorded = fid;
    check(vslam_ctx_synchronize(context()), "PointMap: map_step (a capacity of the map, or more than 16 acceptable hits)");
}

void map_attach_world(PointMap &pm, int min_links) {
    if (!pm.device) throw std::logic_error("PointMap: vslam::map_create first");
    DeviceMap &d = *pm.device;
    if (d.world) throw std::logic_error("PointMap: a world is attached already");
    d.world.reset(new World(context(), 1, d.max_frames, d.kp_stride, min_links));
    d.world->attach_to(d.map);
}

namespace detail {
vslam_map *device_map(PointMap &pm) {
    if (!pm.device) throw std::logic_error("PointMap: vslam::map_create first");
    return pm.device->map;
}
}  // namespace detail
}  // namespace vslam

void PointMap::sync_to_host() {
    if (!device) throw std::logic_error("PointMap: vslam::map_create first");
    vslam::DeviceMap &d = *device;
    vslam_map_arrays a;
    check(vslam_map_view(d.map, &a), "vslam_map_view");
    check(vslam_map_observations(context(), d.map, d.offsets, d.obs_frames, d.obs_points), "vslam_map_observations");
    check(vslam_ctx_wait(context()), "vslam_ctx_wait");
    int32_t sz = 0, total = 0;
    check(vslam_copy_d2h(context(), &sz, a.d_sizes, sizeof(sz)), "copy_d2h");
    check(vslam_copy_d2h(context(), &total, a.d_n_obs, sizeof(total)), "copy_d2h");
    size = (usize)sz;
    capacity = (usize)d.map_capacity;
    points.create(sz, 4, CV_32FC1);
    std::vector<uint8_t> col(3 * (size_t)sz + 1);
    std::vector<int32_t> off((size_t)sz + 1, 0), fr((size_t)total + 1), pt((size_t)total + 1);
    if (sz > 0) {
        check(vslam_copy_d2h(context(), points.ptr<float>(0), a.d_points, sizeof(float) * 4 * (size_t)sz), "copy_d2h");
        check(vslam_copy_d2h(context(), col.data(), a.d_colors, 3 * (size_t)sz), "copy_d2h");
        check(vslam_copy_d2h(context(), off.data(), d.offsets, sizeof(int32_t) * ((size_t)sz + 1)), "copy_d2h");
    }
    if (total > 0) {
        check(vslam_copy_d2h(context(), fr.data(), d.obs_frames, sizeof(int32_t) * (size_t)total), "copy_d2h");
        check(vslam_copy_d2h(context(), pt.data(), d.obs_points, sizeof(int32_t) * (size_t)total), "copy_d2h");
    }
    colors.assign((size_t)sz, cv::Point3_<u8>());
    frame_ids.assign((size_t)sz, {});
    frame_point_ids.assign((size_t)sz, {});
    for (int i = 0; i < sz; i++) {
        colors[i] = cv::Point3_<u8>(col[3 * i], col[3 * i + 1], col[3 * i + 2]);
        for (int o = off[i]; o < off[i + 1]; o++) {
            frame_ids[i].push_back((usize)fr[o]);
            frame_point_ids[i].push_back((usize)pt[o]);
        }
    }
    const int nf = std::min<int>((int)frames.size(), std::min(a.frames, d.max_frames));
    std::vector<int32_t> ids((size_t)d.kp_stride);
    for (int f = 0; f < nf; f++) {
        Frame &frm = frames[f];
        check(vslam_copy_d2h(context(), ids.data(), a.d_map_point_ids + (size_t)f * d.kp_stride, sizeof(int32_t) * ids.size()),
              "copy_d2h");
        frm.map_point_ids.assign(ids.begin(), ids.begin() + std::min<size_t>(ids.size(), frm.points.size()));
        frm.R_t.create(4, 4, CV_32FC1);
        frm.pose.create(4, 4, CV_32FC1);
        check(vslam_copy_d2h(context(), frm.R_t.ptr<float>(0), a.d_R_t + (size_t)f * 16, sizeof(float) * 16), "copy_d2h");
        check(vslam_copy_d2h(context(), frm.pose.ptr<float>(0), a.d_pose + (size_t)f * 16, sizeof(float) * 16), "copy_d2h");
    }
    world_points_ = cv::Mat();
    world_poses_.clear();
    if (d.world) {
        const vslam_world_arrays w = d.world->view();
        world_points_.create(sz, 4, CV_32FC1);
        if (sz > 0) check(vslam_copy_d2h(context(), world_points_.ptr<float>(0), w.d_world_points, sizeof(float) * 4 * (size_t)sz), "copy_d2h");
        for (int f = 0; f < std::min<int>(w.frames, w.max_frames); f++) {
            cv::Mat pose4(4, 4, CV_32FC1);
            check(vslam_copy_d2h(context(), pose4.ptr<float>(0), w.d_pose + (size_t)f * 16, sizeof(float) * 16), "copy_d2h");
            world_poses_.push_back(pose4);
        }
    }
}

// reference: src/PointMap.cpp:3-34
void add_reprojection_inliers(PointMap &pm, const cv::Mat &points_4d, const std::vector<usize> &reprojection_inliers,
                              const std::vector<cv::Point3_<u8>> &colors, u64 last_frame_id, u64 frame_id,
                              const std::vector<std::pair<int, int>> &matches) {
    const usize num_new_points = reprojection_inliers.size();
    cv::Mat grown((int)(pm.size + num_new_points), 4, CV_32FC1);
    for (usize r = 0; r < pm.size; r++) std::memcpy(grown.ptr<float>((int)r), pm.points.ptr<float>((int)r), sizeof(float) * 4);
    pm.colors.insert(pm.colors.end(), colors.begin(), colors.end());
    usize j = pm.size;
    for (usize row : reprojection_inliers) {
        float *dst = grown.ptr<float>((int)j++);
        const float *src = points_4d.ptr<float>((int)row);
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
        dst[3] = 1;
        pm.frame_point_ids.push_back({static_cast<usize>(matches[row].first), static_cast<usize>(matches[row].second)});
    }
    pm.points = grown;
    pm.size += num_new_points;
    if (pm.capacity < pm.size) pm.capacity = pm.size;
    pm.frame_ids.resize(pm.size, {static_cast<usize>(last_frame_id), static_cast<usize>(frame_id)});
}

// reference: src/PointMap.cpp:36-46
u32 orb_distance(const PointMap &pm, usize map_point_id, const Frame &frame, usize frame_point_id) {
    u32 min = u32_max;
    const std::vector<usize> &frame_ids = pm.frame_ids[map_point_id];
    const std::vector<usize> &frame_point_ids = pm.frame_point_ids[map_point_id];
    const u8 *a = frame.descriptors.ptr<u8>((int)frame_point_id);
    for (usize i = 0; i < frame_ids.size(); i++) {
        const u8 *b = pm.frames[frame_ids[i]].descriptors.ptr<u8>((int)frame_point_ids[i]);
        u32 curr = 0;
        for (int k = 0; k < VSLAM_DESC_BYTES; k++) curr += (u32)__builtin_popcount((unsigned)(a[k] ^ b[k]));
        if (curr < min) min = curr;
    }
    return min;
}
