// include/vslam/Display.h over the C ABI's renderer (vslam_render_points).
#include <cstring>
#include <stdexcept>

#include "../../include/vslam/Display.h"
#include "host_internal.h"

using vslam::detail::check;
using vslam::detail::context;

namespace {
struct DevBuf {   // freed on every path out of render()
    void *p = nullptr;
    explicit DevBuf(size_t bytes) { check(vslam_dev_alloc(context(), bytes ? bytes : 1, &p), "Display: device memory"); }
    ~DevBuf() { vslam_dev_free(context(), p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};
}  // namespace

Display::Display(const char *window_name, const int W, const int H, std::mutex *mtx) : mtx(mtx), window_name(window_name), W(W), H(H) {
    if (vslam_view_default(W, H, &view) != VSLAM_OK) throw std::invalid_argument("Display: W and H must be positive");
}

void Display::render(cv::Mat &bgr_out) {
    std::vector<float> pts;
    std::vector<uint8_t> col;
    std::vector<float> poses;
    int32_t n = 0;
    int frames = 0;
    {
        std::unique_lock<std::mutex> lk;
        if (mtx) lk = std::unique_lock<std::mutex>(*mtx);
        if (ds.points != NULL && ds.size > 0) {
            const cv::Mat &P = *ds.points;
            if (!P.isContinuous() || P.cols != 4 || (usize)P.rows < ds.size || P.type() != CV_32FC1)
                throw std::invalid_argument("Display: ds.points must be a continuous N x 4 CV_32F matrix with N >= ds.size");
            n = (int32_t)ds.size;
            pts.assign(P.ptr<float>(0), P.ptr<float>(0) + 4 * (size_t)n);
            col.assign(3 * (size_t)n, 0);
            const size_t have = ds.colors ? std::min<size_t>(ds.colors->size(), (size_t)n) : 0;
            for (size_t i = 0; i < have; i++) {
                col[3 * i] = (*ds.colors)[i].x;
                col[3 * i + 1] = (*ds.colors)[i].y;
                col[3 * i + 2] = (*ds.colors)[i].z;
            }
        }
        if (ds.frames != NULL)
            for (const Frame &f : *ds.frames) {
                if (f.pose.empty() || !f.pose.isContinuous() || f.pose.rows != 4 || f.pose.cols != 4 || f.pose.type() != CV_32FC1) continue;
                poses.insert(poses.end(), f.pose.ptr<float>(0), f.pose.ptr<float>(0) + 16);
                frames++;
            }
    }
    const int cap = n > 0 ? n : 1;
    pts.resize(4 * (size_t)cap, 0.f);
    col.resize(3 * (size_t)cap, 0);
    const size_t image = (size_t)W * H * 3;
    DevBuf d_pts(sizeof(float) * pts.size()), d_col(col.size()), d_n(sizeof(n)), d_pose(sizeof(float) * poses.size()), d_img(image);
    check(vslam_copy_h2d(context(), d_pts.p, pts.data(), sizeof(float) * pts.size()), "Display: upload");
    check(vslam_copy_h2d(context(), d_col.p, col.data(), col.size()), "Display: upload");
    check(vslam_copy_h2d(context(), d_n.p, &n, sizeof(n)), "Display: upload");
    if (frames) check(vslam_copy_h2d(context(), d_pose.p, poses.data(), sizeof(float) * poses.size()), "Display: upload");
    check(vslam_render_points(context(), static_cast<const float *>(d_pts.p), static_cast<const uint8_t *>(d_col.p),
                              static_cast<const int32_t *>(d_n.p), 1, cap, frames ? static_cast<const float *>(d_pose.p) : nullptr, frames,
                              frames, &view, W, H, 3 * W, static_cast<uint8_t *>(d_img.p), nullptr),
          "vslam_render_points");
    check(vslam_ctx_wait(context()), "vslam_ctx_wait");
    bgr_out.create(H, W, CV_8UC3);
    if (bgr_out.isContinuous()) {
        check(vslam_copy_d2h(context(), bgr_out.ptr<uint8_t>(0), d_img.p, image), "Display: download");
    } else {
        std::vector<uint8_t> packed(image);
        check(vslam_copy_d2h(context(), packed.data(), d_img.p, image), "Display: download");
        for (int r = 0; r < H; r++) std::memcpy(bgr_out.ptr<uint8_t>(r), packed.data() + (size_t)3 * W * r, (size_t)3 * W);
    }
}

namespace vslam {
cv::Mat render_map(PointMap &pm, const vslam_view &view, int W, int H) {
    vslam_map *map = detail::device_map(pm);
    if (W <= 0 || H <= 0) throw std::invalid_argument("render_map: W and H must be positive");
    const size_t image = (size_t)W * H * 3;
    DevBuf d_img(image);
    check(vslam_map_render(context(), map, 0, 1, &view, W, H, 3 * W, static_cast<uint8_t *>(d_img.p), nullptr), "vslam_map_render");
    check(vslam_ctx_wait(context()), "vslam_ctx_wait");
    cv::Mat out(H, W, CV_8UC3);   // freshly made: continuous
    check(vslam_copy_d2h(context(), out.ptr<uint8_t>(0), d_img.p, image), "render_map: download");
    return out;
}
}  // namespace vslam
