// Uses the drop-in include/vslam/Display.h the way the reference's main loop feeds its window (src/vslam.cpp:264-276), headless:
//   1. a Display whose `ds` points at host-side points / colours / frames read from the input, drawn once with render();
//   2. the reference's loop through PointMap.h as in pointmap_demo.cpp, then vslam::render_map of the DEVICE map, and
//      sync_to_host() so that the Python test can draw the same arrays itself.
//
// usage: display_demo <in.bin> <out.bin>
//   in.bin : int32 W, H; vslam_view (raw bytes); int32 n; n x 4 f32; n x 3 u8; int32 frames; frames x 16 f32;
//            int32 w, h, max_corners, hyp, nf; uint32 seeds[nf - 1]; nf BGR frames
//   out.bin: W x H x 3 image of 1;  W x H x 3 image of 2;  int32 size; size x 4 f32; size x 3 u8; int32 nf; nf x 16 f32 poses
#include <cstdio>
#include <mutex>
#include <vector>

#include "vslam/Display.h"
#include "vslam/Frame.h"
#include "vslam/PointMap.h"

static void wr(FILE *f, const void *p, size_t n) { fwrite(p, 1, n, f); }
static void wr_i(FILE *f, int v) { wr(f, &v, 4); }
static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    int WH[2], n = 0, nfr = 0;
    vslam_view view;
    if (!fi || !rd(fi, WH, 8) || !rd(fi, &view, sizeof(view)) || !rd(fi, &n, 4)) return 3;
    const int W = WH[0], H = WH[1];
    cv::Mat points(n, 4, CV_32FC1);
    std::vector<unsigned char> col(3 * (size_t)n);
    if (!rd(fi, points.ptr<float>(0), 16 * (size_t)n) || !rd(fi, col.data(), col.size()) || !rd(fi, &nfr, 4)) return 3;
    std::vector<cv::Point3_<u8>> colors;
    for (int i = 0; i < n; i++) colors.emplace_back(col[3 * i], col[3 * i + 1], col[3 * i + 2]);
    std::vector<Frame> frames(nfr);
    for (Frame &f : frames) {
        f.kdtree.root = nullptr;
        f.pose.create(4, 4, CV_32FC1);
        if (!rd(fi, f.pose.ptr<float>(0), 64)) return 3;
    }
    int hdr[5];
    if (!rd(fi, hdr, 20)) return 3;
    const int w = hdr[0], h = hdr[1], maxc = hdr[2], hyp = hdr[3], nf = hdr[4];
    std::vector<unsigned> seeds(nf - 1);
    if (!rd(fi, seeds.data(), 4 * seeds.size())) return 3;
    std::vector<std::vector<unsigned char>> img(nf);
    for (auto &b : img) {
        b.resize((size_t)w * h * 3);
        if (!rd(fi, b.data(), b.size())) return 3;
    }
    fclose(fi);
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 6;

    // 1. the producer end of src/vslam.cpp:272-275
    std::mutex mtx;
    Display display("map", W, H, &mtx);
    display.initialize();
    display.view = view;
    mtx.lock();
    display.ds.points = &points;
    display.ds.colors = &colors;
    display.ds.size = (usize)n;
    display.ds.frames = &frames;
    mtx.unlock();
    cv::Mat shot;
    display.render(shot);
    if (shot.rows != H || shot.cols != W) return 7;
    for (int r = 0; r < H; r++) wr(fo, shot.ptr<unsigned char>(r), (size_t)3 * W);
    display.close();
    display.join();

    // 2. a map that lives on the device
    vslam::settings().max_corners = maxc;
    const float kv[9] = {525.f, 0, (float)(w / 2), 0, 525.f, (float)(h / 2), 0, 0, 1};   // src/vslam.cpp:32
    cv::Mat K(3, 3, CV_32FC1);
    for (int i = 0; i < 9; i++) K.ptr<float>(i / 3)[i % 3] = kv[i];
    PointMap pm;
    vslam::map_create(pm, nf, maxc, nf * maxc, 4 * nf * maxc);
    pm.frames.reserve(nf);
    for (int i = 0; i < nf; i++) {
        pm.frames.emplace_back();
        Frame &frame = pm.frames.back();
        frame.kdtree.root = nullptr;
        cv::Mat image(h, w, CV_8UC3, img[i].data());
        initialize_frame(frame, image, i);
        extract_features(frame);
        if (i == 0) continue;
        RansacFilter rf(8, hyp, 10);
        rf.set_seed(seeds[i - 1]);
        std::vector<std::pair<int, int>> matches;
        cv::Mat fundamental;
        match_features(pm.frames[i - 1], frame, rf, matches, fundamental);
        vslam::map_step(pm, matches, fundamental, K);
    }
    cv::Mat seen = vslam::render_map(pm, view, W, H);
    for (int r = 0; r < H; r++) wr(fo, seen.ptr<unsigned char>(r), (size_t)3 * W);
    pm.sync_to_host();
    wr_i(fo, (int)pm.size);
    for (usize i = 0; i < pm.size; i++) wr(fo, pm.points.ptr<float>((int)i), 16);
    for (usize i = 0; i < pm.size; i++) {
        const unsigned char c[3] = {pm.colors[i].x, pm.colors[i].y, pm.colors[i].z};
        wr(fo, c, 3);
    }
    wr_i(fo, nf);
    for (int f = 0; f < nf; f++) wr(fo, pm.frames[f].pose.ptr<float>(0), 64);
    fclose(fo);
    return 0;
}
