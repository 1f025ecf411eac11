// Uses the drop-in include/vslam/PointMap.h the way the reference's main loop uses PointMap (src/vslam.cpp:53-262): per frame
// initialize_frame + extract_features, match_features against the previous frame, then the whole map iteration on the device
// (vslam::map_step); at the end sync_to_host() and a dump of the host-side vectors for the Python test to hold to the model.
//
// usage: pointmap_demo <in.bin> <out.bin>    in.bin: int32 w, h, max_corners, hyp, frames; uint32 seeds[frames - 1]; BGR frames
#include <cstdio>
#include <vector>

#include "vslam/Frame.h"
#include "vslam/PointMap.h"

static void wr(FILE *f, const void *p, size_t n) { fwrite(p, 1, n, f); }
static void wr_i(FILE *f, int v) { wr(f, &v, 4); }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    int hdr[5];
    if (!fi || fread(hdr, 4, 5, fi) != 5) return 3;
    const int w = hdr[0], h = hdr[1], maxc = hdr[2], hyp = hdr[3], nf = hdr[4];
    std::vector<unsigned> seeds(nf - 1);
    if (fread(seeds.data(), 4, seeds.size(), fi) != seeds.size()) return 3;
    std::vector<std::vector<unsigned char>> img(nf);
    for (auto &b : img) {
        b.resize((size_t)w * h * 3);
        if (fread(b.data(), 1, b.size(), fi) != b.size()) return 3;
    }
    fclose(fi);
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
    pm.sync_to_host();

    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 6;
    wr_i(fo, (int)pm.size);
    for (usize i = 0; i < pm.size; i++) wr(fo, pm.points.ptr<float>((int)i), 16);
    for (usize i = 0; i < pm.size; i++) {
        const unsigned char c[3] = {pm.colors[i].x, pm.colors[i].y, pm.colors[i].z};
        wr(fo, c, 3);
    }
    for (usize i = 0; i < pm.size; i++) {
        wr_i(fo, (int)pm.frame_ids[i].size());
        for (usize k = 0; k < pm.frame_ids[i].size(); k++) {
            wr_i(fo, (int)pm.frame_ids[i][k]);
            wr_i(fo, (int)pm.frame_point_ids[i][k]);
        }
    }
    for (int f = 0; f < nf; f++) {
        const Frame &fr = pm.frames[f];
        wr_i(fo, (int)fr.map_point_ids.size());
        for (s32 v : fr.map_point_ids) wr_i(fo, v);
        wr(fo, fr.R_t.ptr<float>(0), 64);
        wr(fo, fr.pose.ptr<float>(0), 64);
    }
    // orb_distance of every map point against keypoint 0 of the last frame (host-side members, after sync_to_host)
    for (usize i = 0; i < pm.size; i++) wr_i(fo, (int)orb_distance(pm, i, pm.frames.back(), 0));
    // add_reprojection_inliers on the host-side members: one more point, from match 0 of a made-up pair
    cv::Mat p4(1, 4, CV_32FC1);
    const float one[4] = {1.5f, -2.f, 3.f, 7.f};
    for (int i = 0; i < 4; i++) p4.ptr<float>(0)[i] = one[i];
    const usize before = pm.size;
    add_reprojection_inliers(pm, p4, {0}, {cv::Point3_<u8>(1, 2, 3)}, 4, 5, {{11, 12}});
    const int ok = pm.size == before + 1 && pm.points.ptr<float>((int)before)[2] == 3.f && pm.points.ptr<float>((int)before)[3] == 1.f &&
                   pm.frame_ids[before] == std::vector<usize>({4, 5}) && pm.frame_point_ids[before] == std::vector<usize>({11, 12}) &&
                   pm.colors[before] == cv::Point3_<u8>(1, 2, 3) && pm.points.ptr<float>(0)[3] == 1.f;
    wr_i(fo, ok);
    fclose(fo);
    return 0;
}
