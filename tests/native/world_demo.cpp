// Uses the C++ surfaces of the world frame the way a consumer of include/vslam/*.h would, and dumps what they give so that
// tests/test_gpu_world.py can hold it to the C entry points:
//   mode 0  vslam::World (include/vslam/World.h) stepped by hand on one track's script, every pair's points lifted;
//   mode 1  the reference's loop over a PointMap with a world attached (vslam::map_attach_world), then sync_to_host() and
//           world_points() / world_poses().
//
// usage: world_demo <in.bin> <out.bin>
//   mode 0 in:  int32 0, kp_stride, steps; per step: int32 winner, n, n_last, n_cur; R [9] f32; t [3] f32; matches [n][2] i32;
//               X [n][4] f32
//          out: Twc [frames][16] f64; pose [frames][16] f32; scale [frames] f64; links [frames] i32; per step the lifted
//               points [kp_stride][4] f32 (rows [0, n) lifted, the rest zero)
//   mode 1 in:  int32 1, w, h, max_corners, hyp, frames; uint32 seeds[frames - 1]; BGR frames
//          out: int32 size; points [size][4] f32; world_points [size][4] f32; int32 poses; world_poses [poses][16] f32
#include <cstdio>
#include <vector>

#include "vslam/Frame.h"
#include "vslam/PointMap.h"
#include "vslam/World.h"

static int run_script(FILE *fi, FILE *fo) {
    int hdr[2];
    if (fread(hdr, 4, 2, fi) != 2) return 3;
    const int K = hdr[0], steps = hdr[1], frames = steps + 1;
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    void *d_m, *d_best, *d_X, *d_R, *d_t, *d_nl, *d_nc, *d_lo, *d_hi, *d_out;
    if (vslam_dev_alloc(ctx, 8 * (size_t)K, &d_m) || vslam_dev_alloc(ctx, 16, &d_best) || vslam_dev_alloc(ctx, 16 * (size_t)K, &d_X) ||
        vslam_dev_alloc(ctx, 36, &d_R) || vslam_dev_alloc(ctx, 12, &d_t) || vslam_dev_alloc(ctx, 4, &d_nl) ||
        vslam_dev_alloc(ctx, 4, &d_nc) || vslam_dev_alloc(ctx, 4, &d_lo) || vslam_dev_alloc(ctx, 4, &d_hi) ||
        vslam_dev_alloc(ctx, 16 * (size_t)K, &d_out))
        return 5;
    std::vector<std::vector<float>> lifted;
    std::vector<double> Twc((size_t)frames * 16), scale((size_t)frames);
    std::vector<float> pose((size_t)frames * 16);
    std::vector<int> links((size_t)frames);
    {
        vslam::World world(ctx, 1, frames, K);
        for (int s = 0; s < steps; s++) {
            int h[4];
            float R[9], t[3];
            if (fread(h, 4, 4, fi) != 4 || fread(R, 4, 9, fi) != 9 || fread(t, 4, 3, fi) != 3) return 3;
            const int n = h[1];
            if (n < 0 || n > K) return 3;
            std::vector<int> m(2 * (size_t)K, 0);
            std::vector<float> X(4 * (size_t)K, 0.f), zero(4 * (size_t)K, 0.f);
            if (n && (fread(m.data(), 8, (size_t)n, fi) != (size_t)n || fread(X.data(), 16, (size_t)n, fi) != (size_t)n)) return 3;
            const int best[4] = {h[0] ? 0 : -1, n, 0, n}, lo = 0;
            if (vslam_copy_h2d(ctx, d_m, m.data(), 8 * (size_t)K) || vslam_copy_h2d(ctx, d_best, best, 16) ||
                vslam_copy_h2d(ctx, d_X, X.data(), 16 * (size_t)K) || vslam_copy_h2d(ctx, d_R, R, 36) || vslam_copy_h2d(ctx, d_t, t, 12) ||
                vslam_copy_h2d(ctx, d_nl, &h[2], 4) || vslam_copy_h2d(ctx, d_nc, &h[3], 4) || vslam_copy_h2d(ctx, d_lo, &lo, 4) ||
                vslam_copy_h2d(ctx, d_hi, &n, 4) || vslam_copy_h2d(ctx, d_out, zero.data(), 16 * (size_t)K))
                return 6;
            world.step((const int32_t *)d_m, (const int32_t *)d_best, (const float *)d_X, (const float *)d_R, (const float *)d_t,
                       (const int32_t *)d_nl, (const int32_t *)d_nc);
            world.lift(s + 1, (const float *)d_X, K, (const int32_t *)d_lo, (const int32_t *)d_hi, (float *)d_out);
            lifted.emplace_back(4 * (size_t)K);
            if (vslam_copy_d2h(ctx, lifted.back().data(), d_out, 16 * (size_t)K)) return 7;
        }
        const vslam_world_arrays a = world.view();
        if (a.frames != frames || vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
        if (vslam_copy_d2h(ctx, Twc.data(), a.d_Twc, 128 * (size_t)frames) || vslam_copy_d2h(ctx, pose.data(), a.d_pose, 64 * (size_t)frames) ||
            vslam_copy_d2h(ctx, scale.data(), a.d_scale, 8 * (size_t)frames) || vslam_copy_d2h(ctx, links.data(), a.d_links, 4 * (size_t)frames))
            return 7;
    }
    for (void *p : {d_m, d_best, d_X, d_R, d_t, d_nl, d_nc, d_lo, d_hi, d_out}) vslam_dev_free(ctx, p);
    vslam_ctx_destroy(ctx);
    fwrite(Twc.data(), 8, Twc.size(), fo);
    fwrite(pose.data(), 4, pose.size(), fo);
    fwrite(scale.data(), 8, scale.size(), fo);
    fwrite(links.data(), 4, links.size(), fo);
    for (const auto &l : lifted) fwrite(l.data(), 4, l.size(), fo);
    return 0;
}

static int run_pointmap(FILE *fi, FILE *fo) {
    int hdr[5];
    if (fread(hdr, 4, 5, fi) != 5) return 3;
    const int w = hdr[0], h = hdr[1], maxc = hdr[2], hyp = hdr[3], nf = hdr[4];
    std::vector<unsigned> seeds(nf - 1);
    if (fread(seeds.data(), 4, seeds.size(), fi) != seeds.size()) return 3;
    std::vector<std::vector<unsigned char>> img(nf);
    for (auto &b : img) {
        b.resize((size_t)w * h * 3);
        if (fread(b.data(), 1, b.size(), fi) != b.size()) return 3;
    }
    vslam::settings().max_corners = maxc;
    const float kv[9] = {525.f, 0, (float)(w / 2), 0, 525.f, (float)(h / 2), 0, 0, 1};
    cv::Mat K(3, 3, CV_32FC1);
    for (int i = 0; i < 9; i++) K.ptr<float>(i / 3)[i % 3] = kv[i];
    PointMap pm;
    vslam::map_create(pm, nf, maxc, nf * maxc, 4 * nf * maxc);
    vslam::map_attach_world(pm);
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
    const int size = (int)pm.size, poses = (int)pm.world_poses().size();
    if (pm.world_points().rows != size) return 8;
    fwrite(&size, 4, 1, fo);
    for (int i = 0; i < size; i++) fwrite(pm.points.ptr<float>(i), 4, 4, fo);
    for (int i = 0; i < size; i++) fwrite(pm.world_points().ptr<float>(i), 4, 4, fo);
    fwrite(&poses, 4, 1, fo);
    for (const cv::Mat &pose4 : pm.world_poses()) fwrite(pose4.ptr<float>(0), 4, 16, fo);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    int mode = 0;
    if (!fi || !fo || fread(&mode, 4, 1, fi) != 1) return 3;
    const int rc = mode == 0 ? run_script(fi, fo) : run_pointmap(fi, fo);
    fclose(fi);
    fclose(fo);
    return rc;
}
