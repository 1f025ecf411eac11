// Uses the C++ surfaces of the similarity between two views the way a consumer of include/vslam/*.h would, and dumps what they give so
// that tests/test_gpu_sim3.py can hold it to the Python call's bits:
//   vslam::sim3_ransac (include/vslam/helpers.h) on one item a caller already holds on the device, without a polish, then
//   vslam::sim3_refine on the winner's mask with the default parameters, then vslam::World::sim3 and vslam::World::apply_sim3
//   (include/vslam/World.h) on a world attached to a map at frame 0 -- an empty map: the calls are taken, nothing is found --, and
//   apply_sim3 with a track listed twice, which throws.
//
// usage: sim3_demo <in.bin> <out.bin>
//   in:  K [9] f32; int32 S, n, seed; s, R [9], T [3] f64 (the bits an item left alone keeps); A [S][3], B [S][3] f64; xa [S][2],
//        xb [S][2] f32
//   out: f64 s, R [9], T [3] of the RANSAC; int32 inlier [S], corr_index [S], n_inliers, winner (outputs start zeroed); f64 s, R [9],
//        T [3], stats [4] behind the refinement; int32 found [2], n_corr [2] of the attached world; int32 1 when the duplicate threw
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "vslam/World.h"
#include "vslam/helpers.h"

template <typename T>
static bool take(FILE *f, std::vector<T> &v) {
    return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <typename T>
static T *upload(vslam_ctx *ctx, const std::vector<T> &v) {
    void *d = nullptr;
    if (vslam_dev_alloc(ctx, sizeof(T) * v.size(), &d) || vslam_copy_h2d(ctx, d, v.data(), sizeof(T) * v.size())) throw std::runtime_error("upload");
    return static_cast<T *>(d);
}

template <typename T>
static void download(vslam_ctx *ctx, std::vector<T> &v, const T *d) {
    if (vslam_copy_d2h(ctx, v.data(), d, sizeof(T) * v.size())) throw std::runtime_error("download");
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    std::vector<float> k(9);
    std::vector<int> h(3);
    if (!take(fi, k) || !take(fi, h)) return 3;
    const int S = h[0];
    if (S <= 0) return 3;
    cv::Mat K(3, 3, CV_32FC1);
    for (int r = 0; r < 3; r++) std::memcpy(K.ptr<float>(r), k.data() + 3 * r, 12);
    std::vector<double> s(1), R(9), T(3), A(3 * (size_t)S), B(3 * (size_t)S);
    std::vector<float> xa(2 * (size_t)S), xb(2 * (size_t)S);
    if (!take(fi, s) || !take(fi, R) || !take(fi, T) || !take(fi, A) || !take(fi, B) || !take(fi, xa) || !take(fi, xb)) return 3;
    std::vector<int> n{h[1]};
    std::vector<unsigned int> seeds{(unsigned int)h[2]};
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    std::vector<int> inlier(S, 0), corr_index(S, 0), n_inliers(1, 0), winner(1, 0);
    std::vector<double> s2(1), R2(9), T2(3), stats(4, 0.0);
    std::vector<int> world_found(2, -7), world_n(2, -7);
    int threw = 0;
    try {
        double *d_s = upload(ctx, s), *d_R = upload(ctx, R), *d_T = upload(ctx, T), *d_st = upload(ctx, stats);
        const double *d_A = upload(ctx, A), *d_B = upload(ctx, B);
        const float *d_xa = upload(ctx, xa), *d_xb = upload(ctx, xb);
        const int *d_n = upload(ctx, n);
        const unsigned int *d_seeds = upload(ctx, seeds);
        int *d_in = upload(ctx, inlier), *d_ci = upload(ctx, corr_index), *d_ni = upload(ctx, n_inliers), *d_w = upload(ctx, winner);
        vslam::sim3_ransac(ctx, d_A, d_xa, d_B, d_xb, d_n, 1, S, K, d_seeds, d_s, d_R, d_T, d_in, d_ci, d_ni, d_w);
        if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
        download(ctx, s, d_s); download(ctx, R, d_R); download(ctx, T, d_T); download(ctx, inlier, d_in); download(ctx, corr_index, d_ci);
        download(ctx, n_inliers, d_ni); download(ctx, winner, d_w);
        vslam::sim3_refine(ctx, d_A, d_xa, d_B, d_xb, d_n, 1, S, d_in, K, d_s, d_R, d_T, d_st);
        if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
        download(ctx, s2, d_s); download(ctx, R2, d_R); download(ctx, T2, d_T); download(ctx, stats, d_st);

        const int tracks = 2, frames = 3, kp = 16;
        vslam_map *map = nullptr;
        if (vslam_map_create(ctx, tracks, frames, kp, 32, 64, &map) != VSLAM_OK) return 8;
        std::vector<float> zxy(2 * (size_t)tracks * kp, 1.f);
        std::vector<int> zm(2 * (size_t)tracks * kp, 0), zn(tracks, kp), zt(tracks, -7), t01{0, 1}, f0(tracks, 0), ones(tracks, 1);
        std::vector<unsigned int> zseeds(tracks, 1u);
        std::vector<double> z9(9 * (size_t)tracks, 0.0);
        const float *d_zxy = upload(ctx, zxy);
        const int *d_zm = upload(ctx, zm), *d_zn = upload(ctx, zn), *d_t01 = upload(ctx, t01), *d_f0 = upload(ctx, f0), *d_ones = upload(ctx, ones);
        const unsigned int *d_zs = upload(ctx, zseeds);
        double *d_ws = upload(ctx, z9), *d_wR = upload(ctx, z9), *d_wT = upload(ctx, z9), *d_wsw = upload(ctx, z9), *d_wRw = upload(ctx, z9),
               *d_wtw = upload(ctx, z9);
        int *d_wf = upload(ctx, zt), *d_wn = upload(ctx, zt), *d_wi = upload(ctx, zt), *d_ww = upload(ctx, zt);
        {
            vslam::World world(ctx, tracks, frames, kp);
            world.attach_to(map);
            world.sim3(map, d_t01, d_f0, d_t01, d_f0, tracks, d_zm, d_zn, d_zxy, d_zxy, k.data(), d_zs, d_ws, d_wR, d_wT, d_wsw, d_wRw, d_wtw, d_wf,
                       d_wn, d_wi, d_ww);
            const int once[2] = {1, 0}, twice[2] = {1, 1};
            world.apply_sim3(map, once, d_wsw, d_wRw, d_wtw, d_ones, 2);   // s = 0: every track is left alone
            if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
            download(ctx, world_found, d_wf);
            download(ctx, world_n, d_wn);
            try {
                world.apply_sim3(map, twice, d_wsw, d_wRw, d_wtw, d_ones, 2);
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            vslam_map_destroy(map);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 9;
    }
    fwrite(s.data(), 8, 1, fo);
    fwrite(R.data(), 8, 9, fo);
    fwrite(T.data(), 8, 3, fo);
    fwrite(inlier.data(), 4, inlier.size(), fo);
    fwrite(corr_index.data(), 4, corr_index.size(), fo);
    fwrite(n_inliers.data(), 4, 1, fo);
    fwrite(winner.data(), 4, 1, fo);
    fwrite(s2.data(), 8, 1, fo);
    fwrite(R2.data(), 8, 9, fo);
    fwrite(T2.data(), 8, 3, fo);
    fwrite(stats.data(), 8, 4, fo);
    fwrite(world_found.data(), 4, 2, fo);
    fwrite(world_n.data(), 4, 2, fo);
    fwrite(&threw, 4, 1, fo);
    fclose(fi);
    fclose(fo);
    vslam_ctx_destroy(ctx);
    return 0;
}
