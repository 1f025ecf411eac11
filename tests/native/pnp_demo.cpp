// Uses the C++ surfaces of the pose without a prior the way a consumer of include/vslam/*.h would, and dumps what they give so
// that tests/test_gpu_pnp.py can hold it to the Python call's bits:
//   vslam::pnp_ransac (include/vslam/helpers.h) on one item a caller already holds on the device, with the default polish, then
//   vslam::World::relocalise (include/vslam/World.h) on a world attached to a map at frame 0 -- an empty map: the call is taken and
//   finds nothing -- and on a world that is not attached, which throws.
//
// usage: pnp_demo <in.bin> <out.bin>
//   in:  K [9] f32; int32 S, n, seed; R [9], T [3] f64 (the bits an item left alone keeps); points [S][3] f64; xy [S][2] f32
//   out: f64 R [9], T [3]; int32 inlier [S], corr_index [S], n_inliers, winner; f64 stats [4], corr_points [S][3]; f32 corr_xy
//        [S][2] (outputs start zeroed); int32 found [2], n_corr [2] of the attached world; int32 1 when the unattached world threw
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
    std::vector<double> R(9), T(3), points(3 * (size_t)S);
    std::vector<float> xy(2 * (size_t)S);
    if (!take(fi, R) || !take(fi, T) || !take(fi, points) || !take(fi, xy)) return 3;
    std::vector<int> n{h[1]};
    std::vector<unsigned int> seeds{(unsigned int)h[2]};
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    std::vector<int> inlier(S, 0), corr_index(S, 0), n_inliers(1, 0), winner(1, 0);
    std::vector<double> stats(4, 0.0), corr_points(3 * (size_t)S, 0.0);
    std::vector<float> corr_xy(2 * (size_t)S, 0.f);
    std::vector<int> world_found(2, -7), world_n(2, -7);
    int threw = 0;
    try {
        double *d_R = upload(ctx, R), *d_T = upload(ctx, T), *d_st = upload(ctx, stats), *d_cpts = upload(ctx, corr_points);
        const double *d_points = upload(ctx, points);
        const float *d_xy = upload(ctx, xy);
        float *d_cxy = upload(ctx, corr_xy);
        const int *d_n = upload(ctx, n);
        const unsigned int *d_seeds = upload(ctx, seeds);
        int *d_in = upload(ctx, inlier), *d_ci = upload(ctx, corr_index), *d_ni = upload(ctx, n_inliers), *d_w = upload(ctx, winner);
        vslam_resect_params polish;
        vslam_resect_params_default(&polish);
        vslam::pnp_ransac(ctx, d_points, d_xy, d_n, 1, S, K, d_seeds, d_R, d_T, d_in, d_cpts, d_cxy, d_ci, d_ni, d_w, nullptr, d_st, nullptr, &polish);
        if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
        download(ctx, R, d_R); download(ctx, T, d_T); download(ctx, inlier, d_in); download(ctx, corr_index, d_ci);
        download(ctx, n_inliers, d_ni); download(ctx, winner, d_w); download(ctx, stats, d_st); download(ctx, corr_points, d_cpts);
        download(ctx, corr_xy, d_cxy);

        const int tracks = 2, frames = 3, kp = 16;
        vslam_map *map = nullptr;
        if (vslam_map_create(ctx, tracks, frames, kp, 32, 64, &map) != VSLAM_OK) return 8;
        std::vector<float> zxy(2 * (size_t)tracks * kp, 1.f);
        std::vector<unsigned char> zdesc(32 * (size_t)tracks * kp, 0);
        std::vector<int> zn(tracks, kp), zi((size_t)tracks * kp, 0), zt(tracks, -7);
        std::vector<unsigned int> zseeds(tracks, 1u);
        const float *d_zxy = upload(ctx, zxy);
        const unsigned char *d_zdesc = upload(ctx, zdesc);
        const int *d_zn = upload(ctx, zn);
        const unsigned int *d_zs = upload(ctx, zseeds);
        int *d_wp = upload(ctx, zi), *d_wk = upload(ctx, zi), *d_wn = upload(ctx, zt), *d_wf = upload(ctx, zt), *d_ww = upload(ctx, zt),
            *d_wi = upload(ctx, zt);
        {
            vslam::World world(ctx, tracks, frames, kp), loose(ctx, tracks, frames, kp);
            world.attach_to(map);
            world.relocalise(map, d_zxy, d_zdesc, d_zn, k.data(), d_zs, d_wf, d_ww, d_wi, d_wp, d_wk, d_wn, &polish);
            if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
            download(ctx, world_found, d_wf);
            download(ctx, world_n, d_wn);
            try {
                loose.relocalise(map, d_zxy, d_zdesc, d_zn, k.data(), d_zs, d_wf, d_ww, d_wi, d_wp, d_wk, d_wn);
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            vslam_map_destroy(map);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 9;
    }
    fwrite(R.data(), 8, 9, fo);
    fwrite(T.data(), 8, 3, fo);
    fwrite(inlier.data(), 4, inlier.size(), fo);
    fwrite(corr_index.data(), 4, corr_index.size(), fo);
    fwrite(n_inliers.data(), 4, 1, fo);
    fwrite(winner.data(), 4, 1, fo);
    fwrite(stats.data(), 8, 4, fo);
    fwrite(corr_points.data(), 8, corr_points.size(), fo);
    fwrite(corr_xy.data(), 4, corr_xy.size(), fo);
    fwrite(world_found.data(), 4, 2, fo);
    fwrite(world_n.data(), 4, 2, fo);
    fwrite(&threw, 4, 1, fo);
    fclose(fi);
    fclose(fo);
    vslam_ctx_destroy(ctx);
    return 0;
}
