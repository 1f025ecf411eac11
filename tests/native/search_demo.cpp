// Uses the C++ surfaces of the search by projection the way a consumer of include/vslam/*.h would, and dumps what they give so
// that tests/test_gpu_search.py can hold it to the C entry point's bits:
//   vslam::search_projection (include/vslam/helpers.h) on one item a caller already holds on the device, then
//   vslam::World::search (include/vslam/World.h) on a world attached to a map at frame 0 -- an empty map: the call is taken and
//   finds nothing -- and on a world that is not attached, which throws.
//
// usage: search_demo <in.bin> <out.bin>
//   in:  K [9] f32; int32 S, O, Kp, n_points, n_kp, width, height; R [9], T [3] f64; points [S][4] f32; int32 offsets [S + 1];
//        u8 obs [O][32]; xy [Kp][2] f32; u8 desc [Kp][32]
//   out: int32 kp_of_point [S], dist [S], corr_point [Kp], corr_kp [Kp], n_corr, stats [4]; f64 corr_points [Kp][3]; f32 corr_xy
//        [Kp][2] (outputs start zeroed); int32 n_corr [2] of the attached world; int32 1 when the unattached world threw
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
    std::vector<int> h(7);
    if (!take(fi, k) || !take(fi, h)) return 3;
    const int S = h[0], O = h[1], Kp = h[2], width = h[5], height = h[6];
    if (S <= 0 || O <= 0 || Kp <= 0) return 3;
    cv::Mat K(3, 3, CV_32FC1);
    for (int r = 0; r < 3; r++) std::memcpy(K.ptr<float>(r), k.data() + 3 * r, 12);
    std::vector<double> R(9), T(3);
    std::vector<float> points(4 * (size_t)S), xy(2 * (size_t)Kp);
    std::vector<int> offsets((size_t)S + 1), n_points{h[3]}, n_kp{h[4]};
    std::vector<unsigned char> obs(32 * (size_t)O), desc(32 * (size_t)Kp);
    if (!take(fi, R) || !take(fi, T) || !take(fi, points) || !take(fi, offsets) || !take(fi, obs) || !take(fi, xy) || !take(fi, desc)) return 3;
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    std::vector<int> kp_of_point(S, 0), dist(S, 0), corr_point(Kp, 0), corr_kp(Kp, 0), n_corr(1, 0), stats(4, 0);
    std::vector<double> corr_points(3 * (size_t)Kp, 0.0);
    std::vector<float> corr_xy(2 * (size_t)Kp, 0.f);
    int threw = 0;
    std::vector<int> world_n(2, -7);
    try {
        const double *d_R = upload(ctx, R), *d_T = upload(ctx, T);
        const float *d_points = upload(ctx, points), *d_xy = upload(ctx, xy);
        const int *d_off = upload(ctx, offsets), *d_np = upload(ctx, n_points), *d_nk = upload(ctx, n_kp);
        const unsigned char *d_obs = upload(ctx, obs), *d_desc = upload(ctx, desc);
        int *d_kop = upload(ctx, kp_of_point), *d_dist = upload(ctx, dist), *d_cp = upload(ctx, corr_point), *d_ck = upload(ctx, corr_kp),
            *d_nc = upload(ctx, n_corr), *d_st = upload(ctx, stats);
        double *d_cpts = upload(ctx, corr_points);
        float *d_cxy = upload(ctx, corr_xy);
        vslam::search_projection(ctx, d_points, d_np, S, d_off, d_obs, O, d_R, d_T, K, width, height, d_xy, d_desc, d_nk, Kp, nullptr, 1, d_kop,
                                 d_dist, d_cpts, d_cxy, d_cp, d_ck, d_nc, d_st);
        if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
        download(ctx, kp_of_point, d_kop); download(ctx, dist, d_dist); download(ctx, corr_point, d_cp); download(ctx, corr_kp, d_ck);
        download(ctx, n_corr, d_nc); download(ctx, stats, d_st); download(ctx, corr_points, d_cpts); download(ctx, corr_xy, d_cxy);

        const int tracks = 2, frames = 3, kp = 16;
        vslam_map *map = nullptr;
        if (vslam_map_create(ctx, tracks, frames, kp, 32, 64, &map) != VSLAM_OK) return 8;
        std::vector<float> zxy(2 * (size_t)tracks * kp, 1.f);
        std::vector<unsigned char> zdesc(32 * (size_t)tracks * kp, 0);
        std::vector<int> zn(tracks, kp), zi((size_t)tracks * kp, 0);
        const float *d_zxy = upload(ctx, zxy);
        const unsigned char *d_zdesc = upload(ctx, zdesc);
        const int *d_zn = upload(ctx, zn);
        int *d_wp = upload(ctx, zi), *d_wk = upload(ctx, zi), *d_wn = upload(ctx, world_n);
        {
            vslam::World world(ctx, tracks, frames, kp), loose(ctx, tracks, frames, kp);
            world.attach_to(map);
            world.search(map, d_zxy, d_zdesc, d_zn, k.data(), width, height, d_wp, d_wk, d_wn);
            if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
            download(ctx, world_n, d_wn);
            try {
                loose.search(map, d_zxy, d_zdesc, d_zn, k.data(), width, height, d_wp, d_wk, d_wn);
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            vslam_map_destroy(map);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 9;
    }
    fwrite(kp_of_point.data(), 4, kp_of_point.size(), fo);
    fwrite(dist.data(), 4, dist.size(), fo);
    fwrite(corr_point.data(), 4, corr_point.size(), fo);
    fwrite(corr_kp.data(), 4, corr_kp.size(), fo);
    fwrite(n_corr.data(), 4, 1, fo);
    fwrite(stats.data(), 4, 4, fo);
    fwrite(corr_points.data(), 8, corr_points.size(), fo);
    fwrite(corr_xy.data(), 4, corr_xy.size(), fo);
    fwrite(world_n.data(), 4, 2, fo);
    fwrite(&threw, 4, 1, fo);
    fclose(fi);
    fclose(fo);
    vslam_ctx_destroy(ctx);
    return 0;
}
