// Uses the C++ surfaces of the track triangulation the way a consumer of include/vslam/*.h would, and dumps what they give so that
// tests/test_gpu_tracks.py can hold it to the C entry point's bits:
//   vslam::triangulate_tracks (include/vslam/helpers.h) on one item that the caller already holds on the device, then
//   vslam::World::retriangulate (include/vslam/World.h) on a world attached to a map at frame 0 -- an empty map: the call is taken,
//   nothing takes part -- and on a world that is not attached, which throws.
//
// usage: tracks_demo <in.bin> <out.bin>
//   in:  int32 S, O, n, Cs, C, Kp; K [9] f32; points [S][4] f32; int32 offsets [S + 1], cam [O], kp [O]; f64 R [Cs][9], T [Cs][3];
//        f32 xy [Cs][Kp][2]
//   out: f32 out_points [S][4]; int32 status [S], counts [S][2]; f64 info [S][3]; int32 stats [4]; int32 world stats [4] of track 0;
//        int32 1 when the unattached world threw
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

template <typename T>
static void put(FILE *f, const std::vector<T> &v) {
    fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    std::vector<int> g(6);
    std::vector<float> k(9);
    if (!take(fi, g) || !take(fi, k)) return 3;
    const int S = g[0], O = g[1], Cs = g[3], Kp = g[5];
    if (S <= 0 || O <= 0 || Cs <= 0 || Kp <= 0) return 3;
    std::vector<float> points(4 * (size_t)S), xy(2 * (size_t)Cs * Kp);
    std::vector<int> off((size_t)S + 1), cam(O), kp(O), n{g[2]}, ncams{g[4]};
    std::vector<double> R(9 * (size_t)Cs), T(3 * (size_t)Cs);
    if (!take(fi, points) || !take(fi, off) || !take(fi, cam) || !take(fi, kp) || !take(fi, R) || !take(fi, T) || !take(fi, xy)) return 3;
    cv::Mat K(3, 3, CV_32FC1);
    for (int r = 0; r < 3; r++) std::memcpy(K.ptr<float>(r), k.data() + 3 * r, 12);
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    std::vector<float> out_points(4 * (size_t)S, 0.f);
    std::vector<int> status(S, 0), counts(2 * (size_t)S, 0), stats(4, 0);
    std::vector<double> info(3 * (size_t)S, 0.0);
    const int tracks = 2, frames = 3, wkp = 16, mcap = 32, ocap = 64;
    std::vector<int> wstats(4 * tracks, -7);
    int threw = 0;
    try {
        const float *d_points = upload(ctx, points), *d_xy = upload(ctx, xy);
        const int *d_n = upload(ctx, n), *d_off = upload(ctx, off), *d_cam = upload(ctx, cam), *d_kp = upload(ctx, kp), *d_nc = upload(ctx, ncams);
        const double *d_R = upload(ctx, R), *d_T = upload(ctx, T);
        float *d_out = upload(ctx, out_points);
        int *d_status = upload(ctx, status), *d_counts = upload(ctx, counts), *d_stats = upload(ctx, stats);
        double *d_info = upload(ctx, info);
        vslam::triangulate_tracks(ctx, d_points, d_n, S, d_off, d_cam, d_kp, O, d_R, d_T, d_nc, Cs, d_xy, Kp, K, 1, d_out, d_status, d_stats, d_counts,
                                  d_info);
        if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
        download(ctx, out_points, d_out); download(ctx, status, d_status); download(ctx, counts, d_counts); download(ctx, info, d_info);
        download(ctx, stats, d_stats);

        vslam_map *map = nullptr;
        if (vslam_map_create(ctx, tracks, frames, wkp, mcap, ocap, &map) != VSLAM_OK) return 8;
        std::vector<float> zxy(2 * (size_t)tracks * frames * wkp, 1.f);
        const float *d_zxy = upload(ctx, zxy);
        int *d_ws = upload(ctx, wstats);
        {
            vslam::World world(ctx, tracks, frames, wkp), loose(ctx, tracks, frames, wkp);
            world.attach_to(map);
            world.retriangulate(map, d_zxy, frames, k.data(), nullptr, nullptr, d_ws);
            if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
            download(ctx, wstats, d_ws);
            try {
                loose.retriangulate(map, d_zxy, frames, k.data());
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            vslam_map_destroy(map);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 9;
    }
    wstats.resize(4);
    put(fo, out_points); put(fo, status); put(fo, counts); put(fo, info); put(fo, stats);
    put(fo, wstats);
    fwrite(&threw, 4, 1, fo);
    fclose(fi);
    fclose(fo);
    vslam_ctx_destroy(ctx);
    return 0;
}
