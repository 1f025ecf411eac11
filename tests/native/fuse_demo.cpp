// Uses the C++ surfaces of the fusion and the cull the way a consumer of include/vslam/*.h would, and dumps what they give so that
// tests/test_gpu_fuse.py can hold it to the C entry points' bits:
//   vslam::fuse_points and vslam::cull_points (include/vslam/helpers.h) on one item each that the caller already holds on the device,
//   then vslam::World::fuse / cull / observations / fuse_to (include/vslam/World.h) on a world attached to a map at frame 0 -- an
//   empty map: the calls are taken, nothing takes part -- and World::fuse on a world that is not attached, which throws.
//
// usage: fuse_demo <in.bin> <out.bin>
//   in:  int32 S, O, n, cam_stride, kp_stride; int32 offsets [S + 1], cam [O], kp [O], mask [S];
//        int32 cS, cO, cn, Cs, C, Kp; K [9] f32; points [cS][4] f32; int32 offsets [cS + 1], cam [cO], kp [cO]; f64 R [Cs][9], T [Cs][3];
//        f32 xy [Cs][Kp][2]
//   out: int32 fuse_to [S], out_offsets [S + 1], out_cam [O], out_kp [O], out_src [O], stats [4] (outputs start zeroed);
//        int32 keep [cS], counts [cS][2], stats [4]; int32 world stats of fuse [2][4] and cull [2][4], state, offsets [2][33];
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
    std::vector<int> h(5);
    if (!take(fi, h)) return 3;
    const int S = h[0], O = h[1], cam_stride = h[3], kp_stride = h[4];
    if (S <= 0 || O <= 0) return 3;
    std::vector<int> offsets((size_t)S + 1), cam(O), kp(O), mask(S), n{h[2]};
    if (!take(fi, offsets) || !take(fi, cam) || !take(fi, kp) || !take(fi, mask)) return 3;
    std::vector<int> g(6);
    std::vector<float> k(9);
    if (!take(fi, g) || !take(fi, k)) return 3;
    const int cS = g[0], cO = g[1], Cs = g[3], Kp = g[5];
    if (cS <= 0 || cO <= 0 || Cs <= 0 || Kp <= 0) return 3;
    std::vector<float> points(4 * (size_t)cS), xy(2 * (size_t)Cs * Kp);
    std::vector<int> coff((size_t)cS + 1), ccam(cO), ckp(cO), cn{g[2]}, ncams{g[4]};
    std::vector<double> R(9 * (size_t)Cs), T(3 * (size_t)Cs);
    if (!take(fi, points) || !take(fi, coff) || !take(fi, ccam) || !take(fi, ckp) || !take(fi, R) || !take(fi, T) || !take(fi, xy)) return 3;
    cv::Mat K(3, 3, CV_32FC1);
    for (int r = 0; r < 3; r++) std::memcpy(K.ptr<float>(r), k.data() + 3 * r, 12);
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    std::vector<int> fuse_to(S, 0), out_off((size_t)S + 1, 0), out_cam(O, 0), out_kp(O, 0), out_src(O, 0), stats(4, 0);
    std::vector<int> keep(cS, 0), counts(2 * (size_t)cS, 0), cstats(4, 0);
    const int tracks = 2, frames = 3, wkp = 16, mcap = 32, ocap = 64;
    std::vector<int> wfuse(4 * tracks, -7), wcull(4 * tracks, -7), woff((size_t)tracks * (mcap + 1), -7), state{-7};
    int threw = 0;
    try {
        const int *d_n = upload(ctx, n), *d_off = upload(ctx, offsets), *d_cam = upload(ctx, cam), *d_kp = upload(ctx, kp), *d_mask = upload(ctx, mask);
        int *d_to = upload(ctx, fuse_to), *d_oo = upload(ctx, out_off), *d_oc = upload(ctx, out_cam), *d_ok = upload(ctx, out_kp),
            *d_os = upload(ctx, out_src), *d_st = upload(ctx, stats);
        vslam::fuse_points(ctx, d_n, S, d_off, d_cam, d_kp, O, cam_stride, kp_stride, d_mask, 1, d_to, d_oo, d_oc, d_ok, d_os, d_st);
        const float *d_points = upload(ctx, points), *d_xy = upload(ctx, xy);
        const int *d_cn = upload(ctx, cn), *d_coff = upload(ctx, coff), *d_ccam = upload(ctx, ccam), *d_ckp = upload(ctx, ckp), *d_nc = upload(ctx, ncams);
        const double *d_R = upload(ctx, R), *d_T = upload(ctx, T);
        int *d_keep = upload(ctx, keep), *d_counts = upload(ctx, counts), *d_cst = upload(ctx, cstats);
        vslam::cull_points(ctx, d_points, d_cn, cS, d_coff, d_ccam, d_ckp, cO, d_R, d_T, d_nc, Cs, d_xy, Kp, K, 1, d_keep, d_cst, d_counts);
        if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
        download(ctx, fuse_to, d_to); download(ctx, out_off, d_oo); download(ctx, out_cam, d_oc); download(ctx, out_kp, d_ok);
        download(ctx, out_src, d_os); download(ctx, stats, d_st);
        download(ctx, keep, d_keep); download(ctx, counts, d_counts); download(ctx, cstats, d_cst);

        vslam_map *map = nullptr;
        if (vslam_map_create(ctx, tracks, frames, wkp, mcap, ocap, &map) != VSLAM_OK) return 8;
        std::vector<float> zxy(2 * (size_t)tracks * frames * wkp, 1.f);
        std::vector<int> zo((size_t)tracks * ocap, 0);
        const float *d_zxy = upload(ctx, zxy);
        int *d_wf = upload(ctx, wfuse), *d_wc = upload(ctx, wcull), *d_wo = upload(ctx, woff), *d_fr = upload(ctx, zo), *d_pt = upload(ctx, zo);
        {
            vslam::World world(ctx, tracks, frames, wkp), loose(ctx, tracks, frames, wkp);
            world.attach_to(map);
            if (world.fuse_to() != nullptr) return 10;
            world.fuse(map, d_wf);
            world.cull(map, d_zxy, frames, k.data(), nullptr, d_wc);
            world.observations(map, d_wo, d_fr, d_pt);
            int32_t st = 0;
            if (world.fuse_to(&st) == nullptr) return 10;
            state[0] = st;
            if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
            download(ctx, wfuse, d_wf); download(ctx, wcull, d_wc); download(ctx, woff, d_wo);
            try {
                loose.fuse(map);
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            vslam_map_destroy(map);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 9;
    }
    put(fo, fuse_to); put(fo, out_off); put(fo, out_cam); put(fo, out_kp); put(fo, out_src); put(fo, stats);
    put(fo, keep); put(fo, counts); put(fo, cstats);
    put(fo, wfuse); put(fo, wcull); put(fo, state); put(fo, woff);
    fwrite(&threw, 4, 1, fo);
    fclose(fi);
    fclose(fo);
    vslam_ctx_destroy(ctx);
    return 0;
}
