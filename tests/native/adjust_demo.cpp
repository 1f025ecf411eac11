// Uses the C++ surfaces of the window adjustment the way a consumer of include/vslam/*.h would, and dumps what they give so that
// tests/test_gpu_adjust.py can hold it to the C entry points' bits:
//   vslam::adjust_windows (include/vslam/helpers.h) on one item a caller already holds on the device, then
//   vslam::World::adjust (include/vslam/World.h) on a world attached to a map at frame 0 -- one camera, nothing to move: the call
//   is taken and leaves (0, NaN, NaN, NaN) per track -- and on a world that is not attached, which throws.
//
// usage: adjust_demo <in.bin> <out.bin>
//   in:  K [9] f32; int32 C, N, M; R [C][9], T [C][3], X [N][3] f64; int32 off [N + 1], cam [M]; xy [M][2] f32
//   out: R [C][9], T [C][3], X [N][3], stats [4] f64 of the item; stats [2][4] f64 of the attached world; int32 1 when the
//        unattached world threw
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "vslam/World.h"
#include "vslam/helpers.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    float k[9];
    int h[3];
    if (fread(k, 4, 9, fi) != 9 || fread(h, 4, 3, fi) != 3 || h[0] <= 0 || h[1] <= 0 || h[2] <= 0) return 3;
    const int C = h[0], N = h[1], M = h[2];
    cv::Mat K(3, 3, CV_32FC1);
    for (int r = 0; r < 3; r++) std::memcpy(K.ptr<float>(r), k + 3 * r, 12);
    std::vector<double> R(9 * (size_t)C), T(3 * (size_t)C), X(3 * (size_t)N), st(4);
    std::vector<int> off((size_t)N + 1), cam((size_t)M);
    std::vector<float> xy(2 * (size_t)M);
    if (fread(R.data(), 8, R.size(), fi) != R.size() || fread(T.data(), 8, T.size(), fi) != T.size() || fread(X.data(), 8, X.size(), fi) != X.size() ||
        fread(off.data(), 4, off.size(), fi) != off.size() || fread(cam.data(), 4, cam.size(), fi) != cam.size() ||
        fread(xy.data(), 4, xy.size(), fi) != xy.size())
        return 3;
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    void *d_R, *d_T, *d_X, *d_nc, *d_n, *d_off, *d_cam, *d_xy, *d_st;
    if (vslam_dev_alloc(ctx, 8 * R.size(), &d_R) || vslam_dev_alloc(ctx, 8 * T.size(), &d_T) || vslam_dev_alloc(ctx, 8 * X.size(), &d_X) ||
        vslam_dev_alloc(ctx, 4, &d_nc) || vslam_dev_alloc(ctx, 4, &d_n) || vslam_dev_alloc(ctx, 4 * off.size(), &d_off) ||
        vslam_dev_alloc(ctx, 4 * cam.size(), &d_cam) || vslam_dev_alloc(ctx, 4 * xy.size(), &d_xy) || vslam_dev_alloc(ctx, 64, &d_st))
        return 5;
    if (vslam_copy_h2d(ctx, d_R, R.data(), 8 * R.size()) || vslam_copy_h2d(ctx, d_T, T.data(), 8 * T.size()) ||
        vslam_copy_h2d(ctx, d_X, X.data(), 8 * X.size()) || vslam_copy_h2d(ctx, d_nc, &C, 4) || vslam_copy_h2d(ctx, d_n, &N, 4) ||
        vslam_copy_h2d(ctx, d_off, off.data(), 4 * off.size()) || vslam_copy_h2d(ctx, d_cam, cam.data(), 4 * cam.size()) ||
        vslam_copy_h2d(ctx, d_xy, xy.data(), 4 * xy.size()))
        return 6;
    vslam::adjust_windows(ctx, (f64 *)d_R, (f64 *)d_T, (const s32 *)d_nc, C, (f64 *)d_X, (const s32 *)d_n, N, (const s32 *)d_off,
                          (const s32 *)d_cam, (const float *)d_xy, M, 1, K, (f64 *)d_st);
    if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
    if (vslam_copy_d2h(ctx, R.data(), d_R, 8 * R.size()) || vslam_copy_d2h(ctx, T.data(), d_T, 8 * T.size()) ||
        vslam_copy_d2h(ctx, X.data(), d_X, 8 * X.size()) || vslam_copy_d2h(ctx, st.data(), d_st, 32))
        return 7;
    fwrite(R.data(), 8, R.size(), fo);
    fwrite(T.data(), 8, T.size(), fo);
    fwrite(X.data(), 8, X.size(), fo);
    fwrite(st.data(), 8, 4, fo);

    const int tracks = 2, frames = 3, kp = 16;
    std::vector<double> ws(8, 7.0);
    int threw = 0;
    {
        vslam_map *map = nullptr;
        if (vslam_map_create(ctx, tracks, frames, kp, 32, 64, &map) != VSLAM_OK) return 8;
        void *d_kxy;
        if (vslam_dev_alloc(ctx, 8 * (size_t)tracks * frames * kp, &d_kxy)) return 5;
        {
            vslam::World world(ctx, tracks, frames, kp), loose(ctx, tracks, frames, kp);
            world.attach_to(map);
            world.adjust(map, (const float *)d_kxy, frames, k, 8, nullptr, (double *)d_st);
            if (vslam_ctx_synchronize(ctx) != VSLAM_OK || vslam_copy_d2h(ctx, ws.data(), d_st, 64)) return 7;
            try {
                loose.adjust(map, (const float *)d_kxy, frames, k);
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            vslam_map_destroy(map);
        }
        vslam_dev_free(ctx, d_kxy);
    }
    fwrite(ws.data(), 8, 8, fo);
    fwrite(&threw, 4, 1, fo);
    for (void *p : {d_R, d_T, d_X, d_nc, d_n, d_off, d_cam, d_xy, d_st}) vslam_dev_free(ctx, p);
    vslam_ctx_destroy(ctx);
    fclose(fi);
    fclose(fo);
    return 0;
}
