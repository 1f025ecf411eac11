// Uses the two C++ additions around the refit of the RANSAC winner the way a consumer of include/vslam/*.h would:
// RansacFilter::refit_fundamental on host vectors (F refitted in place over the flagged matches), and vslam::refit_fundamental
// on arrays a caller already holds on the device.  Dumps both results so the Python test can hold them to the C entry point.
//
// usage: refit_demo <in.bin> <out.bin>
//   in.bin:  int32 K, n; xy1 [K][2] f32; xy2 [K][2] f32; matches [n][2] int32; flags [n] u8; F [9] f32
//   out.bin: F [9] f32 from RansacFilter::refit_fundamental, then F [9] f32 from vslam::refit_fundamental
#include <cstdio>
#include <vector>

#include "vslam/RansacFilter.h"
#include "vslam/helpers.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    int hdr[2];
    if (!fi || fread(hdr, 4, 2, fi) != 2) return 3;
    const int K = hdr[0], n = hdr[1];
    std::vector<cv::Point2f> p1(K), p2(K);
    std::vector<int> flat(2 * (size_t)n);
    std::vector<unsigned char> flags(n);
    float F[9];
    if (fread(p1.data(), 8, K, fi) != (size_t)K || fread(p2.data(), 8, K, fi) != (size_t)K) return 3;
    if (fread(flat.data(), 8, n, fi) != (size_t)n || fread(flags.data(), 1, n, fi) != (size_t)n || fread(F, 4, 9, fi) != 9) return 3;
    fclose(fi);

    std::vector<std::pair<int, int>> matches(n);
    std::vector<bool> inliers(n);
    for (int i = 0; i < n; i++) {
        matches[i] = {flat[2 * i], flat[2 * i + 1]};
        inliers[i] = flags[i] != 0;
    }
    cv::Mat fundamental(3, 3, CV_32FC1);
    for (int i = 0; i < 9; i++) fundamental.ptr<float>(i / 3)[i % 3] = F[i];
    RansacFilter rf(8, 16, 10);
    rf.refit_fundamental(p1, p2, matches, inliers, fundamental);

    // the device form: the compacted inlier matches and d_best as RANSAC would have left them
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    std::vector<int> kept(2 * (size_t)K, -1);
    int k = 0;
    for (int i = 0; i < n; i++)
        if (inliers[i]) {
            kept[2 * k] = flat[2 * i];
            kept[2 * k + 1] = flat[2 * i + 1];
            k++;
        }
    const int best[4] = {0, k, 0, k};
    void *d_xy1, *d_xy2, *d_m, *d_best, *d_F;
    float Fd[9];
    if (vslam_dev_alloc(ctx, 8 * (size_t)K, &d_xy1) || vslam_dev_alloc(ctx, 8 * (size_t)K, &d_xy2) || vslam_dev_alloc(ctx, 8 * (size_t)K, &d_m) ||
        vslam_dev_alloc(ctx, 16, &d_best) || vslam_dev_alloc(ctx, 36, &d_F))
        return 5;
    if (vslam_copy_h2d(ctx, d_xy1, p1.data(), 8 * (size_t)K) || vslam_copy_h2d(ctx, d_xy2, p2.data(), 8 * (size_t)K) ||
        vslam_copy_h2d(ctx, d_m, kept.data(), 8 * (size_t)K) || vslam_copy_h2d(ctx, d_best, best, 16) || vslam_copy_h2d(ctx, d_F, F, 36))
        return 6;
    vslam::refit_fundamental(ctx, (const float *)d_xy1, (const float *)d_xy2, (const s32 *)d_m, (const s32 *)d_best, 1, K, (float *)d_F);
    if (vslam_copy_d2h(ctx, Fd, d_F, 36)) return 7;
    for (void *p : {d_xy1, d_xy2, d_m, d_best, d_F}) vslam_dev_free(ctx, p);
    vslam_ctx_destroy(ctx);

    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 8;
    for (int r = 0; r < 3; r++) fwrite(fundamental.ptr<float>(r), 4, 3, fo);
    fwrite(Fd, 4, 9, fo);
    fclose(fo);
    return 0;
}
