// Uses the two C++ surfaces of the two-view bundle adjustment the way a consumer of include/vslam/*.h would:
// vslam::refine_pairs on arrays a caller already holds on the device, and `struct optimizer` (include/vslam/optimizer.h) on host
// matrices.  Dumps both results so the Python test can hold them to the C entry point.
//
// usage: refine_demo <in.bin> <out.bin>
//   in.bin:  int32 n; K [9] f32; xy1 [n][2] f32; xy2 [n][2] f32; R [9] f32; t [3] f32; points [n][4] f32
//   out.bin: R [9], t [3], c2 [12], points [n][4] f32 from vslam::refine_pairs (match i = (i, i)); then R [9], t [3],
//            points [n][4] f32 and stats [4] f64 from optimizer::optimize
#include <cstdio>
#include <vector>

#include "vslam/helpers.h"
#include "vslam/optimizer.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    int n = 0;
    if (!fi || fread(&n, 4, 1, fi) != 1 || n <= 0) return 3;
    const size_t N = (size_t)n;
    float Kf[9], R[9], t[3];
    std::vector<float> xy1(2 * N), xy2(2 * N), pts(4 * N);
    if (fread(Kf, 4, 9, fi) != 9 || fread(xy1.data(), 8, N, fi) != N || fread(xy2.data(), 8, N, fi) != N || fread(R, 4, 9, fi) != 9 ||
        fread(t, 4, 3, fi) != 3 || fread(pts.data(), 16, N, fi) != N)
        return 3;
    fclose(fi);
    cv::Mat K(3, 3, CV_32FC1);
    for (int i = 0; i < 9; i++) K.ptr<float>(i / 3)[i % 3] = Kf[i];

    // the device form
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    std::vector<int> m(2 * N);
    for (int i = 0; i < n; i++) m[2 * i] = m[2 * i + 1] = i;
    const int best[4] = {0, n, 0, n};
    void *d_xy1, *d_xy2, *d_m, *d_best, *d_R, *d_t, *d_c2, *d_pts;
    if (vslam_dev_alloc(ctx, 8 * N, &d_xy1) || vslam_dev_alloc(ctx, 8 * N, &d_xy2) || vslam_dev_alloc(ctx, 8 * N, &d_m) ||
        vslam_dev_alloc(ctx, 16, &d_best) || vslam_dev_alloc(ctx, 36, &d_R) || vslam_dev_alloc(ctx, 12, &d_t) ||
        vslam_dev_alloc(ctx, 48, &d_c2) || vslam_dev_alloc(ctx, 16 * N, &d_pts))
        return 5;
    if (vslam_copy_h2d(ctx, d_xy1, xy1.data(), 8 * N) || vslam_copy_h2d(ctx, d_xy2, xy2.data(), 8 * N) ||
        vslam_copy_h2d(ctx, d_m, m.data(), 8 * N) || vslam_copy_h2d(ctx, d_best, best, 16) || vslam_copy_h2d(ctx, d_R, R, 36) ||
        vslam_copy_h2d(ctx, d_t, t, 12) || vslam_copy_h2d(ctx, d_pts, pts.data(), 16 * N))
        return 6;
    vslam::refine_pairs(ctx, (const float *)d_xy1, (const float *)d_xy2, (const s32 *)d_m, (const s32 *)d_best, 1, n, K, 16.f, 20,
                        (float *)d_R, (float *)d_t, (float *)d_c2, (float *)d_pts);
    float Rd[9], td[3], c2d[12];
    std::vector<float> pd(4 * N);
    if (vslam_copy_d2h(ctx, Rd, d_R, 36) || vslam_copy_d2h(ctx, td, d_t, 12) || vslam_copy_d2h(ctx, c2d, d_c2, 48) ||
        vslam_copy_d2h(ctx, pd.data(), d_pts, 16 * N))
        return 7;
    for (void *p : {d_xy1, d_xy2, d_m, d_best, d_R, d_t, d_c2, d_pts}) vslam_dev_free(ctx, p);
    vslam_ctx_destroy(ctx);

    // the reference's struct
    optimizer opt;
    opt.initial_poses = {cv::Mat(3, 4, CV_32FC1), cv::Mat(3, 4, CV_32FC1)};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            opt.initial_poses[0].ptr<float>(r)[c] = r == c ? 1.f : 0.f;
            opt.initial_poses[1].ptr<float>(r)[c] = c < 3 ? R[3 * r + c] : t[r];
        }
    opt.landmark_priors = cv::Mat(n, 4, CV_32FC1);
    for (int i = 0; i < n; i++) {
        for (int c = 0; c < 4; c++) opt.landmark_priors.ptr<float>(i)[c] = pts[4 * (size_t)i + c];
        opt.measurements.push_back({cv::Point2f(xy1[2 * i], xy1[2 * i + 1]), cv::Point2f(xy2[2 * i], xy2[2 * i + 1])});
    }
    double stats[4];
    opt.optimize(K, 16.f, 20, stats);

    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 8;
    fwrite(Rd, 4, 9, fo); fwrite(td, 4, 3, fo); fwrite(c2d, 4, 12, fo); fwrite(pd.data(), 16, N, fo);
    for (int r = 0; r < 3; r++) fwrite(opt.initial_poses[1].ptr<float>(r), 4, 3, fo);
    for (int r = 0; r < 3; r++) fwrite(opt.initial_poses[1].ptr<float>(r) + 3, 4, 1, fo);
    for (int i = 0; i < n; i++) fwrite(opt.landmark_priors.ptr<float>(i), 4, 4, fo);
    fwrite(stats, 8, 4, fo);
    fclose(fo);
    return 0;
}
