// Uses the C++ surfaces of the resection the way a consumer of include/vslam/*.h would, and dumps what they give so that
// tests/test_gpu_resect.py can hold it to the C entry points' bits:
//   vslam::resect_poses (include/vslam/helpers.h) on one item a caller already holds on the device, then
//   vslam::World (include/vslam/World.h) with set_resection(), stepped by hand with step_resect on one track's script.
//
// usage: resect_demo <in.bin> <out.bin>
//   in:  K [9] f32; int32 n; P [n][3] f64; x [n][2] f32; R [9] f64; T [3] f64;
//        int32 kp_stride, steps; per step: int32 n; R [9] f32; t [3] f32; matches [n][2] i32; X [n][4] f32; xy_cur [kp_stride][2] f32
//   out: R [9], T [3], stats [4] f64 of the item; Twc [frames][16] f64; pose [frames][16] f32; scale [frames] f64;
//        links [frames] i32; resection stats [frames][4] f64
#include <cstdio>
#include <cstring>
#include <vector>

#include "vslam/World.h"
#include "vslam/helpers.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    float k[9];
    int n = 0;
    if (fread(k, 4, 9, fi) != 9 || fread(&n, 4, 1, fi) != 1 || n <= 0) return 3;
    cv::Mat K(3, 3, CV_32FC1);
    for (int r = 0; r < 3; r++) std::memcpy(K.ptr<float>(r), k + 3 * r, 12);
    std::vector<double> pts(3 * (size_t)n), RT(12), out(16);
    std::vector<float> x(2 * (size_t)n);
    if (fread(pts.data(), 8, pts.size(), fi) != pts.size() || fread(x.data(), 4, x.size(), fi) != x.size() || fread(RT.data(), 8, 12, fi) != 12) return 3;
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx) != VSLAM_OK) return 4;
    void *d_P, *d_x, *d_n, *d_R, *d_T, *d_st;
    if (vslam_dev_alloc(ctx, 24 * (size_t)n, &d_P) || vslam_dev_alloc(ctx, 8 * (size_t)n, &d_x) || vslam_dev_alloc(ctx, 4, &d_n) ||
        vslam_dev_alloc(ctx, 72, &d_R) || vslam_dev_alloc(ctx, 24, &d_T) || vslam_dev_alloc(ctx, 32, &d_st))
        return 5;
    if (vslam_copy_h2d(ctx, d_P, pts.data(), 24 * (size_t)n) || vslam_copy_h2d(ctx, d_x, x.data(), 8 * (size_t)n) ||
        vslam_copy_h2d(ctx, d_n, &n, 4) || vslam_copy_h2d(ctx, d_R, RT.data(), 72) || vslam_copy_h2d(ctx, d_T, RT.data() + 9, 24))
        return 6;
    vslam::resect_poses(ctx, (const f64 *)d_P, (const float *)d_x, (const s32 *)d_n, 1, n, K, (f64 *)d_R, (f64 *)d_T, (f64 *)d_st);
    if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;
    if (vslam_copy_d2h(ctx, out.data(), d_R, 72) || vslam_copy_d2h(ctx, out.data() + 9, d_T, 24) || vslam_copy_d2h(ctx, out.data() + 12, d_st, 32))
        return 7;
    fwrite(out.data(), 8, 16, fo);
    for (void *p : {d_P, d_x, d_n, d_R, d_T, d_st}) vslam_dev_free(ctx, p);

    int hdr[2];
    if (fread(hdr, 4, 2, fi) != 2) return 3;
    const int Kp = hdr[0], steps = hdr[1], frames = steps + 1;
    void *d_m, *d_best, *d_X, *d_Rf, *d_t, *d_nl, *d_nc, *d_xy;
    if (vslam_dev_alloc(ctx, 8 * (size_t)Kp, &d_m) || vslam_dev_alloc(ctx, 16, &d_best) || vslam_dev_alloc(ctx, 16 * (size_t)Kp, &d_X) ||
        vslam_dev_alloc(ctx, 36, &d_Rf) || vslam_dev_alloc(ctx, 12, &d_t) || vslam_dev_alloc(ctx, 4, &d_nl) ||
        vslam_dev_alloc(ctx, 4, &d_nc) || vslam_dev_alloc(ctx, 8 * (size_t)Kp, &d_xy))
        return 5;
    std::vector<double> Twc((size_t)frames * 16), scale((size_t)frames), stats((size_t)frames * 4);
    std::vector<float> pose((size_t)frames * 16);
    std::vector<int> links((size_t)frames);
    {
        vslam::World world(ctx, 1, frames, Kp);
        if (world.resection_stats() != nullptr) return 8;
        world.set_resection();
        for (int s = 0; s < steps; s++) {
            int m_n = 0;
            float R[9], t[3];
            if (fread(&m_n, 4, 1, fi) != 1 || m_n < 0 || m_n > Kp || fread(R, 4, 9, fi) != 9 || fread(t, 4, 3, fi) != 3) return 3;
            std::vector<int> m(2 * (size_t)Kp, 0);
            std::vector<float> X(4 * (size_t)Kp, 0.f), xy(2 * (size_t)Kp);
            if (m_n && (fread(m.data(), 8, (size_t)m_n, fi) != (size_t)m_n || fread(X.data(), 16, (size_t)m_n, fi) != (size_t)m_n)) return 3;
            if (fread(xy.data(), 8, (size_t)Kp, fi) != (size_t)Kp) return 3;
            const int best[4] = {0, m_n, 0, m_n};
            if (vslam_copy_h2d(ctx, d_m, m.data(), 8 * (size_t)Kp) || vslam_copy_h2d(ctx, d_best, best, 16) ||
                vslam_copy_h2d(ctx, d_X, X.data(), 16 * (size_t)Kp) || vslam_copy_h2d(ctx, d_Rf, R, 36) || vslam_copy_h2d(ctx, d_t, t, 12) ||
                vslam_copy_h2d(ctx, d_nl, &Kp, 4) || vslam_copy_h2d(ctx, d_nc, &Kp, 4) || vslam_copy_h2d(ctx, d_xy, xy.data(), 8 * (size_t)Kp))
                return 6;
            world.step_resect((const int32_t *)d_m, (const int32_t *)d_best, (const float *)d_X, (const float *)d_Rf, (const float *)d_t,
                              (const int32_t *)d_nl, (const int32_t *)d_nc, (const float *)d_xy, k);
            if (vslam_ctx_synchronize(ctx) != VSLAM_OK) return 7;   // the host arrays above are reused
        }
        const vslam_world_arrays a = world.view();
        if (a.frames != frames) return 7;
        if (vslam_copy_d2h(ctx, Twc.data(), a.d_Twc, 128 * (size_t)frames) || vslam_copy_d2h(ctx, pose.data(), a.d_pose, 64 * (size_t)frames) ||
            vslam_copy_d2h(ctx, scale.data(), a.d_scale, 8 * (size_t)frames) || vslam_copy_d2h(ctx, links.data(), a.d_links, 4 * (size_t)frames) ||
            vslam_copy_d2h(ctx, stats.data(), world.resection_stats(), 32 * (size_t)frames))
            return 7;
    }
    for (void *p : {d_m, d_best, d_X, d_Rf, d_t, d_nl, d_nc, d_xy}) vslam_dev_free(ctx, p);
    vslam_ctx_destroy(ctx);
    fwrite(Twc.data(), 8, Twc.size(), fo);
    fwrite(pose.data(), 4, pose.size(), fo);
    fwrite(scale.data(), 8, scale.size(), fo);
    fwrite(links.data(), 4, links.size(), fo);
    fwrite(stats.data(), 8, stats.size(), fo);
    fclose(fi);
    fclose(fo);
    return 0;
}
