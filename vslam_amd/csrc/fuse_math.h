// What decides something in the fusion and the cull (include/vslam_fuse.h) and does not know about lanes: which observations and
// CSR rows count, the per-observation test of the cull and a point's verdict.  The projection is lm_math.h's, as the resection's
// and the search's.  Compiled for the device by fuse.hip and for the host by tests/native/fuse_serial.cpp.  All f64, never fused
// (compile host code with -ffp-contract=off); the fusion is integers only.
#pragma once

#include <cmath>
#include <cstdint>

#include "lm_math.h"

namespace vs_fuse {
using vs_lm::LmCam;

struct FuCull {
    double r2;   // inlier_px * inlier_px, one product
    int32_t min_good, mature_good, mature_age, good10;
};

LM_FN FuCull fu_cull(double inlier_px, int32_t min_good, int32_t mature_good, int32_t mature_age, int32_t good10) {
    FuCull p;
    p.r2 = inlier_px * inlier_px;
    p.min_good = min_good;
    p.mature_good = mature_good;
    p.mature_age = mature_age;
    p.good10 = good10;
    return p;
}

// the fusion's VALID observation
LM_FN bool fu_valid(int cam, int kp, int cam_stride, int kp_stride) { return cam >= 0 && cam < cam_stride && kp >= 0 && kp < kp_stride; }

// offsets[i] of a sound CSR, given its predecessor (prev = 0 for i = 0)
LM_FN bool fu_offset_ok(int prev, int cur, int obs_stride) { return cur >= prev && cur >= 0 && cur <= obs_stride; }

// GOOD of a usable observation: camera c, point P, keypoint (x, y)
LM_FN bool fu_good(const double (&K)[9], const LmCam &c, const double (&P)[3], float x, float y, double r2) {
    double RP[3], Y[3], u, v, q2;
    vs_lm::lm_transform(c.R, c.T, P, RP, Y);
    if (!(Y[2] > 0.0)) return false;
    vs_lm::lm_project(K, Y, u, v, q2);
    if (!(std::isfinite(u) && std::isfinite(v))) return false;
    const double r0 = u - (double)x, r1 = v - (double)y;
    return r0 * r0 + r1 * r1 <= r2;
}

LM_FN bool fu_kept(int n_usable, int n_good, int last, int C, const FuCull &p) {
    const int need = last + p.mature_age < C ? p.mature_good : p.min_good;
    return n_good >= need && 10 * n_good >= p.good10 * n_usable;
}

// One point of the cull: 1 kept, 0 culled, -1 took no part.  obs_cam / obs_kp: the item's rows; R [cam_stride][9], T [cam_stride][3],
// xy [cam_stride][kp_stride][2]: the item's cameras, C <= cam_stride of them.
LM_FN int fu_cull_point(const double (&K)[9], float px, float py, float pz, int o0, int o1, int obs_stride, const int32_t *obs_cam,
                        const int32_t *obs_kp, int C, int kp_stride, const double *R, const double *T, const float *xy, const FuCull &p,
                        int &n_usable, int &n_good) {
    n_usable = 0;
    n_good = 0;
    if (!(o0 >= 0 && o0 < o1 && o1 <= obs_stride)) return -1;
    if (!(std::isfinite(px) && std::isfinite(py) && std::isfinite(pz))) return -1;
    const double P[3] = {(double)px, (double)py, (double)pz};
    int last = -1;
    for (int o = o0; o < o1; o++) {
        const int cam = obs_cam[o], kp = obs_kp[o];
        if (!fu_valid(cam, kp, C, kp_stride)) continue;
        LmCam c;
#pragma unroll
        for (int k = 0; k < 9; k++) c.R[k] = R[(size_t)cam * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; k++) c.T[k] = T[(size_t)cam * 3 + k];
        if (!vs_lm::lm_finite(c)) continue;
        const float x = xy[((size_t)cam * kp_stride + kp) * 2], y = xy[((size_t)cam * kp_stride + kp) * 2 + 1];
        if (!(std::isfinite(x) && std::isfinite(y))) continue;
        n_usable++;
        last = cam > last ? cam : last;
        n_good += fu_good(K, c, P, x, y, p.r2) ? 1 : 0;
    }
    return fu_kept(n_usable, n_good, last, C, p) ? 1 : 0;
}
}  // namespace vs_fuse
