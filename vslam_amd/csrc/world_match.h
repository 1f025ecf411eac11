// One match of a world step under the step's R, t (include/vslam_amd.h, "the world frame": in range, usable): what the step kernel
// (world.hip) and the resection behind it (resect.hip) both read a match as.  f64, never fused.
#pragma once

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

struct VsWorldMatch {
    bool usable;   // in range, X and Y finite and in front of both cameras
    int first, second;
    double X[3], Y[3];
};

__device__ __forceinline__ VsWorldMatch vs_world_load_match(const int2 *__restrict__ M, const float4 *__restrict__ P, int k, int nl,
                                                            int nc, const double *R, const double *t) {
    VsWorldMatch m;
    const int2 mt = M[k];
    m.first = mt.x;
    m.second = mt.y;
    m.usable = false;
    if (!(mt.x >= 0 && mt.x < nl && mt.y >= 0 && mt.y < nc)) return m;   // keypoints the frames hold
    const float4 p = P[k];   // the stored w is not read
    m.X[0] = (double)p.x; m.X[1] = (double)p.y; m.X[2] = (double)p.z;
#pragma unroll
    for (int r = 0; r < 3; r++) m.Y[r] = ((R[3 * r] * m.X[0] + R[3 * r + 1] * m.X[1]) + R[3 * r + 2] * m.X[2]) + t[r];
    m.usable = isfinite(m.X[0]) && isfinite(m.X[1]) && isfinite(m.X[2]) && isfinite(m.Y[0]) && isfinite(m.Y[1]) &&
               isfinite(m.Y[2]) && m.X[2] > 0.0 && m.Y[2] > 0.0;
    return m;
}
