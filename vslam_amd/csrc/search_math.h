// What decides something in the search by projection (include/vslam_search.h) and does not know about lanes: visibility, the
// disc test, the Hamming distance, the (d, k) and (d, i) orders, the ratio rule, the proposal key and the grid's cell of a
// coordinate.  Compiled for the device by search.hip and for the host by tests/native/search_serial.cpp.  All f64, never fused
// (compile host code with -ffp-contract=off); everything behind the disc test is integers.
#pragma once

#include <cmath>
#include <cstdint>

#include "lm_math.h"

namespace vs_search {
using vs_lm::LmCam;

constexpr uint32_t kSsNone = 0xFFFFFFFFu;               // no distance
constexpr unsigned long long kSsNoKey = ~0ull;          // a keypoint nobody proposed to
constexpr int kSsMaxCells = 64;                         // cells per axis at the most
constexpr double kSsMargin = 0x1p-10;                   // pixels by which the walked window exceeds the radius on every side

struct SsParams {
    double radius, r2;   // r2 = radius * radius, one product
    int32_t dist_threshold, ratio10;
};

LM_FN SsParams ss_params(double radius, int32_t dist_threshold, int32_t ratio10) {
    SsParams p;
    p.radius = radius;
    p.r2 = radius * radius;
    p.dist_threshold = dist_threshold;
    p.ratio10 = ratio10;
    return p;
}

// rule 1: (u, v) of a visible point; cam_ok = the item's R and T are finite
LM_FN bool ss_visible(const double (&K)[9], const LmCam &cam, bool cam_ok, float px, float py, float pz, int o0, int o1, int obs_stride,
                      int width, int height, double &u, double &v) {
    if (!cam_ok) return false;
    if (!(o0 >= 0 && o0 < o1 && o1 <= obs_stride)) return false;
    if (!(std::isfinite(px) && std::isfinite(py) && std::isfinite(pz))) return false;
    const double P[3] = {(double)px, (double)py, (double)pz};
    double RP[3], Y[3], q2;
    vs_lm::lm_transform(cam.R, cam.T, P, RP, Y);
    if (!(std::isfinite(Y[0]) && std::isfinite(Y[1]) && std::isfinite(Y[2]) && Y[2] > 0.0)) return false;
    vs_lm::lm_project(K, Y, u, v, q2);
    if (!(std::isfinite(u) && std::isfinite(v))) return false;
    return u >= 0.0 && u < (double)width && v >= 0.0 && v < (double)height;
}

// rule 2: the closed disc
LM_FN bool ss_in_disc(float x, float y, double u, double v, double r2) {
    if (!(std::isfinite(x) && std::isfinite(y))) return false;
    const double dx = (double)x - u, dy = (double)y - v;
    return dx * dx + dy * dy <= r2;
}

LM_FN uint32_t ss_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}

// 256-bit Hamming distance of two descriptors held as 8 words
LM_FN uint32_t ss_ham256(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) d += ss_popc(a[w] ^ b[w]);
    return d;
}

// rule 3: the running choice of a point over its candidates, in any order
struct SsBest {
    uint32_t d0 = kSsNone, k0 = kSsNone, d1 = kSsNone;
};

LM_FN void ss_offer(SsBest &b, uint32_t d, uint32_t k) {
    if (d < b.d0 || (d == b.d0 && k < b.k0)) {   // (d, k) < (d0, k0): the old best becomes one of the others
        b.d1 = b.d0;                             // d0 <= every other d seen, so it is their minimum (kSsNone when there was none)
        b.d0 = d;
        b.k0 = k;
    } else if (d < b.d1) {
        b.d1 = d;
    }
}

LM_FN bool ss_proposes(const SsBest &b, const SsParams &p) {
    if (b.d0 == kSsNone || !((int32_t)b.d0 < p.dist_threshold)) return false;
    return p.ratio10 == 0 || b.d1 == kSsNone || 10 * (int32_t)b.d0 < p.ratio10 * (int32_t)b.d1;
}

// rule 4: the smallest key wins a keypoint
LM_FN unsigned long long ss_key(uint32_t d0, uint32_t i) { return ((unsigned long long)d0 << 32) | i; }

// The grid: square cells of side c >= radius + 2 margins and >= the image's longer side / 64, at most 64 x 64 of them.  A
// coordinate's cell is monotone in the coordinate (a product with a positive constant, a floor, a clamp), and keypoints outside
// the image are clamped into the border cells, so the cells ss_cell(u - radius - margin) .. ss_cell(u + radius + margin) hold every
// keypoint whose coordinate lies inside that window, wherever the cell borders fall; the margin is far above the rounding of the
// disc test's f64 arithmetic on coordinates of this size.  Which keypoints are candidates is decided by ss_in_disc alone.
struct SsGrid {
    double inv_c;
    int nx, ny;
};

LM_FN SsGrid ss_grid(int width, int height, double radius) {
    const double longer = (double)(width > height ? width : height);
    const double c = fmax(radius + 2.0 * kSsMargin, longer / (double)kSsMaxCells);
    SsGrid g;
    g.inv_c = 1.0 / c;
    const double fx = floor((double)width * g.inv_c) + 1.0, fy = floor((double)height * g.inv_c) + 1.0;
    g.nx = fx < (double)kSsMaxCells ? (int)fx : kSsMaxCells;
    g.ny = fy < (double)kSsMaxCells ? (int)fy : kSsMaxCells;
    return g;
}

LM_FN int ss_cell(double x, double inv_c, int n) {   // x finite
    const double t = floor(x * inv_c);
    return t < 0.0 ? 0 : t > (double)(n - 1) ? n - 1 : (int)t;
}
}  // namespace vs_search
