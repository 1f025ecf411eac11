// What decides something in the geometric fusing (include/vslam_fuse_project.h) beyond the search's and the fusion's own rules and
// does not know about lanes: which points and cameras take part, which pairs are tried, and the word a pair's proposal is kept
// in.  Visibility, the disc, the Hamming distance, the choice and the key are search_math.h's; a valid entry and a sound offset
// are fuse_math.h's.  Compiled for the device by fuse_project.hip and for the host by tests/native/fuse_project_serial.cpp.
#pragma once

#include <cmath>
#include <cstdint>

#include "fuse_math.h"
#include "search_math.h"

namespace vs_fuse_project {
using vs_lm::LmCam;

constexpr int32_t kFpNoHolder = 0x7F7F7F7F;                       // what the fill (bytes of 0x7F) leaves in a holder's cell
constexpr unsigned long long kFpNoKey = 0x7F7F7F7F7F7F7F7Full;    // and in a key: above every (d0 <= 256, i)

// rule 1
LM_FN bool fp_point_part(float px, float py, float pz, int o0, int o1, int obs_stride) {
    return o0 >= 0 && o0 < o1 && o1 <= obs_stride && std::isfinite(px) && std::isfinite(py) && std::isfinite(pz);
}

// rule 2: cam is camera c's pose; mask the item's d_cam_mask or null
LM_FN bool fp_cam_part(const LmCam &cam, int c, int C, const int32_t *mask) {
    return c < C && vs_lm::lm_finite(cam) && (!mask || mask[c] >= 0);
}

// rule 3: the row o0 .. o1 - 1 (of a point that takes part) holds a valid entry of camera c < cam_stride
LM_FN bool fp_seen(const int32_t *obs_cam, const int32_t *obs_kp, int o0, int o1, int c, int kp_stride) {
    bool seen = false;
    for (int o = o0; o < o1; o++) seen = seen || (obs_cam[o] == c && obs_kp[o] >= 0 && obs_kp[o] < kp_stride);
    return seen;
}

// a pair's proposal in one word: k0 (< 16384) in bits 0 .. 13, d0 (<= 256) in bits 14 .. 22, three flags above
constexpr int32_t kFpTried = 1 << 24, kFpVisible = 1 << 25, kFpProposes = 1 << 26;

LM_FN int32_t fp_pack(bool tried, bool visible, bool proposes, uint32_t k0, uint32_t d0) {
    return (tried ? kFpTried : 0) | (visible ? kFpVisible : 0) | (proposes ? (int32_t)(kFpProposes | (d0 << 14) | k0) : 0);
}
LM_FN int fp_k0(int32_t w) { return w & 0x3FFF; }
LM_FN int fp_d0(int32_t w) { return (w >> 14) & 0x1FF; }
}  // namespace vs_fuse_project
