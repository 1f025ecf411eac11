// The winner's key of vslam_pnp_ransac (vslam_amd/csrc/pnp_math.h: pn_key) checked exhaustively on the host: a larger count wins
// whatever the pose indices; at an equal count the smaller 4 h + s wins -- between hypotheses and between the slots of one
// hypothesis --; count and pose come back out of the key; no pose (-1) is below every key of a pose that counts anything.
// Prints "ok" and returns 0, or the first violation and 1.  tests/test_pnp_serial.py builds and runs it.
#include <cstdio>

#include "../../vslam_amd/csrc/pnp_math.h"

using namespace vs_pnp;

int main() {
    const int counts[] = {0, 1, 3, 4, 7, 8, 255, 256, 4095, 4096, 16383, 16384};
    for (int c : counts) {
        for (int p = 0; p < kPnMaxPoses; p++) {
            const uint32_t k = pn_key(c, p);
            if (pn_key_count(k) != c || pn_key_pose(k) != p) return printf("round trip %d %d\n", c, p), 1;
            if (p + 1 < kPnMaxPoses && !(k > pn_key(c, p + 1))) return printf("tie %d: %d against %d\n", c, p, p + 1), 1;   // s and h alike
            if (c > 0 && !(k > pn_key(-1, p))) return printf("no pose %d %d\n", c, p), 1;
        }
    }
    for (size_t i = 0; i + 1 < sizeof(counts) / sizeof(counts[0]); i++) {
        if (!(pn_key(counts[i + 1], kPnMaxPoses - 1) > pn_key(counts[i], 0))) return printf("count %d against %d\n", counts[i + 1], counts[i]), 1;
    }
    // the slots of one hypothesis at an equal count: 4 h + 0 beats 4 h + 1 .. 3, and 4 h + 3 beats 4 (h + 1) + 0
    for (int h = 0; h + 1 < kPnMaxPoses / 4; h++) {
        for (int s = 0; s < 3; s++)
            if (!(pn_key(40, 4 * h + s) > pn_key(40, 4 * h + s + 1))) return printf("slot %d %d\n", h, s), 1;
        if (!(pn_key(40, 4 * h + 3) > pn_key(40, 4 * (h + 1)))) return printf("hypothesis %d\n", h), 1;
    }
    if (pn_key(-1, 0) != 0u) return printf("no pose is not 0\n"), 1;
    printf("ok\n");
    return 0;
}
