// What decides something in place recognition (include/vslam_places.h) and does not know about lanes: the distance and the rule of
// assignment, the float key the matrix-core kernel keeps and what it decodes to, where training starts, the majority vote, a weight
// as the index keeps it, a score's term and the order of candidates.  Compiled for the device by places.hip and for the host by
// tests/native/places_serial.cpp.  Integers throughout; the one float, the key, holds an integer below 2^23 exactly.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PL_FN __host__ __device__ __forceinline__
#else
#define PL_FN inline
#endif

namespace vs_places {

constexpr int kPlMaxWords = 16384;
constexpr float kPlKeyScale = 16384.f;   // kPlMaxWords: the word occupies the low 14 bits of a key

PL_FN int pl_popc(uint32_t x) {
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (int)((((x + (x >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
}

// differing bits of two 256-bit rows given as 8 dwords
PL_FN int pl_dist(const uint32_t *a, const uint32_t *b) {
    int d = 0;
    for (int k = 0; k < 8; k++) d += pl_popc(a[k] ^ b[k]);
    return d;
}

// (dist, w) comes before the best so far: smaller distance, then the lower word
PL_FN bool pl_closer(int dist, int w, int best_dist, int best_w) { return dist < best_dist || (dist == best_dist && w < best_w); }

// The matrix-core form of the same rule.  dot = 256 - 2 dist; key = dot x 16384 - w, largest first.  |key| < 2^23: exact in f32.
PL_FN float pl_key(int dist, int w) { return (float)(256 - 2 * dist) * kPlKeyScale - (float)w; }
PL_FN void pl_key_decode(int key, int &dist, int &w) {
    const int dot = (key + (kPlMaxWords - 1)) >> 14;   // ceil (arithmetic shift: floor)
    w = dot * kPlMaxWords - key;
    dist = (256 - dot) >> 1;
}

// training starts word w at this descriptor
PL_FN int pl_start(int w, int n, int n_words) { return (int)(((int64_t)w * (int64_t)n) / (int64_t)n_words); }

// a word's bit from the votes of its members (members > 0); a tie gives 0
PL_FN bool pl_majority(int ones, int members) { return 2 * ones > members; }

PL_FN int pl_weight(int w) { return w < 0 ? 0 : (w > 65535 ? 65535 : w); }

PL_FN int pl_term(int weight, int tf_q, int tf_e) { return weight * (tf_q < tf_e ? tf_q : tf_e); }

// candidate a (score, den, id) comes before b; every factor is below 2^31 (include/vslam_places.h, PROOF OF THE BOUND)
PL_FN bool pl_before(int sa, int da, int ia, int sb, int db, int ib) {
    const uint64_t l = (uint64_t)(uint32_t)sa * (uint64_t)(uint32_t)db, r = (uint64_t)(uint32_t)sb * (uint64_t)(uint32_t)da;
    return l > r || (l == r && ia < ib);
}

}  // namespace vs_places
