// The lane-independent part of the world frame's scale selection (world.hip): how a link's ratio becomes an integer key, which
// rank is chosen, and how one radix pass narrows the search.  Compiled by the kernel and by tests/native/world_select_check.cpp,
// which runs the same functions serially on the host against a sort.
//
// q = |carry|^2 / |X|^2 is a non-negative double; non-negative doubles order as their bit patterns, so the element of rank k is
// found over u64 keys: eight passes of eight bits from the top, each a 256-bin histogram of the keys that still share the
// prefix chosen so far (integer counts: the order in which lanes add to them cannot show).
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define WS_HD __host__ __device__ __forceinline__
#else
#define WS_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr uint64_t kWsNoKey = ~0ull;   // not a link; no finite double has these bits
constexpr int kWsPasses = 8, kWsBins = 256;

WS_HD uint64_t ws_bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

WS_HD double ws_value(uint64_t key) {
    double v;
    memcpy(&v, &key, 8);
    return v;
}

WS_HD double ws_norm2(const double v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }

// the key of a link's ratio, or kWsNoKey when the ratio is not finite (an overflowed square, |X|^2 underflowed to 0)
WS_HD uint64_t ws_link_key(const double carry[3], const double X[3]) {
    const double q = ws_norm2(carry) / ws_norm2(X);
    if (!(q >= 0.0 && q <= 1.7976931348623157e308)) return kWsNoKey;   // NaN compares false
    return ws_bits(q) & 0x7FFFFFFFFFFFFFFFull;
}

// the LOWER median of L >= 1 values: rank (L - 1) / 2 in ascending order
WS_HD uint32_t ws_rank(uint32_t L) { return (L - 1u) / 2u; }

WS_HD uint32_t ws_digit(uint64_t key, int pass) { return (uint32_t)(key >> (56 - 8 * pass)) & 255u; }

// does `key` still share the top 8 * pass bits of `prefix`?
WS_HD bool ws_in_prefix(uint64_t key, uint64_t prefix, int pass) {
    if (key == kWsNoKey) return false;
    if (pass == 0) return true;
    const int sh = 64 - 8 * pass;
    return (key >> sh) == (prefix >> sh);
}

// One pass decided: hist[d] = keys in the prefix whose digit is d, `rank` the rank wanted among them.  Appends the digit that
// holds that rank to the prefix and makes the rank relative to it.
WS_HD void ws_pick(const uint32_t *hist, int pass, uint32_t *rank, uint64_t *prefix) {
    uint32_t below = 0, d = 0;
    for (; d < (uint32_t)kWsBins - 1u; d++) {
        const uint32_t c = hist[d];
        if (*rank < below + c) break;
        below += c;
    }
    *rank -= below;
    *prefix |= (uint64_t)d << (56 - 8 * pass);
}
