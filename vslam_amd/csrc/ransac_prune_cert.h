// The one-sided certificate of ransac_prune.hip: when a float32 value of the epipolar numerator n and of the first line
// coefficient a0, formed in ANY order of additions, proves that the reference's residual e exceeds the threshold.  Compiled by
// the kernel and by tests/native/prune_cert_check.cpp, which runs the same functions on the host against the oracle.
//
// The reference (RansacFilter.cpp:119-126, restated by residual_e in ransac_residual.h) computes in floats, round to nearest,
//   a_k = (f_3k x1 + f_3k+1 y1) + f_3k+2,   n = (x2 a0 + y2 a1) + a2,   q = (n n) / (a0 a0),   e = ((q + a1 a1) + t0 t0) + t1 t1
// and calls the match an inlier iff e <= thr.  Write n_ref, a0_ref for its floats, and N, A0 for the real numbers
//   N = sum_k F_k phi_k,  phi = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1),   A0 = f0 x1 + f1 y1 + f2.
// u = 2^-24; C1, C2 = the pair's largest |coordinate| in frame 1 / 2; phimax = (C2 C1, C2 C1, C2, C2 C1, C2 C1, C2, C1, C1, 1).
//
// 1. Distances.  A term of n_ref passes at most 6 roundings (f0 x1: product, two additions of a0, the product with x2, two
//    additions of n), so |n_ref - N| <= 6 u' T with T = sum_k |F_k| phimax_k and u' = u (1 + 6u).  The kernel's n~ rounds phi_k
//    once, the product once and at most 8 additions of a 9-term sum (the padding term is an exact zero and adding it rounds
//    nothing); an fma chain rounds less.  So |n~ - N| <= 10 u' T in any order, with or without fma, and
//        |n~ - n_ref| <= 16 u' T.   E = kPcNumer u T with kPcNumer = 18: the 16 counted, and 2 for u' and for forming E itself.
//    This relies on every step of the pipe that forms n~ and a~0 (vector or matrix: v_mfma_f32_32x32x2_f32 is a chain of f32
//    fmas) rounding to nearest with relative error at most u on normal results, and on nothing more for tiny ones: gradual
//    underflow adds at most 2^-149 per step, and a pipe that flushes subnormal inputs or results to zero instead drops at most
//    9 terms, each below 2^-126 as a product, or below 2^-126 2^40 = 2^-86 as a flushed F times a phi <= 2^40.  Either way the
//    absolute error stays below 2^-82, which the 2^-40 in c below covers many times over; the same for a~0.
//    Likewise a0_ref and a~0 pass 3 roundings each:  |a~0 - a0_ref| <= 6 u' T0,  T0 = |f0| C1 + |f1| C1 + |f2|;  E0 = kPcDenom u T0
//    with kPcDenom = 7.
// 2. The comparison.  s+ = sqrt(thr) (1 + 2^-20) rounded to float, c >= (E + s+ E0)(1 + 2^-20) + 2^-40 (pc_margin).
//    A result is a CERTIFIED MISS iff the ordered float comparison  |n~| > fma(s+, |a~0|, c)  is true.  The fma rounds once,
//    and c >= 2^-40 keeps it normal: |n~| > (1 - u)(s+ |a~0| + c).  With 1.:
//        |n_ref| >= |n~| - E > (1 - u) s+ (|a0_ref| - E0) + (1 - u) c - E >= (1 - u) s+ |a0_ref| + (1 - u) 2^-40
//    because (1 - u)(1 + 2^-20)(E + s+ E0) >= E + s+ E0.  (1 - u) s+ >= sqrt(thr)(1 + 2^-21) after the roundings of s+, so
//        n_ref^2 > thr (1 + 2^-20) a0_ref^2     and     |n_ref| > 2^-41.
// 3. From there to e > thr.  |n_ref| > 2^-41 keeps nn = fl(n_ref^2) >= 2^-82 out of the denormals: nn >= n_ref^2 (1 - u).
//    a) dd = fl(a0_ref^2) normal: dd <= a0_ref^2 (1 + u), nn / dd > thr (1 + 2^-20)(1 - u)/(1 + u) > thr (1 + 2^-21), which lies
//       beyond the float after thr; rounding is monotone, so q = fl(nn / dd) > thr (or q = inf).
//    b) dd zero or denormal (< 2^-126): nn / dd > 2^-82 / 2^-126 = 2^44 > 2^20 >= thr: q = inf or huge.
//    e adds three squares to q, each >= 0 or NaN.  fl(q + x) >= q for x >= 0 (monotone rounding, q a float), so without a NaN
//    e >= q > thr; with one, e is NaN and `e <= thr` is false.  Either way the reference does not count the match.
// 4. What must hold for 1. and 3.: nothing overflows before the true value does.  With |f| <= 2^10, coordinates <= 2^20 and
//    thr in [2^-20, 2^20] (the count kernel's stated ranges) |n| < 2^54 and n^2 < 2^108.  Outside them pc_margin returns +inf
//    and no comparison of that hypothesis is true.  A NaN in F fails the range test; and a NaN n~ or a~0 makes the ordered
//    comparison false by itself.  So a hypothesis or pair outside the ranges, or not finite, is never pruned.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define PC_HD __host__ __device__ inline
#else
#define PC_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr double kPcNumer = 18.0, kPcDenom = 7.0;
constexpr double kPcU = 0x1p-24, kPcFloor = 0x1p-40;

// s+ : sqrt(thr)(1 + 2^-20) as a float (two roundings of relative 2^-53 and one of u: inside the 2^-20)
PC_HD float pc_splus(float thr) { return (float)(sqrt((double)thr) * (1.0 + 0x1p-20)); }

// do the pair's figures lie inside the stated ranges?  (false for NaN)
PC_HD bool pc_pair_ok(float C1, float C2, float thr) {
    return thr >= 0x1p-20f && thr <= 0x1p20f && C1 <= 0x1p20f && C2 <= 0x1p20f && C1 >= 0.f && C2 >= 0.f;
}

// c of one hypothesis (see 2.; splus = pc_splus(thr), formed once per launch on the host), +inf when it or the pair lies outside the stated ranges: then nothing of it is certified.
// Formed in float from non-negative terms, so each of its (fewer than 24) roundings is a relative u downwards at worst:
// the factor 1 + 2^-18 = 1 + 64 u puts the result above the real number it stands for, the 2^-20 of 2. included.
PC_HD float pc_margin(const float *f, float C1, float C2, float thr, float splus) {
    float big = 0.f;
    bool finite = true;
    for (int k = 0; k < 9; k++) {
        big = fmaxf(big, fabsf(f[k]));   // fmaxf drops a NaN:
        finite = finite && f[k] == f[k];   // looked at on its own
    }
    if (!(pc_pair_ok(C1, C2, thr) && finite && big <= 1024.f)) return INFINITY;
    const float c21 = C2 * C1;
    const float T = (((fabsf(f[0]) + fabsf(f[1])) + (fabsf(f[3]) + fabsf(f[4]))) * c21 + (fabsf(f[2]) + fabsf(f[5])) * C2) +
                    ((fabsf(f[6]) + fabsf(f[7])) * C1 + fabsf(f[8]));
    const float T0 = (fabsf(f[0]) + fabsf(f[1])) * C1 + fabsf(f[2]);
    const float E = (float)(kPcNumer * kPcU) * T, E0 = (float)(kPcDenom * kPcU) * T0;
    return (E + splus * E0) * (1.f + 0x1p-18f) + (float)kPcFloor;
}

// the comparison: true only for a certified miss (ordered: false when anything is NaN)
PC_HD bool pc_miss(float n, float a0, float splus, float c) { return fabsf(n) > fmaf(splus, fabsf(a0), c); }
