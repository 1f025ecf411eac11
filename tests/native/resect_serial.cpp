// The arithmetic of the resection (vslam_amd/csrc/resect_math.h, the text the kernels compile) on the host, one correspondence
// after the other: the rounds of include/vslam_resect.h with plain left-to-right sums where the device has its lane-strided ones.
// tests/test_resect_serial.py holds its result to tests/ref_resect.py, which checks the formulas without a GPU.
//
// usage: resect_serial <in.bin>      (build with -ffp-contract=off; the test adds -fsanitize=address,undefined)
//   in.bin: int32 n, max_iterations, rounds, min_links; f64 huber, gate; K [9], R [9], T [3] f64; P [n][3] f64; x [n][2] f64
//   stdout: moved (0 / 1); stats [4]; R [9]; T [3] -- %.17g
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vslam_amd/csrc/resect_math.h"

using namespace vs_resect;

struct SerialSrc {
    const std::vector<double> &P, &x;
    int n;
    template <class F>
    void each(F f) const {
        for (int i = 0; i < n; i++) {
            const double p[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
            const double o[2] = {x[2 * (size_t)i], x[2 * (size_t)i + 1]};
            f(p, o);
        }
    }
};

struct SerialRed {   // one caller owns every correspondence: its partial sums are the sums
    template <int N>
    void sum(double (&)[N]) {}
    bool any(bool f) { return f; }
};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    int hdr[4];
    double hg[2], K[9];
    RsCam in, out;
    if (!f || fread(hdr, 4, 4, f) != 4 || hdr[0] < 0 || fread(hg, 8, 2, f) != 2 || fread(K, 8, 9, f) != 9 || fread(in.R, 8, 9, f) != 9 ||
        fread(in.T, 8, 3, f) != 3)
        return 3;
    const int n = hdr[0];
    std::vector<double> P(3 * (size_t)n), x(2 * (size_t)n);
    if (fread(P.data(), 8, P.size(), f) != P.size() || fread(x.data(), 8, x.size(), f) != x.size()) return 3;
    fclose(f);
    RsParams p;
    p.max_iterations = hdr[1]; p.rounds = hdr[2]; p.min_links = hdr[3];
    p.huber = hg[0]; p.gate = hg[1];
    SerialSrc src{P, x, n};
    SerialRed red;
    double stats[4];
    const bool moved = rs_run(K, in, p, src, red, out, stats);
    if (!moved) out = in;
    printf("%d\n", moved ? 1 : 0);
    for (int k = 0; k < 4; k++) printf("%.17g ", stats[k]);
    printf("\n");
    for (int k = 0; k < 9; k++) printf("%.17g ", out.R[k]);
    printf("\n");
    for (int k = 0; k < 3; k++) printf("%.17g ", out.T[k]);
    printf("\n");
    return 0;
}
