// The refinement of vslam_refine_pairs (vslam_amd/csrc/refine_math.h, the text the kernel compiles) on the host, one correspondence
// after the other: ba_run with plain left-to-right sums where the device has its lane-strided ones.
// tests/test_refine_serial.py holds its result to tests/ref_refine.py, which checks the formulas and the rules without a GPU.
//
// usage: refine_serial <in.bin>      (build with -ffp-contract=off; the test adds -fsanitize=address,undefined)
//   in.bin: int32 n, winner, max_iterations, 0; f64 gate_sq; K [9], R [9], t [3] f64 (the f32 inputs widened); obs [n][4] f64;
//           X [n][3] f64 (points4d widened)
//   stdout: moved (0 / 1); stats [4]; accepted steps, objective; R [9]; t [3]; X of the participants [.][3] -- %.17g, the last
//           four lines before the rounding to f32 (the inputs' R, t and no X when the pair is left alone)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vslam_amd/csrc/refine_math.h"

using namespace vs_refine;

struct SerialEx {   // one caller owns every correspondence: its partial sums are the sums
    int n;
    const std::vector<double> &obs, &X;
    std::vector<double> st;    // [2][3][n]
    std::vector<uint8_t> fl;   // [n]
    template <class F>
    void each(int count, F f) const {
        for (int i = 0; i < count; i++) f(i);
    }
    bool observed(int i, double (&o)[4]) const {
        for (int k = 0; k < 4; k++) o[k] = obs[4 * (size_t)i + k];
        return true;
    }
    void input(int i, double (&x)[3]) const {
        for (int k = 0; k < 3; k++) x[k] = X[3 * (size_t)i + k];
    }
    double &state(int buf, int k, int i) { return st[((size_t)buf * 3 + k) * n + i]; }
    uint8_t &flag(int i) { return fl[i]; }
    template <int N>
    void sum(double (&)[N]) {}
    bool any(bool f) { return f; }
};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    int hdr[4];
    double gate_sq, K[9];
    LmCam in;
    if (!f || fread(hdr, 4, 4, f) != 4 || hdr[0] < 0 || fread(&gate_sq, 8, 1, f) != 1 || fread(K, 8, 9, f) != 9 ||
        fread(in.R, 8, 9, f) != 9 || fread(in.T, 8, 3, f) != 3)
        return 3;
    const int n = hdr[0];
    std::vector<double> obs(4 * (size_t)n), X(3 * (size_t)n);
    if (fread(obs.data(), 8, obs.size(), f) != obs.size() || fread(X.data(), 8, X.size(), f) != X.size()) return 3;
    fclose(f);
    SerialEx ex{n, obs, X, std::vector<double>(6 * (size_t)n), std::vector<uint8_t>((size_t)n)};
    BaResult res;
    double stats[4];
    const bool moved = ba_run(K, in, hdr[1], n, gate_sq, hdr[2], ex, res, stats);
    if (!moved) {
        res.cam = in;
        res.objective = __builtin_nan("");
    }
    printf("%d\n", moved ? 1 : 0);
    for (int k = 0; k < 4; k++) printf("%.17g ", stats[k]);
    printf("\n%d %.17g\n", moved ? (int)stats[3] : 0, res.objective);
    for (int k = 0; k < 9; k++) printf("%.17g ", res.cam.R[k]);
    printf("\n");
    for (int k = 0; k < 3; k++) printf("%.17g ", res.cam.T[k]);
    printf("\n");
    for (int i = 0; moved && i < n; i++) {
        if (!ex.fl[i]) continue;
        for (int k = 0; k < 3; k++) printf("%.17g ", ex.state(res.buf, k, i));
    }
    printf("\n");
    return 0;
}
