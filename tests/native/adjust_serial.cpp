// The arithmetic of the window adjustment (vslam_amd/csrc/adjust_math.h, the text the kernel compiles) on the host, one point, one
// entry and one row after the other: the rounds of include/vslam_adjust.h with plain left-to-right sums over the points where
// the device has its lane-strided ones.  tests/test_adjust_serial.py holds its result to tests/ref_adjust.py, which checks the
// formulas without a GPU.
//
// usage: adjust_serial <in.bin>      (build with -ffp-contract=off; the test adds -fsanitize=address,undefined)
//   in.bin: int32 cam_stride, pt_stride, obs_stride, C, N, max_iterations, rounds, min_obs, n_fixed, 0; f64 huber, gate; K [9] f64;
//           R [cam_stride][9], T [cam_stride][3], X [pt_stride][3] f64; int32 offsets [pt_stride + 1], cam [obs_stride];
//           xy [obs_stride][2] f32
//   stdout: moved (0 / 1); stats [4]; R; T; X -- %.17g, one line each; then the bits of X, one hexadecimal word per entry (a NaN's
//           payload does not survive %.17g)
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "../../vslam_amd/csrc/adjust_math.h"

using namespace vs_adjust;

struct SerialEx {   // one caller owns everything: its partial sums are the sums
    template <class F>
    void points(int n, F f) const {
        for (int i = 0; i < n; i++) f(i);
    }
    template <class F>
    void entries(int n, F f) const {
        for (int i = 0; i < n; i++) f(i);
    }
    template <class F>
    void rows(int n, F f) const {
        for (int i = 0; i < n; i++) f(i);
    }
    template <class F>
    void one(F f) const {
        f();
    }
    void sync() const {}
    template <int N>
    void sum(double (&)[N]) {}
    bool any(bool f) { return f; }
};

template <class T>
static bool rd(FILE *f, std::vector<T> &v) {
    return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    int hdr[10];
    double hg[2], K[9];
    if (!f || fread(hdr, 4, 10, f) != 10 || fread(hg, 8, 2, f) != 2 || fread(K, 8, 9, f) != 9) return 3;
    const int cs = hdr[0], ps = hdr[1], os = hdr[2];
    if (cs < 1 || ps < 1 || os < 1) return 3;
    std::vector<double> R(9 * (size_t)cs), T(3 * (size_t)cs), X(3 * (size_t)ps);
    std::vector<int32_t> off((size_t)ps + 1), cam((size_t)os);
    std::vector<float> xy(2 * (size_t)os);
    if (!rd(f, R) || !rd(f, T) || !rd(f, X) || !rd(f, off) || !rd(f, cam) || !rd(f, xy)) return 3;
    fclose(f);
    AdParams p;
    p.max_iterations = hdr[5]; p.rounds = hdr[6]; p.min_obs = hdr[7]; p.n_fixed = hdr[8];
    p.huber = hg[0]; p.gate = hg[1];
    AdItem it;
    it.C = hdr[3]; it.N = hdr[4]; it.cam_stride = cs; it.pt_stride = ps; it.obs_stride = os;
    it.R = R.data(); it.T = T.data(); it.X = X.data(); it.off = off.data(); it.cam = cam.data(); it.xy = xy.data();
    std::vector<double> Xa(3 * (size_t)ps), Xb(3 * (size_t)ps), z(3 * (size_t)ps), stage((size_t)ps * kAdMaxSlots * kAdStage);
    std::vector<int32_t> mask((size_t)ps);
    std::vector<uint8_t> fa((size_t)os), fb((size_t)os);
    AdWork w{Xa.data(), Xb.data(), z.data(), stage.data(), mask.data(), fa.data(), fb.data()};
    static AdShared sh;
    SerialEx ex;
    AdResult res{nullptr, nullptr, 0};
    double stats[4];
    const bool moved = ad_run(K, it, p, w, sh, ex, res, stats);
    if (moved) {
        for (int c = 0; c < it.C; c++) {
            if (!((res.ever_free >> c) & 1)) continue;
            for (int k = 0; k < 9; k++) R[9 * (size_t)c + k] = sh.cur[c].R[k];
            for (int k = 0; k < 3; k++) T[3 * (size_t)c + k] = sh.cur[c].T[k];
        }
        for (int i = 0; i < it.N; i++) {
            if (!ad_took_part(it.off, res.flags, i)) continue;
            for (int k = 0; k < 3; k++) X[3 * (size_t)i + k] = res.X[3 * (size_t)i + k];
        }
    }
    printf("%d\n", moved ? 1 : 0);
    for (int k = 0; k < 4; k++) printf("%.17g ", stats[k]);
    printf("\n");
    for (double v : R) printf("%.17g ", v);
    printf("\n");
    for (double v : T) printf("%.17g ", v);
    printf("\n");
    for (double v : X) printf("%.17g ", v);
    printf("\n");
    for (double v : X) {
        unsigned long long u;
        memcpy(&u, &v, sizeof u);
        printf("%llx ", u);
    }
    printf("\n");
    return 0;
}
