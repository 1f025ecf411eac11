// vslam_pnp_ransac (include/vslam_pnp.h) on the host, one hypothesis and one correspondence after the other: the text the kernels
// compile (vslam_amd/csrc/pnp_math.h; the polish is resect_math.h's rounds with plain left-to-right sums, as
// tests/native/resect_serial.cpp walks them).  tests/test_pnp_serial.py holds it to tests/ref_pnp.py without a GPU, and
// tests/test_gpu_pnp.py holds the device's integers to it exactly.
//
// usage: pnp_serial <in.bin> <out.bin>      (build with -ffp-contract=off; the test adds -fsanitize=address,undefined)
//   in.bin : int32 cases; per case int32 S, n, hypotheses, min_inliers, polish (0 / 1), max_iterations, rounds, min_links;
//            uint32 seed; f64 inlier_px, huber, gate; K [9] f32; R [9], T [3] f64 (the bits an item left alone keeps);
//            points [S][3] f64; xy [S][2] f32
//   out.bin: per case counts [hypotheses][4] int32; winner, n_inliers int32; inlier [S] int32; corr_index [n_inliers] int32;
//            R [9], T [3] f64 before the polish; R [9], T [3] f64 after it; stats [4] f64
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vslam_amd/csrc/pnp_math.h"
#include "../../vslam_amd/csrc/resect_math.h"

using namespace vs_pnp;
using namespace vs_resect;

struct SerialSrc {
    const std::vector<double> &P;
    const std::vector<float> &x;
    int n;
    template <class F>
    void each(F f) const {
        for (int i = 0; i < n; i++) {
            const double p[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
            const double o[2] = {(double)x[2 * (size_t)i], (double)x[2 * (size_t)i + 1]};
            f(p, o);
        }
    }
};

struct SerialRed {
    template <int N>
    void sum(double (&)[N]) {}
    bool any(bool f) { return f; }
};

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE *f, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) exit(4); }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    int cases;
    if (!f || !g || !rd(f, &cases, 1)) return 3;
    for (int ci = 0; ci < cases; ci++) {
        int hdr[8];
        uint32_t seed;
        double dp[3];
        float Kf[9];
        LmCam keep;
        if (!rd(f, hdr, 8) || !rd(f, &seed, 1) || !rd(f, dp, 3) || !rd(f, Kf, 9) || !rd(f, keep.R, 9) || !rd(f, keep.T, 3)) return 3;
        const int S = hdr[0], H = hdr[2], min_inliers = hdr[3];
        if (S < 0 || H < 1 || H > 1024) return 3;
        const int n = hdr[1] < 0 ? 0 : hdr[1] > S ? S : hdr[1];
        std::vector<double> pts(3 * (size_t)S);
        std::vector<float> xy(2 * (size_t)S);
        if (!rd(f, pts.data(), pts.size()) || !rd(f, xy.data(), xy.size())) return 3;
        double K[9], Kinv[9];
        bool good = n >= 4;
        for (int k = 0; k < 9; k++) {
            K[k] = (double)Kf[k];
            good = good && std::isfinite(K[k]);
        }
        pn_kinv(K, Kinv);
        auto at = [&](int i, double(&P)[3], double(&x)[2]) {
            for (int k = 0; k < 3; k++) P[k] = pts[3 * (size_t)i + k];
            x[0] = (double)xy[2 * (size_t)i];
            x[1] = (double)xy[2 * (size_t)i + 1];
        };
        for (int i = 0; i < n; i++) {
            double P[3], x[2];
            at(i, P, x);
            good = good && pn_finite_row(P, x);
        }
        const double thr2 = dp[0] * dp[0];
        std::vector<int32_t> counts(4 * (size_t)H, -1);
        uint32_t best = 0;
        LmCam win = keep;
        for (int h = 0; h < H && good; h++) {
            LmCam cam[4];
            bool ok[4];
            pn_hypothesis(Kinv, seed, h, n, at, cam, ok);
            for (int s = 0; s < 4; s++) {
                if (!ok[s]) continue;
                int cnt = 0;
                for (int i = 0; i < n; i++) {
                    double P[3], x[2];
                    at(i, P, x);
                    cnt += pn_inlier(K, cam[s], P, x, thr2) ? 1 : 0;
                }
                counts[4 * (size_t)h + s] = cnt;
                const uint32_t key = pn_key(cnt, 4 * h + s);
                if (key > best) {
                    best = key;
                    win = cam[s];
                }
            }
        }
        const bool found = best != 0 && pn_key_count(best) >= min_inliers;
        const int32_t winner = found ? pn_key_pose(best) : -1;
        std::vector<int32_t> inl((size_t)S, 0), idx;
        std::vector<double> cp;
        std::vector<float> cx;
        if (found) {
            for (int i = 0; i < n; i++) {
                double P[3], x[2];
                at(i, P, x);
                if (!pn_inlier(K, win, P, x, thr2)) continue;
                inl[i] = 1;
                idx.push_back(i);
                cp.insert(cp.end(), P, P + 3);
                cx.push_back(xy[2 * (size_t)i]);
                cx.push_back(xy[2 * (size_t)i + 1]);
            }
        }
        const LmCam raw = found ? win : keep;
        LmCam out = raw;
        const double qnan = __builtin_nan("");
        double stats[4] = {qnan, qnan, qnan, qnan};
        if (hdr[4]) {
            RsParams p;
            p.max_iterations = hdr[5]; p.rounds = hdr[6]; p.min_links = hdr[7];
            p.huber = dp[1]; p.gate = dp[2];
            SerialSrc src{cp, cx, (int)idx.size()};
            SerialRed red;
            LmCam moved;
            if (rs_run(K, raw, p, src, red, moved, stats)) out = moved;
        }
        const int32_t tail[2] = {winner, (int32_t)idx.size()};
        wr(g, counts.data(), counts.size());
        wr(g, tail, 2);
        wr(g, inl.data(), inl.size());
        wr(g, idx.data(), idx.size());
        wr(g, raw.R, 9);
        wr(g, raw.T, 3);
        wr(g, out.R, 9);
        wr(g, out.T, 3);
        wr(g, stats, 4);
    }
    fclose(f);
    fclose(g);
    return 0;
}
