// The arithmetic of vslam_refine_pairs (vslam_amd/csrc/refine_math.h, the text the kernel compiles) on the host, one point after
// the other: the iteration of include/vslam_amd.h with plain left-to-right sums where the device has its lane-strided ones.
// tests/test_refine_serial.py holds its result to tests/ref_refine.py, which checks the formulas without a GPU.
//
// usage: refine_serial <in.bin> <max_iterations>      (build with -ffp-contract=off)
//   in.bin: int32 n; K [9], R [9], t [3] f64 (the start: R, t as the device forms them); obs [n][4] f64; X [n][3] f64
//   stdout: accepted steps, objective; R [9]; t [3]; X [n][3] -- %.17g
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vslam_amd/csrc/refine_math.h"

using namespace vs_refine;

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n <= 0) return 3;
    const int max_iterations = atoi(argv[2]);
    std::vector<double> obs(4 * (size_t)n), X(3 * (size_t)n), Xn(3 * (size_t)n);
    double K[9];
    BaCam cur, cand;
    if (fread(K, 8, 9, f) != 9 || fread(cur.R, 8, 9, f) != 9 || fread(cur.t, 8, 3, f) != 3 || fread(obs.data(), 8, 4 * (size_t)n, f) != 4 * (size_t)n ||
        fread(X.data(), 8, 3 * (size_t)n, f) != 3 * (size_t)n)
        return 3;
    fclose(f);
    auto point = [&](const std::vector<double> &P, int i, double (&x)[3], double (&o)[4]) {
        for (int k = 0; k < 3; k++) x[k] = P[3 * (size_t)i + k];
        for (int k = 0; k < 4; k++) o[k] = obs[4 * (size_t)i + k];
    };
    double obj = 0.0, lambda = kLambda0;
    for (int i = 0; i < n; i++) {
        double x[3], o[4], e1, e2, dz;
        point(X, i, x, o);
        ba_errors(K, cur, x, o, e1, e2, dz);
        obj += e1 + e2;
    }
    int accepted = 0;
    for (int it = 0; it < max_iterations; it++) {
        double b1[3], b2[3], acc[20] = {0}, dc[5];
        ba_tangent(cur.t, b1, b2);
        bool bad = false;
        for (int i = 0; i < n; i++) {
            double x[3], o[4], Yv[3][5], z[3], a[20];
            point(X, i, x, o);
            if (!ba_point_blocks(K, cur, b1, b2, lambda, x, o, Yv, z, a)) bad = true;
            for (int k = 0; k < 20; k++) acc[k] += a[k];
        }
        bool accept = false;
        double obj_new = 0.0;
        if (!bad && ba_reduced_solve(acc, dc)) {
            ba_candidate(cur, b1, b2, dc, cand);
            bool behind = false;
            for (int i = 0; i < n; i++) {
                double x[3], o[4], Yv[3][5], z[3], a[20], xn[3], e1, e2, dz;
                point(X, i, x, o);
                ba_point_blocks(K, cur, b1, b2, lambda, x, o, Yv, z, a);
                ba_point_step(x, Yv, z, dc, xn);
                for (int k = 0; k < 3; k++) Xn[3 * (size_t)i + k] = xn[k];
                ba_errors(K, cand, xn, o, e1, e2, dz);
                obj_new += e1 + e2;
                if (!(xn[2] > 0.0) || !(dz > 0.0)) behind = true;
            }
            accept = !behind && obj_new < obj;
        }
        if (accept) {
            const double rel = (obj - obj_new) / obj;
            cur = cand;
            obj = obj_new;
            X.swap(Xn);
            accepted++;
            lambda = fmax(lambda / 10.0, kLambdaMin);
            if (rel < kRelStop) break;
        } else {
            lambda = lambda * 10.0;
            if (lambda > kLambdaMax) break;
        }
    }
    printf("%d %.17g\n", accepted, obj);
    for (int k = 0; k < 9; k++) printf("%.17g ", cur.R[k]);
    printf("\n");
    for (int k = 0; k < 3; k++) printf("%.17g ", cur.t[k]);
    printf("\n");
    for (size_t k = 0; k < 3 * (size_t)n; k++) printf("%.17g ", X[k]);
    printf("\n");
    return 0;
}
