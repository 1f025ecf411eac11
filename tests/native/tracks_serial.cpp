// vslam_triangulate_tracks (include/vslam_tracks.h) walked serially on the host over what the kernel compiles
// (vslam_amd/csrc/tracks_math.h), the points in descending order: no result depends on it.  tests/test_tracks_serial.py builds this
// with -fsanitize=address,undefined and holds the results bit for bit to tests/ref_tracks.py.
//   tracks_serial <in> <out>
// in:  int32 cases; per case int32 S, O, n, Cs, C, Kp, iterations, min_good, good10; f64 cos_parallax_max, huber_px, inlier_px; f32 K [9];
//      f32 points [S][4]; int32 offsets [S + 1], cam [O], kp [O]; f64 R [Cs][9], T [Cs][3]; f32 xy [Cs][Kp][2]
// out: per case int32 refused (1: the parameters or K are refused, nothing else follows); f32 out_points [S][4]; int32 status [S],
//      counts [S][2]; f64 info [S][3]; int32 stats [4]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vslam_amd/csrc/tracks_math.h"

using namespace vs_tracks;

template <typename T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}

template <typename T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

static void one_case(FILE *in, FILE *out) {
    const auto h = take<int32_t>(in, 9);
    const int S = h[0], O = h[1], Cs = h[3], Kp = h[5];
    const int n = std::min(std::max(h[2], 0), S), C = std::min(std::max(h[4], 0), Cs);
    const auto d = take<double>(in, 3);
    const auto Kf = take<float>(in, 9);
    const auto points = take<float>(in, (size_t)S * 4);
    const auto off = take<int32_t>(in, S + 1), cam = take<int32_t>(in, O), kp = take<int32_t>(in, O);
    const auto R = take<double>(in, (size_t)Cs * 9), T = take<double>(in, (size_t)Cs * 3);
    const auto xy = take<float>(in, (size_t)Cs * Kp * 2);
    double K[9], Ki[9];
    for (int k = 0; k < 9; k++) K[k] = (double)Kf[k];
    const bool ok = tr_params_ok(d[0], d[1], d[2], h[6], h[7], h[8]) && tr_kinv(K, Ki);
    const std::vector<int32_t> refused{ok ? 0 : 1};
    put(out, refused);
    if (!ok) return;
    const TrParams prm = tr_params(d[0], d[1], d[2], h[6], h[7], h[8]);
    TrItem it;
    it.cam = cam.data(); it.kp = kp.data(); it.R = R.data(); it.T = T.data(); it.xy = xy.data(); it.C = C; it.kp_stride = Kp;
    std::vector<float> out_points(points);
    std::vector<int32_t> status(S, kTrNoPart), counts((size_t)S * 2, 0), stats(4, 0);
    std::vector<double> info((size_t)S * 3, tr_qnan());
    for (int i = n - 1; i >= 0; i--) {
        TrResult res;
        tr_point(K, Ki, it, off[i], off[i + 1], O, points[4 * i], points[4 * i + 1], points[4 * i + 2], prm, res);
        status[i] = res.status;
        counts[2 * i] = res.m;
        counts[2 * i + 1] = res.n_good;
        info[3 * i] = res.cos_parallax;
        info[3 * i + 1] = res.cost_in;
        info[3 * i + 2] = res.cost_out;
        if (res.status == kTrOk) {
            for (int k = 0; k < 3; k++) out_points[4 * i + k] = (float)res.X[k];
            out_points[4 * i + 3] = 1.0f;
        }
        if (res.status >= 0) {
            stats[0]++;
            stats[res.status == kTrOk ? 1 : res.status == kTrLowParallax ? 2 : 3]++;
        }
    }
    put(out, out_points);
    put(out, status);
    put(out, counts);
    put(out, info);
    put(out, stats);
}

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    const int cases = take<int32_t>(in, 1)[0];
    for (int c = 0; c < cases; c++) one_case(in, out);
    fclose(in);
    fclose(out);
    return 0;
}
