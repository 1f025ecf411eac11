// The search by projection walked serially on the host with what the kernels compile (vslam_amd/csrc/search_math.h): the grid
// (ss_grid / ss_cell) filled by a serial counting sort, every point's window walked cell by cell, the running (d, k) choice, the
// ratio rule, the 64-bit keys and their minimum, the ordered compaction.  Built with -fsanitize=address,undefined by
// tests/test_search_serial.py and held bit for bit to tests/ref_search.py, which has no grid.
//
// usage: search_serial <cases.bin> <out.bin>
//   in : int32 cases; per case int32 S, O, Kp, n_points, n_kp, width, height, has_taken, dist_threshold, ratio10; f64 radius;
//        f64 R[9], T[3]; f32 K[9]; f32 points[S][4]; int32 offsets[S + 1]; u8 obs[O][32]; f32 xy[Kp][2]; u8 desc[Kp][32];
//        int32 taken[Kp] when has_taken
//   out: per case int32 kp_of_point[S], dist[S], stats[4], n_corr, corr_point[n_corr], corr_kp[n_corr]; f64 corr_points[n_corr][3];
//        f32 corr_xy[n_corr][2]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vslam_amd/csrc/search_math.h"

using namespace vs_search;

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

static void words(const uint8_t *row, uint32_t (&w)[8]) { memcpy(w, row, 32); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int cases = take<int32_t>(in, 1)[0];
    for (int c = 0; c < cases; c++) {
        const auto h = take<int32_t>(in, 10);
        const int S = h[0], O = h[1], Kp = h[2], width = h[5], height = h[6];
        const int n = h[3] < 0 ? 0 : h[3] > S ? S : h[3], n_kp = h[4] < 0 ? 0 : h[4] > Kp ? Kp : h[4];
        const double radius = take<double>(in, 1)[0];
        const SsParams prm = ss_params(radius, h[8], h[9]);
        const auto Rv = take<double>(in, 9), Tv = take<double>(in, 3);
        const auto Kf = take<float>(in, 9);
        const auto points = take<float>(in, (size_t)S * 4);
        const auto offsets = take<int32_t>(in, (size_t)S + 1);
        const auto obs = take<uint8_t>(in, (size_t)O * 32);
        const auto xy = take<float>(in, (size_t)Kp * 2);
        const auto desc = take<uint8_t>(in, (size_t)Kp * 32);
        const auto taken = take<int32_t>(in, h[7] ? (size_t)Kp : 0);
        double K[9];
        LmCam cam;
        for (int k = 0; k < 9; k++) {
            K[k] = (double)Kf[k];
            cam.R[k] = Rv[k];
        }
        for (int k = 0; k < 3; k++) cam.T[k] = Tv[k];
        const bool cam_ok = vs_lm::lm_finite(cam);

        // the grid: count, scan, fill
        const SsGrid g = ss_grid(width, height, radius);
        const int cells = g.nx * g.ny;
        std::vector<uint32_t> cell_end(cells, 0);
        std::vector<uint16_t> cell_kp(n_kp);
        auto cell_of = [&](int k) -> int {
            if (h[7] && taken[k] >= 0) return -1;
            const float x = xy[2 * (size_t)k], y = xy[2 * (size_t)k + 1];
            if (!(std::isfinite(x) && std::isfinite(y))) return -1;
            return ss_cell((double)y, g.inv_c, g.ny) * g.nx + ss_cell((double)x, g.inv_c, g.nx);
        };
        for (int k = 0; k < n_kp; k++)
            if (cell_of(k) >= 0) cell_end[cell_of(k)]++;
        uint32_t run = 0;
        for (int i = 0; i < cells; i++) {
            const uint32_t cnt = cell_end[i];
            cell_end[i] = run;
            run += cnt;
        }
        for (int k = n_kp - 1; k >= 0; k--)   // any order inside a cell will do: descending here
            if (cell_of(k) >= 0) cell_kp.at(cell_end[cell_of(k)]++) = (uint16_t)k;

        std::vector<unsigned long long> keys(Kp, kSsNoKey);
        std::vector<int32_t> prop_k(S, -1), prop_d(S, 0), stats(4, 0);
        const double reach = radius + kSsMargin;
        for (int i = 0; i < n; i++) {
            const int o0 = offsets[i], o1 = offsets[i + 1];
            double u, v;
            if (!ss_visible(K, cam, cam_ok, points[4 * (size_t)i], points[4 * (size_t)i + 1], points[4 * (size_t)i + 2], o0, o1, O, width,
                            height, u, v))
                continue;
            stats[0]++;
            SsBest best;
            bool any = false;
            const int cx0 = ss_cell(u - reach, g.inv_c, g.nx), cx1 = ss_cell(u + reach, g.inv_c, g.nx);
            const int cy0 = ss_cell(v - reach, g.inv_c, g.ny), cy1 = ss_cell(v + reach, g.inv_c, g.ny);
            for (int cy = cy0; cy <= cy1; cy++) {
                const int lo = cy * g.nx + cx0, hi = cy * g.nx + cx1;
                for (uint32_t j = lo > 0 ? cell_end.at(lo - 1) : 0; j < cell_end.at(hi); j++) {
                    const int k = cell_kp.at(j);
                    if (!ss_in_disc(xy[2 * (size_t)k], xy[2 * (size_t)k + 1], u, v, prm.r2)) continue;
                    any = true;
                    uint32_t dk[8], dobs[8];
                    words(&desc[(size_t)k * 32], dk);
                    uint32_t d = kSsNone;
                    for (int o = o0; o < o1; o++) {
                        words(&obs[(size_t)o * 32], dobs);
                        const uint32_t cur = ss_ham256(dk, dobs);
                        d = cur < d ? cur : d;
                    }
                    ss_offer(best, d, (uint32_t)k);
                }
            }
            stats[1] += any ? 1 : 0;
            if (!ss_proposes(best, prm)) continue;
            stats[2]++;
            prop_k[i] = (int32_t)best.k0;
            prop_d[i] = (int32_t)best.d0;
            const unsigned long long key = ss_key(best.d0, (uint32_t)i);
            if (key < keys.at(best.k0)) keys[best.k0] = key;
        }
        std::vector<int32_t> kp_of_point(S, -1), dist(S, -1), corr_point, corr_kp;
        std::vector<double> corr_points;
        std::vector<float> corr_xy;
        for (int i = 0; i < n; i++) {
            if (prop_k[i] < 0 || keys[prop_k[i]] != ss_key((uint32_t)prop_d[i], (uint32_t)i)) continue;
            kp_of_point[i] = prop_k[i];
            dist[i] = prop_d[i];
            corr_point.push_back(i);
            corr_kp.push_back(prop_k[i]);
            for (int r = 0; r < 3; r++) corr_points.push_back((double)points[4 * (size_t)i + r]);
            corr_xy.push_back(xy[2 * (size_t)prop_k[i]]);
            corr_xy.push_back(xy[2 * (size_t)prop_k[i] + 1]);
        }
        stats[3] = (int32_t)corr_point.size();
        put(out, kp_of_point);
        put(out, dist);
        put(out, stats);
        put(out, std::vector<int32_t>{(int32_t)corr_point.size()});
        put(out, corr_point);
        put(out, corr_kp);
        put(out, corr_points);
        put(out, corr_xy);
    }
    fclose(in);
    fclose(out);
    return 0;
}
