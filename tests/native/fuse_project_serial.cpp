// vslam_fuse_project (include/vslam_fuse_project.h) walked serially on the host over what the kernels compile
// (vslam_amd/csrc/fuse_project_math.h, and through it search_math.h and fuse_math.h), in another order than the device's: cameras
// and points from the last to the first, the grid of every camera filled by a serial counting sort in descending keypoint order,
// keys and holders in ordered maps, every pair's proposal through the packed word, the found pairs sorted at the end.
// tests/test_fuse_project_serial.py builds this with -fsanitize=address,undefined and holds the results bit for bit to
// tests/ref_fuse_project.py, which has no grid.
//   fuse_project_serial <in> <out>
// in:  int32 cases; per case int32 S, O, Cs, Kp, n, n_cams, width, height, has_mask, found_stride, dist_threshold, ratio10; f64 radius;
//      f32 K [9]; f32 points [S][4]; int32 offsets [S + 1], cam [O], kp [O]; u8 obs_desc [O][32]; f64 R [Cs][9], T [Cs][3]; f32 xy
//      [Cs][Kp][2]; u8 desc [Cs][Kp][32]; int32 n_kp [Cs]; int32 mask [Cs] if has_mask
// out: per case int32 m; found_point, found_cam, found_kp, found_dist, found_holder [m]; stats [6]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "../../vslam_amd/csrc/fuse_project_math.h"

using namespace vs_search;
using namespace vs_fuse;
using namespace vs_fuse_project;

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

static int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int cases = take<int32_t>(in, 1)[0];
    for (int q = 0; q < cases; q++) {
        const auto h = take<int32_t>(in, 12);
        const int S = h[0], O = h[1], Cs = h[2], Kp = h[3], width = h[6], height = h[7], found_stride = h[9];
        const int n = clampi(h[4], S), C = clampi(h[5], Cs);
        const double radius = take<double>(in, 1)[0];
        const SsParams prm = ss_params(radius, h[10], h[11]);
        const auto Kf = take<float>(in, 9);
        const auto points = take<float>(in, (size_t)S * 4);
        const auto offsets = take<int32_t>(in, (size_t)S + 1);
        const auto ocam = take<int32_t>(in, O), okp = take<int32_t>(in, O);
        const auto obs = take<uint8_t>(in, (size_t)O * 32);
        const auto Rv = take<double>(in, (size_t)Cs * 9), Tv = take<double>(in, (size_t)Cs * 3);
        const auto xy = take<float>(in, (size_t)Cs * Kp * 2);
        const auto desc = take<uint8_t>(in, (size_t)Cs * Kp * 32);
        const auto n_kp = take<int32_t>(in, Cs);
        const auto mask = take<int32_t>(in, h[8] ? Cs : 0);
        double K[9];
        for (int k = 0; k < 9; k++) K[k] = (double)Kf[k];

        std::vector<int32_t> stats(6, 0);
        std::vector<std::tuple<int, int, int, int, int>> found;   // (c, i, k, d0, holder)
        bool sound = true;
        for (int i = n; i >= 0; i--) sound = sound && fu_offset_ok(i > 0 ? offsets[i - 1] : 0, offsets[i], O);
        if (sound) {
            std::map<std::pair<int, int>, int> holder;
            for (int i = n - 1; i >= 0; i--)   // descending: the last write of a cell is its smallest point
                for (int o = offsets[i]; o < offsets[i + 1]; o++)
                    if (fu_valid(ocam.at(o), okp.at(o), Cs, Kp)) holder[{ocam[o], okp[o]}] = i;
            const SsGrid g = ss_grid(width, height, radius);
            const int cells = g.nx * g.ny;
            const double reach = radius + kSsMargin;
            for (int c = Cs - 1; c >= 0; c--) {
                LmCam cam;
                for (int k = 0; k < 9; k++) cam.R[k] = Rv[(size_t)c * 9 + k];
                for (int k = 0; k < 3; k++) cam.T[k] = Tv[(size_t)c * 3 + k];
                if (!fp_cam_part(cam, c, C, h[8] ? mask.data() : nullptr)) continue;
                const int nk = clampi(n_kp[c], Kp);
                const float *XY = xy.data() + (size_t)c * Kp * 2;
                const uint8_t *D = desc.data() + (size_t)c * Kp * 32;
                std::vector<uint32_t> cell_end(cells, 0);
                std::vector<uint16_t> cell_kp(nk);
                auto cell_of = [&](int k) -> int {
                    const float x = XY[2 * (size_t)k], y = XY[2 * (size_t)k + 1];
                    if (!(std::isfinite(x) && std::isfinite(y))) return -1;
                    return ss_cell((double)y, g.inv_c, g.ny) * g.nx + ss_cell((double)x, g.inv_c, g.nx);
                };
                for (int k = 0; k < nk; k++)
                    if (cell_of(k) >= 0) cell_end.at(cell_of(k))++;
                uint32_t run = 0;
                for (int j = 0; j < cells; j++) {
                    const uint32_t cnt = cell_end[j];
                    cell_end[j] = run;
                    run += cnt;
                }
                for (int k = nk - 1; k >= 0; k--)
                    if (cell_of(k) >= 0) cell_kp.at(cell_end.at(cell_of(k))++) = (uint16_t)k;

                std::map<int, unsigned long long> keys;
                std::vector<int32_t> prop(n, 0);
                for (int i = n - 1; i >= 0; i--) {
                    const float px = points[4 * (size_t)i], py = points[4 * (size_t)i + 1], pz = points[4 * (size_t)i + 2];
                    const int o0 = offsets[i], o1 = offsets[i + 1];
                    const bool tried = fp_point_part(px, py, pz, o0, o1, O) && !fp_seen(ocam.data(), okp.data(), o0, o1, c, Kp);
                    double u, v;
                    const bool visible = tried && ss_visible(K, cam, true, px, py, pz, o0, o1, O, width, height, u, v);
                    SsBest best;
                    if (visible) {
                        const int cx0 = ss_cell(u - reach, g.inv_c, g.nx), cx1 = ss_cell(u + reach, g.inv_c, g.nx);
                        const int cy0 = ss_cell(v - reach, g.inv_c, g.ny), cy1 = ss_cell(v + reach, g.inv_c, g.ny);
                        for (int cy = cy1; cy >= cy0; cy--) {
                            const int lo = cy * g.nx + cx0, hi = cy * g.nx + cx1;
                            for (uint32_t j = lo > 0 ? cell_end.at(lo - 1) : 0; j < cell_end.at(hi); j++) {
                                const int k = cell_kp.at(j);
                                if (!ss_in_disc(XY[2 * (size_t)k], XY[2 * (size_t)k + 1], u, v, prm.r2)) continue;
                                uint32_t dk[8], dobs[8];
                                words(D + (size_t)k * 32, dk);
                                uint32_t d = kSsNone;
                                for (int o = o0; o < o1; o++) {
                                    words(&obs.at((size_t)o * 32), dobs);
                                    const uint32_t cur = ss_ham256(dk, dobs);
                                    d = cur < d ? cur : d;
                                }
                                ss_offer(best, d, (uint32_t)k);
                            }
                        }
                    }
                    const bool proposes = visible && ss_proposes(best, prm);
                    prop[i] = fp_pack(tried, visible, proposes, best.k0, best.d0);
                    stats[0] += tried ? 1 : 0;
                    stats[1] += visible ? 1 : 0;
                    stats[2] += proposes ? 1 : 0;
                    if (!proposes) continue;
                    const unsigned long long key = ss_key(best.d0, (uint32_t)i);
                    auto it = keys.find((int)best.k0);
                    if (it == keys.end() || key < it->second) keys[(int)best.k0] = key;
                }
                for (int i = 0; i < n; i++) {
                    const int32_t w = prop[i];
                    if (!(w & kFpProposes) || keys.at(fp_k0(w)) != ss_key((uint32_t)fp_d0(w), (uint32_t)i)) continue;
                    const auto hd = holder.find({c, fp_k0(w)});
                    found.emplace_back(c, i, fp_k0(w), fp_d0(w), hd == holder.end() ? -1 : hd->second);
                }
            }
        }
        std::sort(found.begin(), found.end());
        const int m = std::min((int)found.size(), found_stride);
        stats[3] = (int32_t)found.size();
        for (const auto &t : found) stats[4] += std::get<4>(t) >= 0 ? 1 : 0;
        stats[5] = m;
        std::vector<int32_t> col[5];
        for (int j = 0; j < m; j++) {
            col[0].push_back(std::get<1>(found[j]));
            col[1].push_back(std::get<0>(found[j]));
            col[2].push_back(std::get<2>(found[j]));
            col[3].push_back(std::get<3>(found[j]));
            col[4].push_back(std::get<4>(found[j]));
        }
        put(out, std::vector<int32_t>{m});
        for (const auto &v : col) put(out, v);
        put(out, stats);
    }
    fclose(in);
    fclose(out);
    return 0;
}
