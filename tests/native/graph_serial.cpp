// vslam_amd/csrc/graph_math.h walked serially on the host: one caller that owns every unit, so the sums run 0, 1, 2, ... and
// nothing needs closing.  Built by tests/graph_cases.py with -fsanitize=address,undefined -ffp-contract=off; reads a list of cases
// and writes what vslam_graph_optimize would leave: scale, R, T (whole, padding included), the four statistics and the number of
// CG iterations taken.
//   in:  int32 cases; per case: int32 node_stride, edge_stride, n_nodes, n_edges, max_iterations, cg_iterations; f64 cg_tolerance;
//        scale [S], R [S][9], T [S][3] f64; fixed [S] i32; ab [Es][2] i32; zs [Es], zR [Es][9], zt [Es][3], zw [Es][3] f64
//   out: per case: scale, R, T; stats [4] f64; cg iterations i32
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vslam_amd/csrc/graph_math.h"

using namespace vs_graph;

struct Serial {
    template <class F>
    void each(int n, F f) const {
        for (int i = 0; i < n; i++) f(i);
    }
    template <int N>
    void sum(double (&)[N]) const {}
    bool any(bool f) const { return f; }
    void sync() const {}
    void adjacency(const GrItem &it, int N, int E) const {
        for (int i = 0; i <= N; i++) it.start[i] = 0;
        for (int k = 0; k < E; k++) {
            if (!it.use[k]) continue;
            it.start[it.ab[2 * k] + 1]++;
            it.start[it.ab[2 * k + 1] + 1]++;
        }
        for (int i = 0; i < N; i++) {
            it.start[i + 1] += it.start[i];
            it.fill[i] = 0;
        }
        for (int k = 0; k < E; k++) {
            if (!it.use[k]) continue;
            for (int side = 0; side < 2; side++) {
                const int n = it.ab[2 * k + side];
                it.adj[it.start[n] + it.fill[n]++] = (k << 1) | side;
            }
        }
    }
};

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return v;
}

template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
}

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    const int cases = take<int32_t>(in, 1)[0];
    for (int c = 0; c < cases; c++) {
        const auto h = take<int32_t>(in, 6);
        const size_t S = (size_t)h[0], Es = (size_t)h[1];
        GrParams prm{h[4], h[5], take<double>(in, 1)[0]};
        auto scale = take<double>(in, S), R = take<double>(in, 9 * S), T = take<double>(in, 3 * S);
        const auto fixed = take<int32_t>(in, S), ab = take<int32_t>(in, 2 * Es);
        const auto zs = take<double>(in, Es), zR = take<double>(in, 9 * Es), zt = take<double>(in, 3 * Es), zw = take<double>(in, 3 * Es);
        std::vector<double> ws(gr_workspace_bytes((int)S, (int)Es) / sizeof(double));   // exactly the bytes the header states
        GrItem it;
        it.n_nodes = h[2]; it.n_edges = h[3]; it.node_stride = (int)S; it.edge_stride = (int)Es;
        it.scale = scale.data(); it.R = R.data(); it.T = T.data();
        it.fixed = fixed.data(); it.ab = ab.data();
        it.z_scale = zs.data(); it.z_R = zR.data(); it.z_T = zt.data(); it.z_w = zw.data();
        gr_workspace(ws.data(), it);
        Serial par;
        std::vector<double> stats(4);
        double st[4];
        int cg = 0;
        gr_run(par, it, prm, st, cg);
        for (int k = 0; k < 4; k++) stats[k] = st[k];
        put(out, scale);
        put(out, R);
        put(out, T);
        put(out, stats);
        put(out, std::vector<int32_t>{cg});
    }
    fclose(in);
    fclose(out);
    return 0;
}
