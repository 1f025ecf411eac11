// The scale selection of the world frame on the host: vslam_amd/csrc/world_select.h -- the header the kernel of world.hip
// compiles -- run serially: keys from (carry, X) pairs, the rank of the lower median, eight radix passes over 256-bin
// histograms.  Checks itself against std::sort and writes what it selected, so that tests/test_world_select_host.py can hold it
// to tests/ref_world.py.  Built with -fsanitize=address,undefined by that test.
//
// usage: world_select_check <in.bin> <out.bin>
//   in.bin:  int32 cases; per case: int32 n, then n x (carry[3], X[3]) f64
//   out.bin: per case: int32 links, f64 selected q (NaN when there is no link), f64 sqrt of it
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../vslam_amd/csrc/world_select.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    int cases = 0;
    if (!fi || !fo || fread(&cases, 4, 1, fi) != 1) return 3;
    for (int c = 0; c < cases; c++) {
        int n = 0;
        if (fread(&n, 4, 1, fi) != 1 || n < 0) return 3;
        std::vector<double> in(6 * (size_t)n);
        if (n && fread(in.data(), 48, (size_t)n, fi) != (size_t)n) return 3;
        std::vector<uint64_t> keys((size_t)n);
        uint32_t L = 0;
        for (int i = 0; i < n; i++) {
            keys[i] = ws_link_key(&in[6 * (size_t)i], &in[6 * (size_t)i + 3]);
            L += keys[i] != kWsNoKey ? 1u : 0u;
        }
        double q = std::nan(""), s = std::nan("");
        if (L) {
            uint32_t rank = ws_rank(L);
            uint64_t prefix = 0;
            for (int pass = 0; pass < kWsPasses; pass++) {
                uint32_t hist[kWsBins] = {0};
                for (int i = 0; i < n; i++)
                    if (ws_in_prefix(keys[i], prefix, pass)) hist[ws_digit(keys[i], pass)]++;
                ws_pick(hist, pass, &rank, &prefix);
            }
            std::vector<uint64_t> sorted;
            for (uint64_t k : keys)
                if (k != kWsNoKey) sorted.push_back(k);
            std::sort(sorted.begin(), sorted.end());
            if (sorted[(L - 1) / 2] != prefix) {
                fprintf(stderr, "case %d: radix select %016llx, sort %016llx\n", c, (unsigned long long)prefix,
                        (unsigned long long)sorted[(L - 1) / 2]);
                return 4;
            }
            q = ws_value(prefix);
            s = std::sqrt(q);
        }
        const int links = (int)L;
        fwrite(&links, 4, 1, fo);
        fwrite(&q, 8, 1, fo);
        fwrite(&s, 8, 1, fo);
    }
    fclose(fi);
    fclose(fo);
    return 0;
}
