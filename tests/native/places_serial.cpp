// vslam_amd/csrc/places_math.h walked serially on the host (tests/test_places_serial.py builds this with -fsanitize=address,undefined):
// the same text the device compiles decides every distance, assignment, vote, term and comparison; only the loops are this file's.
// Assignment is taken BOTH ways -- by pl_closer on distances and by the largest pl_key decoded with pl_key_decode, the form the
// matrix-core kernel keeps -- and the program fails if they ever differ.
// Input / output: tests/places_cases.py, run_serial.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vslam_amd/csrc/places_math.h"

using namespace vs_places;

static FILE *fin, *fout;
template <typename T>
static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, fin) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return v;
}
static int rd1() { return rd<int32_t>(1)[0]; }
template <typename T>
static void wr(const std::vector<T> &v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), fout);
}

static void row32(const uint8_t *p, uint32_t *o) { memcpy(o, p, 32); }

static void assign_row(const uint8_t *d, const std::vector<uint8_t> &vocab, int W, int &word, int &dist) {
    uint32_t a[8], b[8];
    row32(d, a);
    int bw = -1, bd = 1 << 30;
    float bkey = -3.0e38f;
    for (int w = W - 1; w >= 0; w--) {   // descending: the tie rule has to come from pl_closer, not from the order of the walk
        row32(&vocab[(size_t)w * 32], b);
        const int dd = pl_dist(a, b);
        if (pl_closer(dd, w, bd, bw)) {
            bd = dd;
            bw = w;
        }
        const float key = pl_key(dd, w);
        if (key > bkey) bkey = key;
    }
    int kd, kw;
    pl_key_decode((int)bkey, kd, kw);
    if (kd != bd || kw != bw) {
        fprintf(stderr, "key form disagrees: (%d, %d) against (%d, %d)\n", kd, kw, bd, bw);
        exit(3);
    }
    word = bw;
    dist = bd;
}

static void assign(const std::vector<uint8_t> &desc, const std::vector<int32_t> &n, int Fr, int Kp, const std::vector<uint8_t> &vocab, int W,
                   std::vector<int32_t> &word, std::vector<int32_t> &dist) {
    word.assign((size_t)Fr * Kp, -1);
    dist.assign((size_t)Fr * Kp, -1);
    for (int f = 0; f < Fr; f++) {
        const int c = n[f] < 0 ? 0 : (n[f] > Kp ? Kp : n[f]);
        for (int i = 0; i < c; i++) {
            int w, d;
            assign_row(&desc[((size_t)f * Kp + i) * 32], vocab, W, w, d);
            word[(size_t)f * Kp + i] = w;
            dist[(size_t)f * Kp + i] = d;
        }
    }
}

struct Index {
    int W;
    std::vector<uint8_t> vocab;
    std::vector<int32_t> weights, df, offsets{0}, words, tf;
    int size() const { return (int)offsets.size() - 1; }
    void set_weights(const std::vector<int32_t> *w) {
        weights.assign(W, 1);
        if (w)
            for (int i = 0; i < W; i++) weights[i] = pl_weight((*w)[i]);
    }
    static std::vector<int32_t> dense(const int32_t *word, int Kp, int W) {
        std::vector<int32_t> t(W, 0);
        for (int i = 0; i < Kp; i++)
            if (word[i] >= 0) t[word[i]]++;
        return t;
    }
    void add(const std::vector<uint8_t> &desc, const std::vector<int32_t> &n, int Fr, int Kp) {
        std::vector<int32_t> word, dist;
        assign(desc, n, Fr, Kp, vocab, W, word, dist);
        for (int f = 0; f < Fr; f++) {
            const std::vector<int32_t> t = dense(&word[(size_t)f * Kp], Kp, W);
            for (int w = 0; w < W; w++)
                if (t[w]) {
                    words.push_back(w);
                    tf.push_back(t[w]);
                    df[w]++;
                }
            offsets.push_back((int32_t)words.size());
        }
    }
    int norm(int e) const {
        int s = 0;
        for (int j = offsets[e]; j < offsets[e + 1]; j++) s += weights[words[j]] * tf[j];
        return s;
    }
};

int main(int argc, char **argv) {
    if (argc != 3 || !(fin = fopen(argv[1], "rb")) || !(fout = fopen(argv[2], "wb"))) return 2;
    const int ops = rd1();
    for (int o = 0; o < ops; o++) {
        const int op = rd1(), a = rd1(), b = rd1(), c = rd1();
        if (op == 0) {   // assign: frames, kp_stride, n_words
            const auto desc = rd<uint8_t>((size_t)a * b * 32);
            const auto n = rd<int32_t>(a);
            const auto vocab = rd<uint8_t>((size_t)c * 32);
            std::vector<int32_t> word, dist;
            assign(desc, n, a, b, vocab, c, word, dist);
            wr(word);
            wr(dist);
        } else if (op == 1) {   // train: n, n_words, iterations
            const int n = a, W = b;
            const auto desc = rd<uint8_t>((size_t)n * 32);
            std::vector<uint8_t> vocab((size_t)W * 32);
            for (int w = 0; w < W; w++) memcpy(&vocab[(size_t)w * 32], &desc[(size_t)pl_start(w, n, W) * 32], 32);
            std::vector<int32_t> sizes(W, 0), one(1, n), word, dist;
            for (int it = 0; it < c; it++) {
                assign(desc, one, 1, n, vocab, W, word, dist);
                sizes.assign(W, 0);
                std::vector<int32_t> ones((size_t)W * 256, 0);
                for (int i = n - 1; i >= 0; i--) {
                    sizes[word[i]]++;
                    for (int k = 0; k < 256; k++) ones[(size_t)word[i] * 256 + k] += (desc[(size_t)i * 32 + (k >> 3)] >> (k & 7)) & 1;
                }
                for (int w = 0; w < W; w++) {
                    if (!sizes[w]) continue;
                    for (int k = 0; k < 256; k++) {
                        uint8_t &byte = vocab[(size_t)w * 32 + (k >> 3)];
                        byte = (uint8_t)((byte & ~(1u << (k & 7))) | ((pl_majority(ones[(size_t)w * 256 + k], sizes[w]) ? 1u : 0u) << (k & 7)));
                    }
                }
            }
            wr(vocab);
            wr(sizes);
        } else {   // index: n_words, adds, top_k
            Index ix;
            ix.W = a;
            ix.vocab = rd<uint8_t>((size_t)a * 32);
            ix.df.assign(a, 0);
            std::vector<int32_t> w0, w1;
            const bool has0 = rd1();
            if (has0) w0 = rd<int32_t>(a);
            const bool has1 = rd1();
            if (has1) w1 = rd<int32_t>(a);
            ix.set_weights(has0 ? &w0 : nullptr);
            for (int k = 0; k < b; k++) {
                const int Fr = rd1(), Kp = rd1();
                const auto desc = rd<uint8_t>((size_t)Fr * Kp * 32);
                const auto n = rd<int32_t>(Fr);
                ix.add(desc, n, Fr, Kp);
            }
            if (has1) ix.set_weights(&w1);
            const int Q = rd1(), Kp = rd1(), has_below = rd1(), top_k = c, size = ix.size();
            const auto desc = rd<uint8_t>((size_t)Q * Kp * 32);
            const auto n = rd<int32_t>(Q);
            std::vector<int32_t> below;
            if (has_below) below = rd<int32_t>(Q);
            std::vector<int32_t> norms(size), word, dist;
            for (int e = 0; e < size; e++) norms[e] = ix.norm(e);
            assign(desc, n, Q, Kp, ix.vocab, ix.W, word, dist);
            std::vector<int32_t> bid((size_t)Q * top_k, -1), bs((size_t)Q * top_k, 0), bd((size_t)Q * top_k, 0), qn(Q, 0);
            for (int q = 0; q < Q; q++) {
                const std::vector<int32_t> t = Index::dense(&word[(size_t)q * Kp], Kp, ix.W);
                for (int w = 0; w < ix.W; w++) qn[q] += ix.weights[w] * t[w];
                const int lim = has_below ? (below[q] < 0 ? 0 : (below[q] > size ? size : below[q])) : size;
                int ps = 0, pd = 0, pi = -1;
                for (int k = 0; k < top_k; k++) {
                    int s1 = 0, d1 = 0, i1 = -1;
                    for (int e = lim - 1; e >= 0; e--) {   // descending: the tie rule has to come from pl_before
                        int s = 0;
                        for (int j = ix.offsets[e]; j < ix.offsets[e + 1]; j++) s += pl_term(ix.weights[ix.words[j]], t[ix.words[j]], ix.tf[j]);
                        const int d = qn[q] > norms[e] ? qn[q] : norms[e];
                        if (s <= 0 || d <= 0) continue;
                        if (pi >= 0 && !pl_before(ps, pd, pi, s, d, e)) continue;
                        if (i1 < 0 || pl_before(s, d, e, s1, d1, i1)) {
                            s1 = s;
                            d1 = d;
                            i1 = e;
                        }
                    }
                    if (i1 < 0) break;
                    ps = s1;
                    pd = d1;
                    pi = i1;
                    bid[(size_t)q * top_k + k] = i1;
                    bs[(size_t)q * top_k + k] = s1;
                    bd[(size_t)q * top_k + k] = d1;
                }
            }
            std::vector<int32_t> sz(1, size);
            wr(sz);
            wr(ix.offsets);
            wr(ix.words);
            wr(ix.tf);
            wr(ix.df);
            wr(norms);
            wr(bid);
            wr(bs);
            wr(bd);
            wr(qn);
        }
    }
    fclose(fout);
    return 0;
}
