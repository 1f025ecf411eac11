// The C++ surfaces of include/vslam_places.h (include/vslam/helpers.h: vslam::places_assign, vslam::places_train, vslam::Places) on
// one batch of frames: assign against a given vocabulary, train one of the same size, index the frames under the trained words and
// query them.  tests/test_gpu_places.py compares the output with the reference and with the C entry points' bits.
//   in : W Kp Fr iterations top_k | vocab [W][32] | desc [Fr][Kp][32] | n [Fr] | below [Fr]
//   out: word, dist [Fr][Kp] | trained vocab [W][32], sizes [W] | ids [Fr] | best_id, best_score, best_den [Fr][top_k] | q_norm [Fr]
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "vslam/helpers.h"

template <typename T>
static T *upload(vslam_ctx *ctx, const std::vector<T> &h) {
    void *d = nullptr;
    if (vslam_dev_alloc(ctx, sizeof(T) * (h.empty() ? 1 : h.size()), &d) || (!h.empty() && vslam_copy_h2d(ctx, d, h.data(), sizeof(T) * h.size())))
        throw std::runtime_error("upload");
    return static_cast<T *>(d);
}
template <typename T>
static void download(vslam_ctx *ctx, FILE *f, const T *d, size_t n) {
    std::vector<T> h(n);
    if (vslam_copy_d2h(ctx, h.data(), d, sizeof(T) * n)) throw std::runtime_error("download");
    fwrite(h.data(), sizeof(T), n, f);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fin = fopen(argv[1], "rb"), *fout = fopen(argv[2], "wb");
    if (!fin || !fout) return 2;
    int hdr[5];
    if (fread(hdr, sizeof(int), 5, fin) != 5) return 2;
    const int W = hdr[0], Kp = hdr[1], Fr = hdr[2], iterations = hdr[3], top_k = hdr[4];
    std::vector<unsigned char> vocab((size_t)W * 32), desc((size_t)Fr * Kp * 32);
    std::vector<s32> n(Fr), below(Fr);
    if (fread(vocab.data(), 1, vocab.size(), fin) != vocab.size() || fread(desc.data(), 1, desc.size(), fin) != desc.size() ||
        fread(n.data(), 4, Fr, fin) != (size_t)Fr || fread(below.data(), 4, Fr, fin) != (size_t)Fr)
        return 2;
    vslam_ctx *ctx = nullptr;
    if (vslam_ctx_create(0, &ctx)) return 3;
    try {
        unsigned char *d_vocab = upload(ctx, vocab), *d_desc = upload(ctx, desc);
        s32 *d_n = upload(ctx, n), *d_below = upload(ctx, below);
        s32 *d_word = upload(ctx, std::vector<s32>((size_t)Fr * Kp)), *d_dist = upload(ctx, std::vector<s32>((size_t)Fr * Kp));
        vslam::places_assign(ctx, d_desc, d_n, Kp, Fr, d_vocab, W, d_word, d_dist);
        download(ctx, fout, d_word, (size_t)Fr * Kp);
        download(ctx, fout, d_dist, (size_t)Fr * Kp);

        unsigned char *d_trained = upload(ctx, std::vector<unsigned char>((size_t)W * 32));
        s32 *d_sizes = upload(ctx, std::vector<s32>(W));
        vslam::places_train(ctx, d_desc, Fr * Kp, W, iterations, d_trained, d_sizes);
        download(ctx, fout, d_trained, (size_t)W * 32);
        download(ctx, fout, d_sizes, W);

        s32 *d_ids = upload(ctx, std::vector<s32>(Fr));
        s32 *d_best[3];
        for (auto &p : d_best) p = upload(ctx, std::vector<s32>((size_t)Fr * top_k));
        s32 *d_qn = upload(ctx, std::vector<s32>(Fr));
        {
            vslam::Places idx(ctx, W, Fr, Kp);
            idx.set_vocabulary(d_trained);
            idx.add(d_desc, d_n, Kp, Fr, nullptr, d_ids);
            bool thrown = false;
            try {
                idx.set_vocabulary(d_vocab);   // not empty any more
            } catch (const std::runtime_error &) {
                thrown = true;
            }
            if (!thrown || idx.view().size != Fr) return 4;
            idx.query(d_desc, d_n, Kp, Fr, d_below, top_k, d_best[0], d_best[1], d_best[2], d_qn);
            download(ctx, fout, d_ids, Fr);
            for (auto p : d_best) download(ctx, fout, p, (size_t)Fr * top_k);
            download(ctx, fout, d_qn, Fr);
        }
        for (void *p : {(void *)d_vocab, (void *)d_desc, (void *)d_n, (void *)d_below, (void *)d_word, (void *)d_dist, (void *)d_trained, (void *)d_sizes,
                        (void *)d_ids, (void *)d_best[0], (void *)d_best[1], (void *)d_best[2], (void *)d_qn})
            vslam_dev_free(ctx, p);
    } catch (const std::exception &e) {
        fprintf(stderr, "places_demo: %s\n", e.what());
        return 5;
    }
    fclose(fout);
    vslam_ctx_destroy(ctx);
    return 0;
}
