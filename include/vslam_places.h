/* Place recognition: every descriptor quantised to its nearest word of a flat binary vocabulary, every frame a sparse histogram of
 * words, histograms compared -- "which earlier frames look like this one?", the question loop closure, relocalisation across tracks
 * and map merging start from.  Explicit calls: nothing in vslam_amd.h, vslam_resect.h, vslam_adjust.h, vslam_search.h, vslam_pnp.h,
 * vslam_fuse.h or vslam_tracks.h launches a kernel of this file while they are unused, and no existing output changes a bit.
 *
 * THIS TEXT and tests/ref_places.py are the contract.  Everything is an integer: distances, assignments, term counts, majority
 * votes, scores and the ranking.  A result is a function of the arguments (and the index) alone: the same in every run, batch size
 * and batch slot, and the order in which threads arrive never matters (only integer sums are accumulated).
 * A descriptor and a word are 256 bits, 32 bytes; bit k is bit k & 7 of byte k >> 3.  dist(a, b) = the number of differing bits.
 *
 * ---- 1. vslam_places_assign: words of descriptors
 * d_desc [frames][kp_stride][32], d_n [frames], d_vocab [n_words][32].  n = d_n[f] clamped to 0 .. kp_stride.  For i < n:
 *   d_word[f][i] = the w with the smallest dist(desc[f][i], vocab[w]); ties go to the LOWEST w.  d_dist[f][i] = that distance.
 * For n <= i < kp_stride: d_word[f][i] = -1 and d_dist[f][i] = -1.  d_dist may be NULL.
 * On the matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4): a bit becomes the E2M1 nibble +1.0 (0) or -1.0 (1), so the dot product of
 * two rows is 256 - 2 dist, an exact f32 sum of +-1 products; the running best per result is the float key dot x 16384 - w, largest
 * first.  With |dot| <= 256 and w <= 16383 = VSLAM_PLACES_MAX_WORDS - 1 every key is an integer below 2^23 in magnitude: exact.  The
 * vocabulary is spread to nibbles once per call (once per vslam_places_set_vocabulary for an index), every workgroup streams the
 * same spread rows through LDS, and the last tile of an n_words that is no multiple of 32 is filled with the spread of an all-zero
 * word in columns that carry an index of 2^25 and so lose to every word, whatever their dot product.
 * Workspace: "places.spread", ceil(n_words / 32) x 32 x 128 bytes, written by the call before it is read.
 * Refusals, before anything is queued.  VSLAM_ERR_INVALID: a null pointer (d_dist may be); frames or kp_stride not positive; n_words
 * outside 1 .. VSLAM_PLACES_MAX_WORDS; d_desc or d_vocab off 16 bytes; d_n, d_word or d_dist off 4.  VSLAM_ERR_CAPACITY: kp_stride >
 * VSLAM_MAX_KP; frames x ceil(kp_stride / 256) of 2^31 or more (one workgroup each; add and query refuse the same).
 *
 * ---- 2. vslam_places_train: a vocabulary by k-majority
 * d_desc [n][32].  START: word w = descriptor (w x n) / n_words (the product in 64 bits, integer division).  `iterations` times:
 * every descriptor is assigned by rule 1 against the current words; then every word with members becomes their per-bit majority,
 * bit = 1 iff 2 x ones > members (a tie gives 0); a word without members keeps its bits.  d_sizes [n_words] = the member counts of
 * the LAST assignment made (they belong to the words BEFORE the last update); iterations = 0 returns the start with d_sizes all 0.
 * The members of a word are gathered by a counting sort (histogram, scan, scatter; the order inside a word is whatever the atomics
 * give and only integer sums read it) and one wave per word counts the bits.
 * Workspace: "places.spread" as above, "places.train" (n x 8 + n_words x 8 + 4 bytes), all written or cleared by the call.
 * Refusals.  VSLAM_ERR_INVALID: a null pointer; n_words outside 1 .. VSLAM_PLACES_MAX_WORDS; n < n_words; iterations outside 0 .. 64;
 * d_desc or d_vocab off 16 bytes; d_sizes off 4; d_vocab overlapping d_desc.  VSLAM_ERR_CAPACITY: n > VSLAM_PLACES_MAX_TRAIN (2^24).
 *
 * ---- 3. vslam_places: an index of frames
 * vslam_places_create(ctx, n_words, capacity, max_kp, &out): 1 <= n_words <= VSLAM_PLACES_MAX_WORDS, 1 <= capacity <=
 * VSLAM_PLACES_MAX_ENTRIES (2^20), 1 <= max_kp <= VSLAM_MAX_KP; the index owns its device memory (an entry has at most min(max_kp,
 * n_words) distinct words: capacity x that many (word, tf) pairs are reserved, and a product of 2^31 or more is VSLAM_ERR_CAPACITY,
 * as are a capacity or max_kp above their limits; the other bounds are VSLAM_ERR_INVALID).  It starts EMPTY and WITHOUT a vocabulary; all its
 * weights are 1.  _destroy waits for the context's stream.  _reset: size = 0, df = 0; the vocabulary and the weights stay.
 * _set_vocabulary(d_vocab [n_words][32], d_weights [n_words] int32 or NULL = all 1): copies the words, spreads them and keeps the FP4
 * form; allowed only while the index is empty (size = 0), otherwise VSLAM_ERR_INVALID.  _set_weights(d_weights or NULL = all 1):
 * allowed at any time.  A weight is CLAMPED to 0 .. 65535 as it is copied (the host never reads it).
 * vslam_places_add: the frames, assigned by rule 1, become entries with ids size .. size + frames - 1 in argument order (written
 * to d_ids).  Per entry the index stores its distinct words ASCENDING with their term counts tf (the number of the frame's
 * descriptors assigned to the word), and its tag d_tags[f] (two int32; (0, 0) for NULL).  df[w] = the number of entries that contain
 * w.  size + frames > capacity or kp_stride > max_kp: VSLAM_ERR_CAPACITY and nothing changes (`size` is host state: the test is on
 * the host).  A frame with 0 descriptors is a valid empty entry.  VSLAM_ERR_INVALID: no vocabulary set; a null pointer (d_tags may
 * be); frames or kp_stride not positive; d_desc off 16 bytes; another array off 4.
 * vslam_places_query: with tf_q of a query frame by rule 1 and weight[] as the index holds it AT THE CALL,
 *   score(q, e) = sum over w of weight[w] x min(tf_q[w], tf_e[w]);  norm(x) = sum over w of weight[w] x tf_x[w];
 *   den(q, e) = max(norm(q), norm(e)).   (score / den is the similarity, in [0, 1].)
 * The candidates of q are the entries e < size with e < d_below[q] (d_below NULL: all), score > 0 and den > 0.  a comes BEFORE b iff
 * score_a x den_b > score_b x den_a, both products in unsigned 64 bits; on equality the lower id comes first.  PROOF OF THE BOUND: a
 * frame has at most kp_stride <= VSLAM_MAX_KP = 2^14 descriptors, so the tf of a frame sum to at most 2^14; a weight is at most 65535
 * < 2^16; so norm <= 65535 x 2^14 < 2^30, score <= norm(q) and den is a norm: every factor is below 2^30 < 2^31 and every product
 * below 2^60.  The first top_k (1 .. 16) candidates are written as d_best_id, d_best_score, d_best_den [queries][top_k]; the places
 * behind the last candidate hold -1, 0, 0.  d_q_norm [queries] = norm(q).  Nothing of the index changes.
 * VSLAM_ERR_INVALID: no vocabulary; a null pointer (d_below may be); queries or kp_stride not positive; top_k outside 1 .. 16; d_desc
 * off 16 bytes, another array off 4.  VSLAM_ERR_CAPACITY: kp_stride > max_kp; queries > 65535.
 * vslam_places_view: the index as device arrays (they stay the index's; valid until it is destroyed): d_offsets [capacity + 1] (the
 * CSR of entries: entry e owns rows offsets[e] .. offsets[e + 1] - 1 of d_words / d_tf; offsets[0] = 0), d_df [n_words], d_norms
 * [capacity] (entry norms under the weights at THIS call: the call queues their computation; rows at or past size are not written),
 * d_tags [capacity][2], d_weights [n_words], d_vocab [n_words][32]; size, n_words, capacity, max_kp from the host.
 * Workspace of add and query from the context's arena: "places.word" (frames x kp_stride x 4), "places.entry" (add: frames x (2
 * min(kp_stride, n_words) + 1) x 4), "places.score" (query: (queries x size + 1) x 4) -- written before read.
 * All calls are asynchronous on the context's stream and synchronise nothing, except where stated (_destroy).
 *
 * Left open: no geometric verification of a candidate inside the library; no Sim(3) / pose-graph correction; no policy for when a
 * frame is added; the quality of such a vocabulary on real footage is unknown (synthetic scenes only).                            */
#ifndef VSLAM_PLACES_H
#define VSLAM_PLACES_H

#include "vslam_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_PLACES_MAX_WORDS 16384
#define VSLAM_PLACES_MAX_TRAIN (1 << 24)
#define VSLAM_PLACES_MAX_ENTRIES (1 << 20)
#define VSLAM_PLACES_MAX_TOP_K 16

int vslam_places_assign(vslam_ctx *ctx, const uint8_t *d_desc /* [frames][kp_stride][32] */, const int32_t *d_n /* [frames] */,
                        int kp_stride, int frames, const uint8_t *d_vocab /* [n_words][32] */, int n_words,
                        int32_t *d_word /* [frames][kp_stride] */, int32_t *d_dist /* [frames][kp_stride] or NULL */);

int vslam_places_train(vslam_ctx *ctx, const uint8_t *d_desc /* [n][32] */, int n, int n_words, int iterations,
                       uint8_t *d_vocab /* out [n_words][32] */, int32_t *d_sizes /* out [n_words] */);

typedef struct vslam_places vslam_places;
typedef struct vslam_places_arrays {
    int32_t n_words, capacity, max_kp, size;
    const int32_t *d_offsets;   /* [capacity + 1] */
    const int32_t *d_words;     /* [offsets[size]] ascending inside an entry */
    const int32_t *d_tf;        /* [offsets[size]]                           */
    const int32_t *d_df;        /* [n_words]                                 */
    const int32_t *d_norms;     /* [capacity], rows < size, weights of this call */
    const int32_t *d_tags;      /* [capacity][2]                             */
    const int32_t *d_weights;   /* [n_words]                                 */
    const uint8_t *d_vocab;     /* [n_words][32]                             */
} vslam_places_arrays;

int vslam_places_create(vslam_ctx *ctx, int n_words, int capacity, int max_kp, vslam_places **out);
int vslam_places_destroy(vslam_ctx *ctx, vslam_places *idx);
int vslam_places_reset(vslam_ctx *ctx, vslam_places *idx);
int vslam_places_set_vocabulary(vslam_ctx *ctx, vslam_places *idx, const uint8_t *d_vocab, const int32_t *d_weights /* or NULL */);
int vslam_places_set_weights(vslam_ctx *ctx, vslam_places *idx, const int32_t *d_weights /* or NULL: all 1 */);
int vslam_places_add(vslam_ctx *ctx, vslam_places *idx, const uint8_t *d_desc, const int32_t *d_n, int kp_stride, int frames,
                     const int32_t *d_tags /* [frames][2] or NULL */, int32_t *d_ids /* out [frames] */);
int vslam_places_query(vslam_ctx *ctx, vslam_places *idx, const uint8_t *d_desc, const int32_t *d_n, int kp_stride, int queries,
                       const int32_t *d_below /* [queries] or NULL */, int top_k, int32_t *d_best_id, int32_t *d_best_score,
                       int32_t *d_best_den /* [queries][top_k] each */, int32_t *d_q_norm /* [queries] */);
int vslam_places_view(vslam_ctx *ctx, vslam_places *idx, vslam_places_arrays *out);

#ifdef __cplusplus
}
#endif

#endif
