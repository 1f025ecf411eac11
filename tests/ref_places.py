"""include/vslam_places.h restated from its text alone, in numpy and Python integers: a popcount table for the distances, argmin (ties
to the first index) for the assignment, Python ints for the scores and the products of the ranking.  Nothing here knows how the
device does it."""
import numpy as np

POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)
POP16 = (POP8[np.arange(65536) & 255] + POP8[np.arange(65536) >> 8]).astype(np.uint8)   # the table, 16 bits at a time
MAX_WORDS = 16384


def distances(desc, vocab):
    """desc (n, 32) u8, vocab (W, 32) u8 -> (n, W) int32 Hamming distances"""
    desc = np.ascontiguousarray(np.asarray(desc, np.uint8).reshape(-1, 32)).view(np.uint16)
    vocab = np.ascontiguousarray(np.asarray(vocab, np.uint8).reshape(-1, 32)).view(np.uint16)
    out = np.empty((len(desc), len(vocab)), np.int32)
    step = max(1, (1 << 21) // max(len(vocab), 1))
    for lo in range(0, len(desc), step):
        out[lo:lo + step] = POP16[desc[lo:lo + step, None, :] ^ vocab[None, :, :]].sum(2, dtype=np.int32)
    return out


def assign_rows(desc, vocab):
    """-> word, dist (n,) int32: the smallest distance, ties to the lowest word"""
    d = distances(desc, vocab)
    if d.shape[0] == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    w = np.argmin(d, axis=1)
    return w.astype(np.int32), d[np.arange(len(w)), w].astype(np.int32)


def assign(desc, n, vocab):
    """desc (frames, kp_stride, 32), n (frames,) -> word, dist (frames, kp_stride) int32, -1 at or past the count"""
    desc = np.asarray(desc, np.uint8)
    Fr, Kp = desc.shape[:2]
    word, dist = np.full((Fr, Kp), -1, np.int32), np.full((Fr, Kp), -1, np.int32)
    for f in range(Fr):
        c = min(max(int(n[f]), 0), Kp)
        word[f, :c], dist[f, :c] = assign_rows(desc[f, :c], vocab)
    return word, dist


def train(desc, n_words, iterations):
    """k-majority -> vocab (n_words, 32) u8, sizes (n_words,) int32"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc)
    assert 1 <= n_words <= n and 0 <= iterations <= 64
    vocab = np.stack([desc[(w * n) // n_words] for w in range(n_words)]).copy()
    sizes = np.zeros(n_words, np.int32)
    bits = np.unpackbits(desc, axis=1, bitorder="little").astype(np.int64)   # (n, 256): bit k = bit k & 7 of byte k >> 3
    for _ in range(iterations):
        word, _ = assign_rows(desc, vocab)
        sizes = np.bincount(word, minlength=n_words).astype(np.int32)
        for w in np.nonzero(sizes)[0]:
            ones = bits[word == w].sum(0)
            vocab[w] = np.packbits((2 * ones > int(sizes[w])).astype(np.uint8), bitorder="little")
    return vocab, sizes


def weights_clamped(weights, n_words):
    if weights is None:
        return np.ones(n_words, np.int64)
    return np.clip(np.asarray(weights, np.int64), 0, 65535)


def places_weights(df, n_entries):
    """rint(1024 ln(n_entries / df)) where df > 0, else 0, clipped to 65535 -- float64, on the host"""
    df = np.asarray(df, np.int64)
    w = np.zeros(df.shape, np.float64)
    pos = df > 0
    w[pos] = np.rint(1024.0 * np.log(np.float64(n_entries) / df[pos].astype(np.float64)))
    return np.clip(w, 0, 65535).astype(np.int32)


def term_counts(word_row):
    """a frame's assigned words (the -1 rows dropped) -> {word: tf}"""
    w = np.asarray(word_row)
    w = w[w >= 0]
    u, c = np.unique(w, return_counts=True)
    return {int(a): int(b) for a, b in zip(u, c)}


class Index:
    """the index of section 3"""

    def __init__(self, n_words, capacity, max_kp):
        self.n_words, self.capacity, self.max_kp = n_words, capacity, max_kp
        self.vocab, self.weights = None, np.ones(n_words, np.int64)
        self.reset()

    def reset(self):
        self.entries, self.tags = [], []   # entries: {word: tf}
        self.df = np.zeros(self.n_words, np.int32)

    @property
    def size(self):
        return len(self.entries)

    def set_vocabulary(self, vocab, weights=None):
        assert self.size == 0
        self.vocab = np.asarray(vocab, np.uint8).reshape(self.n_words, 32).copy()
        self.set_weights(weights)

    def set_weights(self, weights=None):
        self.weights = weights_clamped(weights, self.n_words)

    def add(self, desc, n, tags=None):
        desc = np.asarray(desc, np.uint8)
        Fr, Kp = desc.shape[:2]
        if self.size + Fr > self.capacity or Kp > self.max_kp:
            return None   # VSLAM_ERR_CAPACITY, nothing changes
        word, _ = assign(desc, n, self.vocab)
        ids = []
        for f in range(Fr):
            tf = term_counts(word[f])
            ids.append(self.size)
            self.entries.append(tf)
            self.tags.append((0, 0) if tags is None else (int(tags[f][0]), int(tags[f][1])))
            for w in tf:
                self.df[w] += 1
        return np.array(ids, np.int32)

    def norm(self, tf):
        return sum(int(self.weights[w]) * c for w, c in tf.items())

    def score(self, tf_q, tf_e):
        return sum(int(self.weights[w]) * min(c, tf_e[w]) for w, c in tf_q.items() if w in tf_e)

    def query(self, desc, n, top_k, below=None):
        """-> best_id, best_score, best_den (queries, top_k), q_norm (queries,) int32"""
        desc = np.asarray(desc, np.uint8)
        Q = desc.shape[0]
        word, _ = assign(desc, n, self.vocab)
        ids, sc, dn = np.full((Q, top_k), -1, np.int32), np.zeros((Q, top_k), np.int32), np.zeros((Q, top_k), np.int32)
        qn = np.zeros(Q, np.int32)
        norms = [self.norm(e) for e in self.entries]
        for q in range(Q):
            tf_q = term_counts(word[q])
            nq = self.norm(tf_q)
            qn[q] = nq
            lim = self.size if below is None else min(max(int(below[q]), 0), self.size)
            cand = []
            for e in range(lim):
                s, d = self.score(tf_q, self.entries[e]), max(nq, norms[e])
                if s > 0 and d > 0:
                    cand.append((s, d, e))
            order = rank(cand)
            for k, (s, d, e) in enumerate(order[:top_k]):
                ids[q, k], sc[q, k], dn[q, k] = e, s, d
        return ids, sc, dn, qn

    def view(self):
        offsets = np.zeros(self.size + 1, np.int32)
        words, tf = [], []
        for e, ent in enumerate(self.entries):
            for w in sorted(ent):
                words.append(w)
                tf.append(ent[w])
            offsets[e + 1] = len(words)
        return dict(size=self.size, offsets=offsets, words=np.array(words, np.int32).reshape(-1), tf=np.array(tf, np.int32).reshape(-1),
                    df=self.df.copy(), norms=np.array([self.norm(e) for e in self.entries], np.int32).reshape(-1),
                    tags=np.array(self.tags, np.int32).reshape(-1, 2), weights=self.weights.astype(np.int32),
                    vocab=None if self.vocab is None else self.vocab.copy())


def before(a, b):
    """candidate a = (score, den, id) comes before b: score_a den_b > score_b den_a in unsigned 64 bits, then the lower id"""
    l, r = a[0] * b[1], b[0] * a[1]
    assert 0 <= l < 1 << 64 and 0 <= r < 1 << 64
    return l > r or (l == r and a[2] < b[2])


def rank(cand):
    """the candidates in order (an insertion sort by `before`: the header's comparison and nothing else)"""
    out = []
    for c in cand:
        k = len(out)
        while k > 0 and before(c, out[k - 1]):
            k -= 1
        out.insert(k, c)
    return out
