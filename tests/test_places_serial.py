"""What the place-recognition kernels compile (vslam_amd/csrc/places_math.h: the distance, the rule of assignment and the float key that
stands for it, where training starts, the majority vote, the clamp of a weight, a score's term and the order of candidates) built
for the host as a stand-alone program with -fsanitize=address,undefined and walked serially (tests/native/places_serial.cpp, against
the order of the reference's walks), held bit for bit to tests/ref_places.py."""
import numpy as np
import pytest

import places_cases as pc
import ref_places as rp


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pc.build_serial(tmp_path_factory.mktemp("serial"))


def same(got, want, name):
    for k, w in want.items():
        g = got[k]
        assert np.array_equal(np.asarray(g), np.asarray(w)), (name, k)


def test_assignment_on_the_serial_walk(exe, tmp_path):
    ops, want = [], []
    for W, Kp, counts in ((1, 40, [40]), (33, 70, [0, 1, 70]), (257, 40, [39]), (64, 64, [64, 99, -2])):
        vocab = pc.awkward_vocab(W, W)
        desc, n = pc.frames_for(10 + W, vocab, len(counts), Kp, counts)
        ops.append(dict(op="assign", desc=desc, n=n, vocab=vocab))
        word, dist = rp.assign(desc, n, vocab)
        want.append(dict(word=word, dist=dist))
    for o, g, w in zip(ops, pc.run_serial(exe, tmp_path, ops), want):
        same(g, w, len(o["vocab"]))
        assert (g["dist"][g["word"] >= 0] <= 256).all()
    assert any((w["dist"] == 0).any() for w in want) and any((w["dist"] == 256).any() for w in want)


def test_the_key_is_exact_at_the_last_word(exe, tmp_path):
    W = rp.MAX_WORDS
    vocab = pc.random_desc(3, (W,))
    vocab[W - 1] = vocab[W - 2] = ~vocab[0]
    desc = np.stack([vocab[W - 1], vocab[0], ~vocab[5], vocab[W - 3]])[None]
    g = pc.run_serial(exe, tmp_path, [dict(op="assign", desc=desc, n=[4], vocab=vocab)])[0]
    word, dist = rp.assign(desc, [4], vocab)
    same(g, dict(word=word, dist=dist), "top")
    assert word[0].tolist()[:2] == [W - 2, 0] and word[0, 3] == W - 3 and dist[0].tolist()[:2] == [0, 0]


def test_training_on_the_serial_walk(exe, tmp_path):
    cases = [(pc.clustered(1, 33, 5), 33, 1), (pc.clustered(2, 34, 5), 33, 4), (pc.clustered(3, 400, 20), 64, 4), (pc.clustered(4, 64, 3), 1, 2),
             (pc.random_desc(5, (90,)), 7, 0), (np.repeat(pc.random_desc(6, (1,)), 50, 0), 9, 3)]
    got = pc.run_serial(exe, tmp_path, [dict(op="train", desc=d, n_words=W, iterations=it) for d, W, it in cases])
    for (d, W, it), g in zip(cases, got):
        vocab, sizes = rp.train(d, W, it)
        same(g, dict(vocab=vocab, sizes=sizes), (len(d), W, it))
    assert got[-1]["sizes"].tolist() == [50] + [0] * 8


def test_the_index_and_its_query_on_the_serial_walk(exe, tmp_path):
    rng = np.random.default_rng(8)
    ops, want = [], []
    for W, Kp, entries, Q, top_k, below, weights in ((33, 60, 40, 5, 3, None, None), (64, 50, 70, 9, 16, "mid", "idf"), (5, 30, 12, 3, 1, "mid", "zero"),
                                                     (16, 40, 30, 4, 16, None, "max")):
        vocab = pc.awkward_vocab(W + 1, W)
        desc, n = pc.frames_for(W, vocab, entries, Kp, [Kp, 0, 1, Kp - 1, Kp // 2])
        desc[entries // 2] = desc[1 + entries // 2]    # entries with equal scores: the lower id first
        n[entries // 2] = n[1 + entries // 2]
        cuts = [0, entries // 3, 2 * entries // 3, entries]
        adds = [(desc[a:b], n[a:b]) for a, b in zip(cuts, cuts[1:])]
        qd, qn = desc[rng.integers(0, entries, Q)], np.full(Q, Kp - 2, np.int32)
        ref = rp.Index(W, entries, Kp)
        ref.set_vocabulary(vocab)
        for d, c in adds:
            ref.add(d, c)
        qw = {None: None, "idf": rp.places_weights(ref.df, ref.size), "zero": np.zeros(W, np.int32), "max": np.full(W, 70000, np.int32)}[weights]
        ref.set_weights(qw)
        bl = None if below is None else rng.integers(-1, entries + 3, Q).astype(np.int32)
        ids, sc, dn, qnorm = ref.query(qd, qn, top_k, bl)
        v = ref.view()
        ops.append(dict(op="index", n_words=W, vocab=vocab, weights=None, adds=adds, query_weights=qw, query=(qd, qn), top_k=top_k, below=bl))
        want.append(dict(size=v["size"], offsets=v["offsets"], words=v["words"], tf=v["tf"], df=v["df"], norms=v["norms"], best_id=ids,
                         best_score=sc, best_den=dn, q_norm=qnorm))
    for k, (g, w) in enumerate(zip(pc.run_serial(exe, tmp_path, ops), want)):
        same(g, w, k)
    assert (want[0]["best_id"] >= 0).any() and (want[2]["best_id"] == -1).all()
