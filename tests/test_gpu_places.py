"""include/vslam_places.h on the device, bit for bit against tests/ref_places.py: words of descriptors, k-majority training, the index
and its query; the 320 x 240 fixture end to end through the device extractor; refusals, workspace and stream order."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import entry_calls as ec
import places_calls as plc
import places_cases as pc
import ref_places as rp
from offset_views import sentinel_fill
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = -1, -4


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h(t):
    return t.cpu().numpy()


def test_header_symbols(ctx):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_places.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.PLACES_SYMBOLS) and set(plc.ENTRIES) <= set(names)
    others = (set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS) | set(capi.SEARCH_SYMBOLS) | set(capi.PNP_SYMBOLS)
              | set(capi.FUSE_SYMBOLS) | set(capi.TRACK_SYMBOLS))
    assert not set(names) & others
    for nm in names:
        assert hasattr(ctx.lib, nm), nm
    assert capi.PLACES_MAX_WORDS == rp.MAX_WORDS == 16384


# ---------------------------------------------------------------------------------------------------------------- assign
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 300]


def _assign_same(ctx, desc, n, vocab):
    o = ctx.places_assign(_t(desc), _t(n), _t(vocab))
    ctx.synchronize()
    word, dist = rp.assign(desc, n, vocab)
    assert np.array_equal(_h(o["word"]), word) and np.array_equal(_h(o["dist"]), dist)
    return word, dist


@pytest.mark.parametrize("frames", [1, 9])
@pytest.mark.parametrize("n_words", [1, 31, 32, 33, 64, 65, 257])
def test_assign(ctx, n_words, frames):
    vocab = pc.awkward_vocab(n_words, n_words)
    desc, n = pc.frames_for(100 + n_words, vocab, frames, 300, COUNTS if frames > 1 else [257])
    word, dist = _assign_same(ctx, desc, n, vocab)
    assert (dist == 0).any() and (word[:, -1] == -1).any()
    if n_words == 1:
        assert (dist == 256).any()
    if n_words >= 4:
        assert not (word == n_words - 1).any() and (word == 1).any()   # the duplicate of word 1 never wins


def test_assign_counts_are_clamped_and_dist_is_optional(ctx):
    vocab = pc.awkward_vocab(5, 40)
    desc, n = pc.frames_for(6, vocab, 3, 70, [-3, 999, 70])
    _assign_same(ctx, desc, n, vocab)
    o = ctx.places_assign(_t(desc), _t(n), _t(vocab), want_dist=False)
    ctx.synchronize()
    assert np.array_equal(_h(o["word"]), rp.assign(desc, n, vocab)[0]) and "dist" not in o


def test_assign_key_is_exact_at_the_last_word(ctx):
    W = rp.MAX_WORDS
    vocab = pc.random_desc(3, (W,))
    vocab[W - 1] = vocab[W - 2] = ~vocab[0]
    desc, n = pc.frames_for(4, vocab[W - 64:], 2, 64, [64])
    desc[0, :4] = np.stack([vocab[W - 1], vocab[0], ~vocab[5], vocab[W - 3]])
    word, dist = _assign_same(ctx, desc, n, vocab)
    assert word[0, :4].tolist()[:2] == [W - 2, 0] and word[0, 3] == W - 3 and (word >= W - 64).sum() > 20


# ---------------------------------------------------------------------------------------------------------------- train
@pytest.mark.parametrize("n_words", [1, 33, 64])
def test_train(ctx, n_words):
    for n in (n_words, n_words + 1, 1000):
        desc = pc.clustered(n + n_words, n, max(n_words // 2, 1))
        for it in (0, 1, 4):
            vocab, sizes = rp.train(desc, n_words, it)
            o = ctx.places_train(_t(desc), n_words, it)
            again = ctx.places_train(_t(desc), n_words, it)
            ctx.synchronize()
            assert np.array_equal(_h(o["vocab"]), vocab) and np.array_equal(_h(o["sizes"]), sizes), (n, it)
            assert torch.equal(o["vocab"], again["vocab"]) and torch.equal(o["sizes"], again["sizes"])
            assert sizes.sum() == (n if it else 0)


def test_train_on_identical_descriptors_leaves_every_word_but_one_empty(ctx):
    desc = np.repeat(pc.random_desc(6, (1,)), 200, 0)
    o = ctx.places_train(_t(desc), 33, 4)
    ctx.synchronize()
    vocab, sizes = rp.train(desc, 33, 4)
    assert np.array_equal(_h(o["vocab"]), vocab) and np.array_equal(_h(o["sizes"]), sizes)
    assert sizes.tolist() == [200] + [0] * 32 and (vocab == desc[0]).all()


# ---------------------------------------------------------------------------------------------------------------- the index
def _views_equal(got, want):
    for k, w in want.items():
        if w is not None:
            assert np.array_equal(np.asarray(got[k]), np.asarray(w)), k


def _pair(ctx, n_words, capacity, max_kp, vocab, weights=None):
    idx, ref = capi.Places(ctx, n_words, capacity, max_kp), rp.Index(n_words, capacity, max_kp)
    idx.set_vocabulary(_t(vocab), None if weights is None else _t(weights))
    ref.set_vocabulary(vocab, weights)
    return idx, ref


def test_add_in_one_call_and_in_three_capacity_and_reset(ctx):
    W, Kp, E = 65, 70, 23
    vocab = pc.awkward_vocab(9, W)
    desc, n = pc.frames_for(10, vocab, E, Kp, [Kp, 0, 1, 64, 65, 30])
    tags = np.stack([np.arange(E) // 5, np.arange(E) % 5], 1).astype(np.int32)
    one, ref = _pair(ctx, W, E, Kp, vocab)
    three, _ = _pair(ctx, W, E, Kp, vocab)
    try:
        ids = one.add(_t(desc), _t(n), _t(tags))
        got_ids = [three.add(_t(desc[a:b]), _t(n[a:b]), _t(tags[a:b])) for a, b in ((0, 1), (1, 10), (10, E))]
        ctx.synchronize()
        assert np.array_equal(_h(ids), ref.add(desc, n, tags)) and np.array_equal(np.concatenate([_h(x) for x in got_ids]), np.arange(E))
        v1, v3, vr = one.view(), three.view(), ref.view()
        _views_equal(v1, vr)
        _views_equal(v3, vr)
        assert v1["size"] == E and (np.diff(vr["offsets"]) == 0).any(), "an empty frame is a valid entry"
        # the capacity is exactly reached: one more is refused and nothing changes
        ids1 = sentinel_fill(torch.empty(1, dtype=torch.int32, device="cuda"))
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            one.add(_t(desc[:1]), _t(n[:1]), out=ids1)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            one.set_vocabulary(_t(vocab))
        ctx.synchronize()
        assert (_h(ids1.view(torch.uint8)) == 0xA5).all()
        _views_equal(one.view(), vr)
        one.reset()
        assert one.view()["size"] == 0 and (one.view()["df"] == 0).all()
        one.set_vocabulary(_t(vocab))                       # allowed again
        one.add(_t(desc[3:9]), _t(n[3:9]))
        ref.reset()
        ref.add(desc[3:9], n[3:9])
        _views_equal(one.view(), ref.view())
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            one.add(_t(np.zeros((1, Kp + 1, 32), np.uint8)), _t(n[:1]))
    finally:
        one.close(); three.close()


def _query_same(idx, ref, qd, qn, top_k, below=None):
    o = idx.query(_t(qd), _t(qn), top_k, None if below is None else _t(np.asarray(below, np.int32)))
    idx.ctx.synchronize()
    ids, sc, dn, qnorm = ref.query(qd, qn, top_k, below)
    assert np.array_equal(_h(o["best_id"]), ids), (top_k, below)
    assert np.array_equal(_h(o["best_score"]), sc) and np.array_equal(_h(o["best_den"]), dn) and np.array_equal(_h(o["q_norm"]), qnorm)
    return ids, sc, dn


@pytest.fixture(scope="module")
def big():
    """300 entries of up to 48 descriptors over 65 words, entries 150 and 151 alike; the reference index with all its sizes' answers"""
    W, Kp, E = 65, 48, 300
    vocab = pc.awkward_vocab(21, W)
    desc, n = pc.frames_for(22, vocab, E, Kp, [Kp, 0, 1, 47, 24, 30])
    desc[151], n[151] = desc[150], n[150]
    return W, Kp, vocab, desc, n


@pytest.mark.parametrize("entries", [0, 1, 63, 65, 300])
def test_query(ctx, big, entries):
    W, Kp, vocab, desc, n = big
    idx, ref = _pair(ctx, W, 300, Kp, vocab)
    try:
        if entries:
            idx.add(_t(desc[:entries]), _t(n[:entries]))
            ref.add(desc[:entries], n[:entries])
        rng = np.random.default_rng(entries)
        pick = np.concatenate([[min(150, max(entries - 1, 0))], rng.integers(0, 300, 8)])
        qd, qn = desc[pick].copy(), np.maximum(n[pick] - 1, 0).astype(np.int32)
        weights = {"ones": None, "idf": rp.places_weights(ref.df, max(ref.size, 1)), "zero": np.zeros(W, np.int32)}
        for name, w in weights.items():
            idx.set_weights(None if w is None else _t(w))
            ref.set_weights(w)
            for Q in (1, 9):
                for top_k in (1, 3, 16):
                    ids, _, _ = _query_same(idx, ref, qd[:Q], qn[:Q], top_k)
                    if name == "zero":
                        assert (ids == -1).all()
            for below in ([0] * 9, [entries // 2] * 9, [entries + 5] * 9, list(rng.integers(-2, entries + 3, 9))):
                _query_same(idx, ref, qd, qn, 3, below)
            _views_equal(idx.view(), ref.view())
        if entries == 300:
            idx.set_weights(None)
            ref.set_weights(None)
            ids, sc, dn = _query_same(idx, ref, qd[:1], qn[:1], 16)
            k = ids[0].tolist().index(150)
            assert ids[0, k + 1] == 151 and sc[0, k] == sc[0, k + 1] and dn[0, k] == dn[0, k + 1], "equal scores: the lower id first"
            same = np.repeat(qd[1:2], 9, 0), np.repeat(qn[1:2], 9)
            ids, _, _ = _query_same(idx, ref, *same, 16)
            assert (ids == ids[0]).all(), "the same query in every batch slot"
    finally:
        idx.close()


def test_query_at_the_product_bound(ctx):
    """weights of 65535 and frames of 16384 descriptors of one word: score = den = 65535 x 16384, the largest there is"""
    Kp = 16384
    vocab = np.stack([np.zeros(32, np.uint8), np.full(32, 255, np.uint8)])
    desc = np.zeros((3, Kp, 32), np.uint8)
    desc[1, : Kp // 2] = 255
    n = np.array([Kp, Kp, Kp], np.int32)
    w = np.array([65535, 70000], np.int32)
    idx, ref = _pair(ctx, 2, 4, Kp, vocab, w)
    try:
        idx.add(_t(desc), _t(n))
        ref.add(desc, n)
        ids, sc, dn = _query_same(idx, ref, desc[:2], n[:2], 4)
        assert ids[0].tolist() == [0, 2, 1, -1] and sc[0, 0] == dn[0, 0] == 65535 * 16384
        _views_equal(idx.view(), ref.view())
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_the_fixture_through_the_device_extractor(ctx):
    """seed 11's frames through the DEVICE extractor, trained on the device, indexed and queried there: equal to the reference on the
    same descriptors, every query's best candidate its own pair's "last" frame"""
    ca, sa = synth.keypoint_rotation()
    pat = _t(synth.brief_pattern())

    def extract(seed, pairs):
        o = ctx.extract_features(_t(pc.fixture_frames(seed, pairs)), pc.FIX_CORNERS, ca, sa, pat, kp_stride=pc.FIX_CORNERS)
        return o["desc"], o["n"]
    td, tn = extract(pc.FIX_TRAIN_SEED, pc.FIX_TRAIN_PAIRS)
    ctx.synchronize()
    rows = torch.cat([td[f, :int(tn[f])] for f in range(td.shape[0])]).contiguous()
    tr = ctx.places_train(rows, pc.FIX_WORDS, pc.FIX_ITERS)
    desc, n = extract(11, pc.FIX_PAIRS)
    P = pc.FIX_PAIRS
    idx = capi.Places(ctx, pc.FIX_WORDS, P, pc.FIX_CORNERS)
    try:
        idx.set_vocabulary(tr["vocab"])
        idx.add(desc[:P].contiguous(), n[:P].contiguous())
        df = idx.view()["df"]
        idx.set_weights(_t(capi.places_weights(df, P)))
        o = idx.query(desc[P:].contiguous(), n[P:].contiguous(), 2)
        ctx.synchronize()
        vocab, sizes = rp.train(_h(rows), pc.FIX_WORDS, pc.FIX_ITERS)
        assert np.array_equal(_h(tr["vocab"]), vocab) and np.array_equal(_h(tr["sizes"]), sizes)
        ref, (ids, sc, dn, qn) = pc.reference_retrieval(vocab, _h(desc), _h(n), P)
        assert np.array_equal(df, ref.df)
        assert np.array_equal(_h(o["best_id"]), ids) and np.array_equal(_h(o["best_score"]), sc) and np.array_equal(_h(o["best_den"]), dn)
        assert np.array_equal(_h(o["q_norm"]), qn)
        _views_equal(idx.view(), ref.view())
        top, margin = pc.retrieval(ids, sc, dn)
        print(f"device fixture: top-1 right for {(top == np.arange(P)).sum()} of {P}, smallest margin {margin.min():.4f}")
        assert top.tolist() == list(range(P))
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def small(ctx):
    W, Kp, E = 33, 40, 12
    vocab = pc.awkward_vocab(31, W)
    desc, n = pc.frames_for(32, vocab, E, Kp, [Kp, 0, 7, 39])
    return W, Kp, E, vocab, desc, n


def _refused(ctx, call, want, note):
    rc, msg, got, _ = ec.run(ctx, call)
    assert rc == want, (note, rc, msg)
    for k, v in got.items():
        if not k.startswith("state:"):
            assert (v == 0xA5).all(), (note, k, "written by a refused call")
    return got


def test_refusals_leave_outputs_untouched_and_the_next_call_exact(ctx, small):
    W, Kp, E, vocab, desc, n = small
    d, nn, v = _t(desc), _t(n), _t(vocab)
    good = plc.assign(d, nn, v)
    rc, msg, first, _ = ec.run(ctx, good)
    assert rc == 0, msg

    def argv(call, **kw):
        names = ["d_desc", "d_n", "kp_stride", "frames", "d_vocab", "n_words", "d_word", "d_dist"]
        a = list(call.argv)
        for k, val in kw.items():
            a[names.index(k)] = val
        return call.replaced(argv=a)
    for note, call, want in (("frames 0", argv(good, frames=0), INVALID), ("kp_stride 0", argv(good, kp_stride=0), INVALID),
                             ("n_words 0", argv(good, n_words=0), INVALID), ("n_words above the maximum", argv(good, n_words=16385), INVALID),
                             ("kp_stride above VSLAM_MAX_KP", argv(good, kp_stride=16385), CAPACITY), ("null d_desc", argv(good, d_desc=None), INVALID),
                             ("null d_n", argv(good, d_n=None), INVALID), ("null d_vocab", argv(good, d_vocab=None), INVALID),
                             ("null d_word", argv(good, d_word=None), INVALID),
                             ("2^31 workgroups: 2^25 frames of 64 each", argv(good, frames=1 << 25, kp_stride=16384), CAPACITY),
                             ("2^31 workgroups and a kp_stride that is refused too", argv(good, frames=1 << 25, kp_stride=16385), CAPACITY)):
        _refused(ctx, call, want, note)
    rc, msg, again, _ = ec.run(ctx, good)
    assert rc == 0 and not ec._same(first, again)

    tr = plc.train(_t(desc.reshape(-1, 32)), W, 2)
    rc, msg, tfirst, _ = ec.run(ctx, tr)
    assert rc == 0, msg
    for note, a, want in (("n below n_words", [tr.argv[0], W - 1, W, 2] + tr.argv[4:], INVALID), ("n_words 0", [tr.argv[0], 480, 0, 2] + tr.argv[4:], INVALID),
                          ("iterations 65", tr.argv[:3] + [65] + tr.argv[4:], INVALID), ("iterations -1", tr.argv[:3] + [-1] + tr.argv[4:], INVALID),
                          ("null d_sizes", tr.argv[:5] + [None], INVALID), ("null d_desc", [None] + tr.argv[1:], INVALID),
                          ("null d_vocab", tr.argv[:4] + [None, tr.argv[5]], INVALID),
                          ("n_words above the maximum", [tr.argv[0], 1 << 15, 16385, 2] + tr.argv[4:], INVALID),
                          ("n above VSLAM_PLACES_MAX_TRAIN", [tr.argv[0], (1 << 24) + 1, W, 2] + tr.argv[4:], CAPACITY),
                          ("d_vocab is d_desc", tr.argv[:4] + [ec.P("d_desc"), tr.argv[5]], INVALID)):
        _refused(ctx, tr.replaced(argv=a), want, note)
    rc, msg, again, _ = ec.run(ctx, tr)
    assert rc == 0 and not ec._same(tfirst, again)
    # d_vocab against d_desc inside one buffer: [vocab W rows][desc nd rows][vocab W rows]; touching is taken, one row of overlap is not
    flat = desc.reshape(-1, 32)
    nd = len(flat)
    buf = torch.zeros((2 * W + nd) * 32, dtype=torch.uint8, device="cuda")
    buf[W * 32:(W + nd) * 32] = _t(flat).reshape(-1)
    sizes = torch.zeros(W, dtype=torch.int32, device="cuda")
    at = lambda row: C.c_void_p(buf.data_ptr() + 32 * row)   # noqa: E731
    want_v, want_s = rp.train(flat, W, 2)
    for row, want in ((1, INVALID), (W, INVALID), (W + nd - 1, INVALID), (nd, INVALID), (0, 0), (W + nd, 0)):
        torch.cuda.synchronize()
        before = buf.clone()
        assert ctx.lib.vslam_places_train(ctx.handle, at(W), nd, W, 2, at(row), C.c_void_p(sizes.data_ptr())) == want, row
        ctx.synchronize()
        if want:
            assert torch.equal(buf, before), (row, "written by a refused call")
        else:
            assert np.array_equal(_h(buf[32 * row:32 * (row + W)]).reshape(W, 32), want_v) and np.array_equal(_h(sizes), want_s), row
            assert torch.equal(buf[W * 32:(W + nd) * 32], before[W * 32:(W + nd) * 32])

    h = C.c_void_p()
    for args, want in (((0, 4, 4), INVALID), ((16385, 4, 4), INVALID), ((4, 0, 4), INVALID), ((4, 4, 0), INVALID), ((4, 4, 16385), CAPACITY),
                       ((4, (1 << 20) + 1, 4), CAPACITY), ((16384, 1 << 17, 16384), CAPACITY), ((1 << 11, 1 << 20, 16384), CAPACITY),
                       ((16384, 1 << 20, 1 << 11), CAPACITY)):
        assert ctx.lib.vslam_places_create(ctx.handle, *args, C.byref(h)) == want and not h.value, args
    assert ctx.lib.vslam_places_create(ctx.handle, 4, 4, 4, None) == INVALID
    idx = capi.Places(ctx, W, E, Kp)
    try:
        q = plc.query(idx, d[:3].contiguous(), nn[:3].contiguous(), 2)
        _refused(ctx, q, INVALID, "a query without a vocabulary")
        _refused(ctx, plc.add(idx, d, nn), INVALID, "an add without a vocabulary")
        idx.set_vocabulary(v)
        idx.add(d[:6].contiguous(), nn[:6].contiguous())
        filled = lambda: None   # noqa: E731  (the index stays as it is in front of every call)
        rc, msg, qfirst, _ = ec.run(ctx, q)
        assert rc == 0, msg
        for note, call, want in (("top_k 0", q.replaced(argv=q.argv[:6] + [0] + q.argv[7:]), INVALID),
                                 ("top_k 17", q.replaced(argv=q.argv[:6] + [17] + q.argv[7:]), INVALID),
                                 ("queries 0", q.replaced(argv=q.argv[:4] + [0] + q.argv[5:]), INVALID),
                                 ("kp_stride above max_kp", q.replaced(argv=q.argv[:3] + [Kp + 1] + q.argv[4:]), CAPACITY),
                                 ("null d_q_norm", q.replaced(argv=q.argv[:10] + [None]), INVALID),
                                 ("null d_best_den", q.replaced(argv=q.argv[:9] + [None] + q.argv[10:]), INVALID),
                                 ("more frames than the index has room for", plc.add(idx, d[:7].contiguous(), nn[:7].contiguous(), before=filled), CAPACITY),
                                 ("null d_ids", plc.add(idx, d[:2].contiguous(), nn[:2].contiguous(), before=filled).replaced(
                                     argv=[idx.handle, ec.P("d_desc"), ec.P("d_n"), Kp, 2, None, None]), INVALID),
                                 ("a vocabulary for an index that is not empty", plc.set_vocabulary(idx, v).replaced(before=filled), INVALID),
                                 ("queries 65536", q.replaced(argv=q.argv[:4] + [65536] + q.argv[5:]), CAPACITY),
                                 ("queries 2^25: 2^31 workgroups", q.replaced(argv=q.argv[:3] + [16384, 1 << 25] + q.argv[5:]), CAPACITY),
                                 ("queries -1", q.replaced(argv=q.argv[:4] + [-1] + q.argv[5:]), INVALID),
                                 ("query kp_stride 0", q.replaced(argv=q.argv[:3] + [0] + q.argv[4:]), INVALID),
                                 ("query null d_desc", q.replaced(argv=[q.argv[0], None] + q.argv[2:]), INVALID),
                                 ("query null d_n", q.replaced(argv=q.argv[:2] + [None] + q.argv[3:]), INVALID),
                                 ("query null d_best_id", q.replaced(argv=q.argv[:7] + [None] + q.argv[8:]), INVALID),
                                 ("query null d_best_score", q.replaced(argv=q.argv[:8] + [None] + q.argv[9:]), INVALID),
                                 *((note, ad.replaced(argv=a), want) for ad in [plc.add(idx, d[:2].contiguous(), nn[:2].contiguous(), before=filled)]
                                   for note, a, want in (("add frames 0", ad.argv[:4] + [0] + ad.argv[5:], INVALID),
                                                         ("add kp_stride 0", ad.argv[:3] + [0] + ad.argv[4:], INVALID),
                                                         ("add kp_stride above max_kp", ad.argv[:3] + [Kp + 1] + ad.argv[4:], CAPACITY),
                                                         ("add null d_desc", [ad.argv[0], None] + ad.argv[2:], INVALID),
                                                         ("add null d_n", ad.argv[:2] + [None] + ad.argv[3:], INVALID),
                                                         ("add 2^25 frames: 2^31 workgroups", ad.argv[:3] + [16384, 1 << 25] + ad.argv[5:], CAPACITY))),
                                 ("a null vocabulary", plc.set_vocabulary(idx, v).replaced(before=filled, argv=[idx.handle, None, None]), INVALID)):
            got = _refused(ctx, call, want, note)
            assert not ec._same({k: x for k, x in got.items() if k.startswith("state:")}, {k: x for k, x in qfirst.items() if k.startswith("state:")}), note
        rc, msg, again, _ = ec.run(ctx, q)
        assert rc == 0 and not ec._same(qfirst, again)
        empty = capi.Places(ctx, W, E, Kp)      # a null vocabulary is refused on an empty index too, which stays without one
        try:
            assert ctx.lib.vslam_places_set_vocabulary(ctx.handle, empty.handle, None, None) == INVALID
            _refused(ctx, plc.query(empty, d[:3].contiguous(), nn[:3].contiguous(), 2), INVALID, "still without a vocabulary")
        finally:
            empty.close()
    finally:
        idx.close()


def test_pointers_at_the_stated_alignment_and_one_step_below(ctx, small):
    W, Kp, E, vocab, desc, n = small
    lib, hnd = ctx.lib, ctx.handle
    room = lambda a: torch.cat([_t(a).view(torch.uint8).reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])  # noqa: E731
    word, dist = rp.assign(desc, n, vocab)
    out = torch.zeros(E * Kp * 4 + 64, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros(E * Kp * 4 + 64, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(W * 4 + 64, dtype=torch.uint8, device="cuda")
    vout = torch.zeros(W * 32 + 64, dtype=torch.uint8, device="cuda")
    idx = capi.Places(ctx, W, E, Kp)
    try:
        def shifted(t, a, k):
            """the tensor's bytes moved k bytes up inside its buffer -> the address"""
            t[k:k + a.nbytes] = _t(a).view(torch.uint8).reshape(-1)
            return t.data_ptr() + k
        D, N, V = room(desc), room(n), room(vocab)
        wts = room(np.arange(W, dtype=np.int32))

        def assign_rc(kd=0, kn=0, kv=0, kw=0, kx=0):
            torch.cuda.synchronize()
            return lib.vslam_places_assign(hnd, C.c_void_p(shifted(D, desc, kd)), C.c_void_p(shifted(N, n, kn)), Kp, E, C.c_void_p(shifted(V, vocab, kv)),
                                           W, C.c_void_p(out.data_ptr() + kw), C.c_void_p(out2.data_ptr() + kx))
        assert assign_rc(16, 4, 16, 4, 4) == 0
        ctx.synchronize()
        assert np.array_equal(_h(out[4:4 + E * Kp * 4]).view(np.int32).reshape(E, Kp), word)
        assert np.array_equal(_h(out2[4:4 + E * Kp * 4]).view(np.int32).reshape(E, Kp), dist)
        for kw in (dict(kd=8), dict(kn=2), dict(kv=8), dict(kw=2), dict(kx=2)):
            assert assign_rc(**kw) == INVALID, kw
        flat = desc.reshape(-1, 32)

        def train_rc(kd=0, kv=0, ks=0):
            torch.cuda.synchronize()
            return lib.vslam_places_train(hnd, C.c_void_p(shifted(D, flat, kd)), len(flat), W, 1, C.c_void_p(vout.data_ptr() + kv), C.c_void_p(sizes.data_ptr() + ks))
        assert train_rc(16, 16, 4) == 0
        ctx.synchronize()
        tv, ts = rp.train(flat, W, 1)
        assert np.array_equal(_h(vout[16:16 + W * 32]).reshape(W, 32), tv) and np.array_equal(_h(sizes[4:4 + W * 4]).view(np.int32), ts)
        for kw in (dict(kd=8), dict(kv=8), dict(ks=2)):
            assert train_rc(**kw) == INVALID, kw
        P = lambda t, a, k: C.c_void_p(shifted(t, a, k))   # noqa: E731
        torch.cuda.synchronize()
        assert lib.vslam_places_set_vocabulary(hnd, idx.handle, P(V, vocab, 8), None) == INVALID
        assert lib.vslam_places_set_vocabulary(hnd, idx.handle, P(V, vocab, 16), P(wts, np.arange(W, dtype=np.int32), 2)) == INVALID
        assert lib.vslam_places_set_vocabulary(hnd, idx.handle, P(V, vocab, 16), P(wts, np.arange(W, dtype=np.int32), 4)) == 0
        assert lib.vslam_places_set_weights(hnd, idx.handle, P(wts, np.arange(W, dtype=np.int32), 2)) == INVALID
        ids = torch.zeros(E * 4 + 64, dtype=torch.uint8, device="cuda")
        tags = room(np.zeros((E, 2), np.int32))
        for kd, kn, kt, ki, want in ((8, 4, 4, 4, INVALID), (16, 2, 4, 4, INVALID), (16, 4, 2, 4, INVALID), (16, 4, 4, 2, INVALID), (16, 4, 4, 4, 0)):
            torch.cuda.synchronize()
            assert lib.vslam_places_add(hnd, idx.handle, P(D, desc, kd), P(N, n, kn), Kp, E, C.c_void_p(tags.data_ptr() + kt),
                                        C.c_void_p(ids.data_ptr() + ki)) == want, (kd, kn, kt, ki)
        ref = rp.Index(W, E, Kp)
        ref.set_vocabulary(vocab, np.arange(W, dtype=np.int32))
        ref.add(desc, n)
        _views_equal(idx.view(), ref.view())
        res = [torch.zeros(E * 16 * 4 + 64, dtype=torch.uint8, device="cuda") for _ in range(4)]
        below = room(np.full(E, E, np.int32))
        for ks, want in (((8, 4, 4, 4, 4, 4, 4), INVALID), ((16, 2, 4, 4, 4, 4, 4), INVALID), ((16, 4, 2, 4, 4, 4, 4), INVALID), ((16, 4, 4, 2, 4, 4, 4), INVALID),
                         ((16, 4, 4, 4, 2, 4, 4), INVALID), ((16, 4, 4, 4, 4, 2, 4), INVALID), ((16, 4, 4, 4, 4, 4, 2), INVALID), ((16, 4, 4, 4, 4, 4, 4), 0)):
            torch.cuda.synchronize()
            rc = lib.vslam_places_query(hnd, idx.handle, P(D, desc, ks[0]), P(N, n, ks[1]), Kp, E, P(below, np.full(E, E, np.int32), ks[2]), 16,
                                        *(C.c_void_p(r.data_ptr() + k) for r, k in zip(res, ks[3:])))
            assert rc == want, ks
        ctx.synchronize()
        ids_r, sc, dn, qn = ref.query(desc, n, 16)
        assert np.array_equal(_h(res[0][4:4 + E * 64]).view(np.int32).reshape(E, 16), ids_r)
        assert np.array_equal(_h(res[1][4:4 + E * 64]).view(np.int32).reshape(E, 16), sc)
        assert np.array_equal(_h(res[3][4:4 + E * 4]).view(np.int32), qn)
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------------------- workspace, stream order
def _calls(ctx, small, variant):
    """the Calls of every new entry point that queues work, at one of two shapes with different contents"""
    W, Kp, E, vocab, desc, n = small
    if variant:
        rng = np.random.default_rng(77)
        vocab = pc.awkward_vocab(55, W)
        desc, n = pc.frames_for(56, vocab, E, Kp, [39, 3, Kp, 0])
        desc = desc[rng.permutation(E)]
    d, nn, v = _t(desc), _t(n), _t(vocab)
    idx = capi.Places(ctx, W, E, Kp)
    idx.set_vocabulary(_t(small[3]))
    half = E // 2
    wts = _t(np.random.default_rng(5 + variant).integers(0, 70000, W).astype(np.int32))
    tags = _t(np.random.default_rng(6 + variant).integers(0, 99, (half, 2)).astype(np.int32))

    def filled():
        idx.reset()
        idx.add(_t(small[4][:half]), _t(small[5][:half]))
    filled()
    zeros = torch.zeros(W, dtype=torch.int32, device="cuda")

    def stale_norms():
        """filled, the norms in the index's memory those of all-zero weights, the weights then `wts`: the view has to form them"""
        filled()
        idx.set_weights(zeros)
        idx.arrays()
        idx.set_weights(wts)
    below = _t(np.random.default_rng(8 + variant).integers(0, half + 2, E).astype(np.int32))
    calls = {
        "vslam_places_assign": plc.assign(d, nn, v),
        "vslam_places_train": plc.train(d.reshape(-1, 32), W, 2),
        "vslam_places_set_vocabulary": plc.set_vocabulary(idx, v, wts),
        "vslam_places_set_weights": plc.set_weights(idx, wts).replaced(before=filled),
        "vslam_places_add": plc.add(idx, d[:half].contiguous(), nn[:half].contiguous(), tags, before=filled),
        "vslam_places_query": plc.query(idx, d, nn, 3, below).replaced(before=filled),
        "vslam_places_reset": plc.reset(idx, filled),
        "vslam_places_view": plc.view(idx, stale_norms),
    }
    return idx, calls


def test_every_entry_point_behind_a_filled_workspace_and_another_shape(ctx, small):
    idx, calls = _calls(ctx, small, 0)
    W, Kp, E, vocab, desc, n = small
    other_vocab = pc.awkward_vocab(90, 257)
    od, on = pc.frames_for(91, other_vocab, 3, 300, [300, 17, 256])
    oidx = capi.Places(ctx, 257, 8, 300)
    try:
        assert sorted(calls) == sorted(plc.ENTRIES)
        first = {}
        for name, call in calls.items():
            rc, msg, first[name], _ = ec.run(ctx, call)
            assert rc == 0, (name, msg)
        assert first["vslam_places_view"]["state:norms"].any() and not first["vslam_places_reset"]["state:df"].any()
        assert first["vslam_places_reset"]["state:offsets"].size == 4 and first["vslam_places_query"]["state:offsets"].size > 4
        slots = ctx.workspace_slots()
        assert {"places.spread", "places.train", "places.word", "places.entry", "places.score"} <= set(slots)
        for fill in (0x00, 0x5A):
            for name, call in calls.items():
                ctx.workspace_fill(fill)
                rc, msg, got, _ = ec.run(ctx, call)
                assert rc == 0 and not ec._same(first[name], got), (name, fill, ec._same(first[name], got))
        # behind a call of itself at another shape
        oidx.set_vocabulary(_t(other_vocab))
        for name, call in calls.items():
            ctx.places_assign(_t(od), _t(on), _t(other_vocab))
            ctx.places_train(_t(od.reshape(-1, 32)), 257, 1)
            oidx.reset()
            oidx.add(_t(od), _t(on))
            oidx.query(_t(od), _t(on), 16)
            rc, msg, got, _ = ec.run(ctx, call)
            assert rc == 0 and not ec._same(first[name], got), (name, ec._same(first[name], got))
    finally:
        idx.close(); oidx.close()


@pytest.mark.parametrize("entry", plc.ENTRIES)
def test_stream_order_behind_a_stalled_stream(small, entry):
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = capi.Context(0)
        idx = other_idx = None
        try:
            idx, calls = _calls(ctx, small, 0)
            other_idx, others = _calls(ctx, small, 1)
            call, other = calls[entry], others[entry]
            decoys = Decoys(call, other, None)
            sizing = choose_sizing(ctx, [call], stream)
            res = run_behind_stall(ctx, call, stream, decoys, sizing)
            assert res.rc == 0, res.msg
            assert res.pending_at_return, f"{entry} waited for the device before it returned"
            assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
            assert set(res.got) == set(res.expected)
            for k in res.expected:
                assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"
        finally:
            for x in (idx, other_idx):
                if x is not None:
                    x.close()
            ctx.close()


# ---------------------------------------------------------------------------------------------------------------- C++ surfaces
def test_cpp_surfaces_match_the_reference(small, tmp_path):
    """tests/native/places_demo.cpp: vslam::places_assign, vslam::places_train and vslam::Places (include/vslam/helpers.h) give the
    reference's bits, and Places::set_vocabulary throws on an index that is not empty."""
    import struct
    import subprocess
    from vslam_amd import build
    if not os.path.exists(build.HOST_LIB):   # build() has made it; nothing is compiled again here but the demo itself
        build.build_host()
    exe = str(tmp_path / "places_demo")
    subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe, os.path.join(ROOT, "tests", "native", "places_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    W, Kp, E, vocab, desc, n = small
    below = np.arange(E, dtype=np.int32) + 1          # every frame may find itself and its elders
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("5i", W, Kp, E, 2, 3))
        for a in (vocab, desc, n, below):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    word, dist = rp.assign(desc, n, vocab)
    trained, sizes = rp.train(desc.reshape(-1, 32), W, 2)
    ref = rp.Index(W, E, Kp)
    ref.set_vocabulary(trained)
    ids = ref.add(desc, n)
    bid, sc, dn, qn = ref.query(desc, n, 3, below)
    want = b"".join(np.ascontiguousarray(a).tobytes() for a in (word, dist, trained, sizes, ids, bid, sc, dn, qn))
    assert open(fout, "rb").read() == want
    assert (bid[:, 0] >= 0).sum() >= E // 2
