"""HIP match kernel vs the oracle (bit-exact: indices, distances, pair lists), and vs the integer definitions of tests/ref_int.py
(written from src/Frame.cpp:83-94, not from the oracle)."""
import numpy as np
import pytest
import torch

import ref_int

from vslam_amd import synth

pytestmark = pytest.mark.gpu


def _pack(items, K):
    B = len(items)
    d = np.zeros((B, K, 32), dtype=np.uint8)
    n = np.zeros(B, dtype=np.int32)
    for b, a in enumerate(items):
        d[b, :len(a)] = a
        n[b] = len(a)
    return torch.from_numpy(d).cuda(), torch.from_numpy(n).cuda()


@pytest.fixture(params=[(0, 0), (1, 1), (2, 1), (1, 2), (2, 2)], ids=["product", "exp-fp4-8x32", "exp-fp4-4x64", "exp-i8-8x32", "exp-i8-4x64"])
def mctx(request):
    """The product library's one matcher (FP4 +-1 products, 8 waves x 32 rows), and -- through the EXPERIMENTS build, the only
    one that carries them -- both workgroup shapes (VSLAM_OPT_MATCH_SHAPE) of both matrix-core forms (VSLAM_OPT_MATCH_FORM:
    FP4, int8 0 / 1 products).  Yields the context to use."""
    if request.param == (0, 0):
        yield request.getfixturevalue("ctx")
        return
    c = request.getfixturevalue("ctx_exp")
    c.set_option(c.OPT_MATCH_SHAPE, request.param[0])
    c.set_option(c.OPT_MATCH_FORM, request.param[1])
    yield c
    c.set_option(c.OPT_MATCH_SHAPE, 0)
    c.set_option(c.OPT_MATCH_FORM, 0)


def test_product_library_carries_one_matcher(ctx):
    """The matcher's variants are settable in the experiments build only."""
    from vslam_amd import VslamError
    for opt, val in ((ctx.OPT_MATCH_SHAPE, 1), (ctx.OPT_MATCH_SHAPE, 2), (ctx.OPT_MATCH_FORM, 2)):
        with pytest.raises(VslamError):
            ctx.set_option(opt, val)
    ctx.set_option(ctx.OPT_MATCH_FORM, 1)   # FP4 is the product's form
    ctx.set_option(ctx.OPT_MATCH_FORM, 0)


def test_knn2_and_ratio_bit_exact_ragged_batch(mctx, oracle):
    ctx = mctx
    K = 700
    sizes = [(500, 500), (700, 650), (1, 2), (513, 257), (256, 512), (0, 10), (10, 1), (10, 0), (3, 2)]
    items = [synth.descriptors_pair(100 + i, a, b) for i, (a, b) in enumerate(sizes)]
    for it in items[:2]:
        if len(it[1]) > 50:
            it[1][7] = it[1][33]      # equal train rows -> distance ties, lower index must win
    d1, n1 = _pack([it[0] for it in items], K)
    d2, n2 = _pack([it[1] for it in items], K)
    pairs, m, knn = ctx.match_knn2_ratio(d1, n1, d2, n2, want_knn=True)
    ctx.synchronize()
    pairs, m, knn = pairs.cpu().numpy(), m.cpu().numpy(), knn.cpu().numpy()
    for b, (a, t, _) in enumerate(items):
        if len(t) >= 2:
            i0, e0, i1, e1 = oracle.match_knn2(a, t)
            g = knn[b, :len(a)]
            assert np.array_equal(g[:, 0], i0) and np.array_equal(g[:, 1], e0), b
            assert np.array_equal(g[:, 2], i1) and np.array_equal(g[:, 3], e1), b
            ref, rc = oracle.match_knn2_ratio(a, t)
            assert rc == 0
            assert m[b] == len(ref), b
            assert np.array_equal(pairs[b, :m[b]], ref), b
        else:
            assert m[b] == 0      # reference reads m[1] of a 1-row result: undefined; we emit nothing
        ref_int.hold_match(a, t, knn=knn[b, :len(a)] if len(t) >= 2 else None, pairs=pairs[b, :m[b]])


def test_full_size_property_self_match(mctx):
    ctx = mctx
    """At the headline size (K = 2000, B = 8 of the 256) every row's best match against a
    shuffled copy of itself is its own image at distance 0, and a copy is its own 2nd-NN-ratio
    survivor: checks index packing over the whole range without the oracle."""
    B, K = 8, 2000
    g = torch.Generator().manual_seed(1)
    d1 = torch.randint(0, 256, (B, K, 32), dtype=torch.uint8, generator=g)
    perm = torch.stack([torch.randperm(K, generator=g) for _ in range(B)])
    d2 = torch.stack([d1[b][perm[b]] for b in range(B)])
    n = torch.full((B,), K, dtype=torch.int32)
    pairs, m, knn = ctx.match_knn2_ratio(d1.cuda(), n.cuda(), d2.cuda(), n.cuda(), want_knn=True)
    ctx.synchronize()
    knn, m, pairs = knn.cpu(), m.cpu(), pairs.cpu()
    inv = torch.argsort(perm, dim=1).to(torch.int32)
    assert torch.equal(knn[:, :, 0], inv) and int(knn[:, :, 1].abs().sum()) == 0
    assert torch.all(m == K)
    assert torch.equal(pairs[:, :, 1], inv)
    for b in range(B):            # and through the definition (about a second of CPU time per item)
        ref_int.hold_match(d1[b].numpy(), d2[b].numpy(), knn=knn[b].numpy(), pairs=pairs[b, :int(m[b])].numpy())


def test_extreme_distances_and_index_range(mctx, oracle):
    ctx = mctx
    """Distances 0, 1, 255 and 256 (the +-1 products of the FP4 form then sum to +-256, where the key arithmetic changes
    sign), all-zero and all-one descriptors, and train indices up to the largest a key can carry at this stride."""
    rng = np.random.default_rng(77)
    K = 2100
    q = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    q[0] = 0; q[1] = 255; q[2] = 0; q[3] = 255
    t = rng.integers(0, 256, (K, 32), dtype=np.uint8)
    t[5] = ~q[10]                         # distance 256 from query 10
    t[K - 1] = q[11]                      # distance 0 at the last index
    t[K - 2] = q[11]; t[K - 2, 0] ^= 1    # distance 1 right before it
    t[100] = 255; t[101] = 0              # |b| = 256 and 0
    far = np.stack([~q[12]] * 40)         # a query whose two best are both far: every train row at distance >= 250
    far[:, 0] ^= np.arange(40, dtype=np.uint8) % 7
    d1, n1 = _pack([q, q[12:13]], K)
    d2, n2 = _pack([t, far], K)
    pairs, m, knn = ctx.match_knn2_ratio(d1, n1, d2, n2, want_knn=True)
    ctx.synchronize()
    knn, m, pairs = knn.cpu().numpy(), m.cpu().numpy(), pairs.cpu().numpy()
    for b, (a, tr) in enumerate(((q, t), (q[12:13], far))):
        i0, e0, i1, e1 = oracle.match_knn2(a, tr)
        g = knn[b, :len(a)]
        assert np.array_equal(g[:, 0], i0) and np.array_equal(g[:, 1], e0), b
        assert np.array_equal(g[:, 2], i1) and np.array_equal(g[:, 3], e1), b
        ref, _ = oracle.match_knn2_ratio(a, tr)
        assert m[b] == len(ref) and np.array_equal(pairs[b, :m[b]], ref), b
        ref_int.hold_match(a, tr, knn=knn[b, :len(a)], pairs=pairs[b, :m[b]])
    assert knn[0, 11, 0] == K - 1 and knn[0, 11, 1] == 0 and knn[0, 11, 2] == K - 2 and knn[0, 11, 3] == 1
    assert knn[1, 0, 1] >= 250


# ------------------------------------------------------------------------------------------ train indices up to 16383
MAX_KP = 16384          # VSLAM_MAX_KP, include/vslam_amd.h: the FP4 matcher's key is dot * 16384 - train index
N_CHOSEN = 512          # rows of item 0 held to ref_int against all 16384 train rows


def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


@pytest.fixture(scope="module")
def top_of_range():
    """Five items of stride 16384 and their references (ref_int, computed once for the five matchers; never written to).
    Train rows 4095/4096, 8191/8192, 16382/16383 and 0/16383 cannot carry an exact / one-bit-off pair AND one row repeated in
    the same train set, so the repeated rows get two small items of their own (64 queries, 16384 train rows) beside the three
    the sizes call for:
      0  nq = nt = 16384; copies around the carries of the index field, extreme distances, and a third of the other queries
         given a noisy copy somewhere in the train set so that the ratio test's survivors are spread over all 16384 rows
      1  nq = 300, nt = 16353 = 511 tiles of 32 and one row      2  nq = 300, nt = 16321: 511 tiles, an odd count
      3  one row repeated at (4095, 4096), (8191, 8192), (16382, 16383)      4  one row repeated at (0, 16383)"""
    rng = np.random.default_rng(2024)
    rnd = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    q0, t0 = rnd(MAX_KP), rnd(MAX_KP)
    fixed = [0, 255, 256, 4095, 4096, 8191, 8192, 16383]
    rest = rng.permutation(np.setdiff1d(np.arange(MAX_KP), fixed))
    chosen = np.sort(np.concatenate([fixed, rest[:N_CHOSEN - len(fixed)]]))
    planted_rows = [16383, 16382, 4095, 4096, 8191, 8192, 16000, 16001, 16380]
    # noisy copies for a third of the queries that are not chosen: query q -> train row spot[q], 0 .. 40 bits off
    others = rest[N_CHOSEN - len(fixed):]
    copied = others[rng.random(len(others)) < 1 / 3]
    spots = rng.permutation(np.setdiff1d(np.arange(MAX_KP), planted_rows))[:len(copied)]
    for q, s in zip(copied, spots):
        t0[s] = _flip(q0[q], rng.choice(256, rng.integers(0, 41), replace=False))
    q0[0] = 0; q0[256] = 255
    t0[16383] = q0[16383]; t0[16382] = _flip(q0[16383], [0])          # query 16383: exact at the last index, one bit off before
    t0[4095] = q0[4095]; t0[4096] = _flip(q0[4095], [100])            # query 4095: exact below the 2^12 carry, one bit off above
    t0[8192] = q0[4096]; t0[8191] = _flip(q0[4096], [255])            # query 4096: exact above the 2^13 carry, one bit off below
    t0[16000] = 0; t0[16001] = 255                                    # all-zero and all-one rows (queries 0 and 256 are those)
    t0[16380] = ~q0[255]                                              # distance 256 from query 255
    items = [(q0, t0)]
    for nt in (16353, 16321):
        q, t = rnd(300), rnd(nt)
        t[nt - 1] = q[7]; t[nt - 2] = _flip(q[7], [9])
        items.append((q, t))
    q3, t3 = rnd(64), rnd(MAX_KP)
    t3[4095] = t3[4096] = q3[1]
    t3[8191] = t3[8192] = _flip(q3[2], [1, 77, 200])
    t3[16382] = t3[16383] = q3[3]
    q4, t4 = rnd(64), rnd(MAX_KP)
    t4[0] = t4[16383] = _flip(q4[5], [3, 250])
    items += [(q3, t3), (q4, t4)]
    ref = {"chosen": chosen, "knn0": np.stack(ref_int.knn2(q0[chosen], t0), 1)}
    for b in (1, 2, 3, 4):
        ref[b] = (np.stack(ref_int.knn2(*items[b]), 1), ref_int.ratio_pairs(*items[b]))
    for a in [x for it in items for x in it] + [ref["knn0"]]:
        a.setflags(write=False)
    return items, ref


def test_train_indices_up_to_max_kp(mctx, top_of_range):
    """kp_stride = VSLAM_MAX_KP: train indices 4096 .. 16383 in both result slots, the carries of the key's index field at 2^12
    and 2^13, a last tile of one row, an odd tile count, and match_compact_kernel over 16384 rows.  512 of item 0's rows are
    held to ref_int.knn2 against all 16384 train rows (a minute of CPU for all of them); for the whole item pairs[:m] must be
    the in-order compaction of the device's own knn under 10 * d0 < 7 * d1.  Items 1 to 4 are held to ref_int in full."""
    ctx = mctx
    items, ref = top_of_range
    d1, n1 = _pack([it[0] for it in items], MAX_KP)
    d2, n2 = _pack([it[1] for it in items], MAX_KP)
    pairs, m, knn = ctx.match_knn2_ratio(d1, n1, d2, n2, want_knn=True)
    ctx.synchronize()
    pairs, m, knn = pairs.cpu().numpy(), m.cpu().numpy(), knn.cpu().numpy()
    for b in (1, 2, 3, 4):
        nq = len(items[b][0])
        want_knn, want_pairs = ref[b]
        for c, name in enumerate(("best index", "best distance", "second index", "second distance")):
            bad = np.nonzero(knn[b, :nq, c] != want_knn[:, c])[0]
            assert bad.size == 0, (b, name, bad[:5], knn[b, bad[:5]], want_knn[bad[:5]])
        assert m[b] == len(want_pairs) and np.array_equal(pairs[b, :m[b]], want_pairs), (b, m[b], len(want_pairs))
    chosen = ref["chosen"]
    assert len(chosen) == N_CHOSEN >= 500
    bad = np.nonzero((knn[0, chosen] != ref["knn0"]).any(1))[0]
    assert bad.size == 0, (chosen[bad[:5]], knn[0, chosen[bad[:5]]], ref["knn0"][bad[:5]])
    g = knn[0].astype(np.int64)
    assert (g[:, 0] >= 0).all() and (g[:, 0] < MAX_KP).all() and (g[:, 2] >= 0).all() and (g[:, 2] < MAX_KP).all()
    assert (g[:, 0] != g[:, 2]).all() and (g[:, 1] <= g[:, 3]).all() and (g[:, 3] <= 256).all()
    keep = 10 * g[:, 1] < 7 * g[:, 3]
    assert m[0] == keep.sum() and 4000 < m[0] < 7000            # about a third of the rows, all over the range
    assert np.array_equal(pairs[0, :m[0]], np.stack([np.nonzero(keep)[0], g[keep, 0]], 1))
    # the planted facts
    assert knn[0, 16383].tolist() == [16383, 0, 16382, 1]
    assert knn[0, 4095].tolist() == [4095, 0, 4096, 1]
    assert knn[0, 4096].tolist() == [8192, 0, 8191, 1]
    assert knn[0, 0, :2].tolist() == [16000, 0] and knn[0, 256, :2].tolist() == [16001, 0]
    for b, nt in ((1, 16353), (2, 16321)):
        assert knn[b, 7].tolist() == [nt - 1, 0, nt - 2, 1]
    assert knn[3, 1].tolist() == [4095, 0, 4096, 0] and knn[3, 2].tolist() == [8191, 3, 8192, 3]
    assert knn[3, 3].tolist() == [16382, 0, 16383, 0] and knn[4, 5].tolist() == [0, 2, 16383, 2]
    assert not np.isin([1, 2, 3], pairs[3, :m[3], 0]).any() and 5 not in pairs[4, :m[4], 0]    # equal distances: rejected
    for q in (16383, 4095, 4096):
        assert keep[q]
