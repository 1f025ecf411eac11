"""The FP4 matcher's keys (match.hip: dot * 16384 - train index).  The product forms them with one v_fma_f32 per result (key
form 0, the kernel of rounds 4 to 8); the experiments build also carries the three ways of getting them out of the multiply
(VSLAM_MATCH_KEY_FORM: 1 = block scales 2^14 on the descriptor steps, 2 = also the index through a fifth K-step, from index
chunks that match_spread_kernel writes, 3 = the index as the C operand), which were measured and not chosen.  The product and
all four forms are held bit for bit to the numpy knn-2 of tests/ref_int.py:
the knn records and the ratio test's survivors (the in-order compaction of sel).  What the new forms can get wrong: the tile and
trip borders (32 and 64 train rows), fewer than two train rows, the never-written columns of the last tile, the borders of the
index encoding (multiples of 6 inside a chunk half, 127 | 128 between the halves, 8191 | 8192), and the ends of the index range."""
import numpy as np
import pytest

import ref_int
from test_gpu_match import MAX_KP, _flip, _pack
from test_gpu_prune import _env

pytestmark = pytest.mark.gpu

NT = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
NQ = [1, 33, 257]
NONE = 0x7FFFFFFF


@pytest.fixture(params=["product", "form 0", "form 1", "form 2", "form 3"])
def matcher(request):
    """match_knn2_ratio of the product library, or of the experiments build with one key form forced."""
    product = request.param == "product"
    c = request.getfixturevalue("ctx" if product else "ctx_exp")

    def run(*a, **kw):
        with _env(**({} if product else {"VSLAM_MATCH_KEY_FORM": request.param[-1]})):
            out = c.match_knn2_ratio(*a, **kw)
            c.synchronize()
        return out
    return run


def _reference(q, t):
    """knn records (nq, 4) and surviving pairs as the kernel defines them, fewer than two train rows included."""
    if len(t) >= 2:
        return np.stack(ref_int.knn2(q, t), 1), ref_int.ratio_pairs(q, t)
    d = np.unpackbits(q ^ t[0][None], axis=1).sum(1)
    knn = np.stack([np.zeros(len(q), np.int64), d, np.full(len(q), -1), np.full(len(q), NONE)], 1)
    return knn, np.zeros((0, 2), np.int32)


def _run_and_compare(matcher, items, refs, K):
    d1, n1 = _pack([it[0] for it in items], K)
    d2, n2 = _pack([it[1] for it in items], K)
    pairs, m, knn = matcher(d1, n1, d2, n2, want_knn=True)
    pairs, m, knn = pairs.cpu().numpy(), m.cpu().numpy(), knn.cpu().numpy()
    for b, ((q, t), (want_knn, want_pairs)) in enumerate(zip(items, refs)):
        got = knn[b, :len(q)]
        bad = np.nonzero((got != want_knn).any(1))[0]
        assert bad.size == 0, (b, len(q), len(t), bad[:4], got[bad[:4]], want_knn[bad[:4]])
        assert m[b] == len(want_pairs) and np.array_equal(pairs[b, :m[b]], want_pairs), (b, len(q), len(t), m[b], len(want_pairs))
    return knn


@pytest.fixture(scope="module")
def borders():
    rng = np.random.default_rng(909)
    items = []
    for nt in NT:
        for nq in NQ:
            q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
            t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
            # a third of the queries get a near copy somewhere: survivors of the ratio test at every train index
            for i in range(0, nq, 3):
                t[(7 * i + nt - 1) % nt] = _flip(q[i], rng.choice(256, int(rng.integers(0, 30)), replace=False))
            items.append((q, t))
    refs = [_reference(q, t) for q, t in items]
    for a in [x for it in items for x in it]:
        a.setflags(write=False)
    return items, refs


def test_tile_and_trip_borders(matcher, borders):
    """nt in {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257} x nq in {1, 33, 257}, one batch at the odd stride 257."""
    items, refs = borders
    assert len(items) == len(NT) * len(NQ)
    _run_and_compare(matcher, items, refs, 257)


@pytest.fixture(scope="module")
def ties():
    rng = np.random.default_rng(910)
    groups = [([5, 37, 69, 133, 261], 300), ([127, 128, 8191, 8192], 8200)]
    items = []
    for rows, nt in groups:
        q = rng.integers(0, 256, (40, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        t[rows] = q[3]                                   # exact copies: distance 0 at every one of them
        t[[r + 2 for r in rows]] = _flip(q[9], [17, 200])   # and a second family two bits off, two rows further
        items.append((q, t))
    refs = [_reference(q, t) for q, t in items]
    return groups, items, refs


def test_equal_keys_but_for_the_index(matcher, ties):
    """One descriptor at train rows {5, 37, 69, 133, 261} and at {127, 128, 8191, 8192}: the lowest index is the best, the next
    copy the second best, both at distance 0 (and the same two bits off, two rows further)."""
    groups, items, refs = ties
    knn = _run_and_compare(matcher, items, refs, 8200)
    for b, (rows, _) in enumerate(groups):
        assert knn[b, 3].tolist() == [rows[0], 0, rows[1], 0], (b, knn[b, 3])
        assert knn[b, 9].tolist() == [rows[0] + 2, 2, rows[1] + 2, 2], (b, knn[b, 9])


@pytest.fixture(scope="module")
def whole_range():
    rng = np.random.default_rng(911)
    q = rng.integers(0, 256, (32, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (MAX_KP, 32), dtype=np.uint8)
    t[MAX_KP - 1] = q[1]; t[0] = q[2]                    # dot = +256 at both ends of the index range
    t[MAX_KP - 2] = ~q[4]; t[1] = ~q[5]                  # dot = -256 next to them: keys near -2^22, never the best
    t[MAX_KP - 3] = q[6]; t[2] = _flip(q[6], [0])        # best at the top, second (one bit off) at the bottom
    items = [(q, t)]
    return items, [_reference(q, t)]


def test_whole_index_range(matcher, whole_range):
    """kp_stride = nt = VSLAM_MAX_KP, nq = 32: the best match planted at rows 16383 and 0."""
    items, refs = whole_range
    knn = _run_and_compare(matcher, items, refs, MAX_KP)
    assert knn[0, 1, :2].tolist() == [MAX_KP - 1, 0] and knn[0, 2, :2].tolist() == [0, 0]
    assert knn[0, 6].tolist() == [MAX_KP - 3, 0, 2, 1]
