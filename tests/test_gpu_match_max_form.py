"""The FP4 matcher's running maximum (match.hip, max_nonan): a bare v_max_f32 where fmaxf() made the compiler quiet every
loop-carried operand first.  No result bit may move: the product, the experiments build, and the experiments build with the
earlier form switched back in (VSLAM_MATCH_MAX_FORM=fmaxf) are held to the oracle's knn-2 and to the numpy definition of
tests/ref_int.py, and to one another, on one pair per case at kp_stride 96: the tile tails on both operands, fewer than two
train rows, and what a maximum over keys can get wrong -- equal keys but for the index, in one tile and across tiles, and
the two ends of the key's range (Hamming distance 0 and 256)."""
import numpy as np
import pytest

from test_gpu_match import _flip, _pack
from test_gpu_match_keys import NONE, _reference
from test_gpu_prune import _env

pytestmark = pytest.mark.gpu

K = 96
SIZES = [(1, 1), (1, 2), (31, 33), (32, 32), (33, 65), (64, 96), (65, 31)]


def _random(rng, nq, nt):
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for i in range(0, nq, 3):      # a third of the queries get a near copy somewhere: survivors of the ratio test
        t[(7 * i + nt - 1) % nt] = _flip(q[i], rng.choice(256, int(rng.integers(0, 30)), replace=False))
    return q, t


@pytest.fixture(scope="module")
def cases():
    """[(tag, q, t)], and per case the reference (knn records, surviving pairs).  Made once, never written to."""
    rng = np.random.default_rng(1212)
    items = []
    for nq, nt in SIZES:
        items.append((f"random {nq}x{nt}", *_random(rng, nq, nt)))
    for nq, nt in SIZES:
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        items.append((f"equal trains {nq}x{nt}", q, np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), nt, 0)))
    for nq, nt in SIZES:
        if nt < 2:
            continue
        q, t = _random(rng, nq, nt)
        t[:] = ~q[0]                      # every train row at distance 256 from query 0 ...
        t[nt - 1] = q[0]                  # ... but the last one, at distance 0
        items.append((f"extremes {nq}x{nt}", q, t))
    for nq, nt, rows in [(33, 65, (3, 40)), (33, 65, (34, 61)), (64, 96, (31, 32)), (64, 96, (0, 95)), (65, 31, (7, 8)),
                         (32, 32, (5, 30, 31))]:
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)      # (no near copies here: random rows lie about 128 bits apart)
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        for r in rows:
            t[r] = _flip(q[nq - 1], [9, 100, 255])      # the last query's best, three bits off, at each of these rows
        items.append((f"ties {nq}x{nt} at {rows}", q, t))
    for _, q, t in items:
        q.setflags(write=False)
        t.setflags(write=False)
    return items, [_reference(q, t) for _, q, t in items]


def _match(c, items, **env):
    d1, n1 = _pack([it[1] for it in items], K)
    d2, n2 = _pack([it[2] for it in items], K)
    with _env(**env):
        pairs, m, knn = c.match_knn2_ratio(d1, n1, d2, n2, want_knn=True)
        c.synchronize()
    return pairs.cpu().numpy(), m.cpu().numpy(), knn.cpu().numpy()


def _hold(out, items, refs, tag):
    pairs, m, knn = out
    for b, ((name, q, t), (want_knn, want_pairs)) in enumerate(zip(items, refs)):
        got = knn[b, :len(q)]
        bad = np.nonzero((got != want_knn).any(1))[0]
        assert bad.size == 0, (tag, name, bad[:4], got[bad[:4]], want_knn[bad[:4]])
        assert m[b] == len(want_pairs) and np.array_equal(pairs[b, :m[b]], want_pairs), (tag, name, m[b], len(want_pairs))


@pytest.fixture(scope="module")
def outputs(cases, ctx, ctx_exp):
    items, _ = cases
    return {"product": _match(ctx, items), "experiments": _match(ctx_exp, items),
            "experiments, fmaxf": _match(ctx_exp, items, VSLAM_MATCH_MAX_FORM="fmaxf")}


@pytest.mark.parametrize("form", ["product", "experiments", "experiments, fmaxf"])
def test_against_the_definition(cases, outputs, form):
    items, refs = cases
    assert len(items) == 7 + 7 + 6 + 6
    _hold(outputs[form], items, refs, form)


def test_against_the_oracle(cases, outputs, oracle):
    """The oracle's knn-2 and ratio test wherever it defines them (two train rows or more)."""
    items, _ = cases
    pairs, m, knn = outputs["product"]
    seen = 0
    for b, (name, q, t) in enumerate(items):
        if len(t) < 2:
            assert m[b] == 0 and (knn[b, :len(q), 2] == -1).all() and (knn[b, :len(q), 3] == NONE).all(), name   # no second
            continue
        i0, e0, i1, e1 = oracle.match_knn2(q, t)
        g = knn[b, :len(q)]
        assert np.array_equal(g[:, 0], i0) and np.array_equal(g[:, 1], e0), name
        assert np.array_equal(g[:, 2], i1) and np.array_equal(g[:, 3], e1), name
        ref, rc = oracle.match_knn2_ratio(q, t)
        assert rc == 0 and m[b] == len(ref) and np.array_equal(pairs[b, :m[b]], ref), name
        seen += 1
    assert seen == len(items) - 2


def test_forms_agree_bit_for_bit(cases, outputs):
    items, _ = cases
    p0, m0, k0 = outputs["product"]
    for form in ("experiments", "experiments, fmaxf"):
        p, m, k = outputs[form]
        assert np.array_equal(m, m0), form
        for b, (name, q, _) in enumerate(items):
            assert np.array_equal(k[b, :len(q)], k0[b, :len(q)]) and np.array_equal(p[b, :m[b]], p0[b, :m0[b]]), (form, name)


def test_what_the_cases_are_for(cases, outputs):
    """Equal train rows: the lowest index wins, the second lowest is second, nothing passes the ratio test.  Extremes: distance 0
    at the last row and 256 at row 0.  Ties: the planted rows in index order, in one tile (rows // 32 equal) and across."""
    items, _ = cases
    pairs, m, knn = outputs["product"]
    spans = set()
    for b, (name, q, t) in enumerate(items):
        g = knn[b, :len(q)]
        if name.startswith("equal trains") and len(t) >= 2:
            assert (g[:, 0] == 0).all() and (g[:, 2] == 1).all() and (g[:, 1] == g[:, 3]).all() and m[b] == 0, name
        if name.startswith("extremes"):
            assert g[0].tolist() == [len(t) - 1, 0, 0, 256], (name, g[0])
        if name.startswith("ties"):
            rows = [int(x) for x in name.split("(")[1].rstrip(")").split(",")]
            assert g[-1].tolist() == [rows[0], 3, rows[1], 3], (name, g[-1])
            spans.add(rows[0] // 32 == rows[1] // 32)
    assert spans == {True, False}
