"""head_on_certificate (ransac_prune_tile.h), the second path of ransac_screen_kernel: the head of a pair -- its 128 most-missed
matches -- on the prune certificate instead of the cheap evaluation, for the pairs whose hypotheses have to miss more matches
than the head holds.
(a) routing: both paths are taken in one launch, and every pair the prune gate can open goes to the certificate;
(b) what it hands on is true: pot0 is an upper bound of the head's exact inliers and never above n0, and says n0 for a
    hypothesis outside the certificate's ranges;
(c) nothing the RANSAC stage returns changes: route forced on, forced off (VSLAM_RANSAC_HEAD_ROUTE, experiments build) and
    the default routing give the same arrays, the product the same again, and the forced-on run is held to the oracle.

hyp_count and the sum rule.  Among the hypotheses that tie the pair's maximum count, ransac_count_kernel may report -1 for
one that is beaten on the residual sum, and which of the beaten ones it does depends on the sum floor ransac_cand_kernel
found and on the block layout of the walk ("Either is correct", ransac_count.hip) -- both move with pot0 and with who
evaluates the head.  So hyp_count is compared bit for bit between the default routing, the route forced off and the product
(the pairs the default sends to the certificate included), and between forced on and forced off at every hypothesis but the
beaten ties the oracle names: there each run reads the oracle's maximum or -1, the contract
tests/test_gpu_ransac.py::check_counts holds every run to.  A pair in which the oracle finds no beaten tie is compared bit for
bit on / off as well (at least three per hypothesis count, of both kinds of data, one of them routed by default).
Measured with the route forced on for the exact 95 % pair of 700 matches, which the default never sends to the certificate: 2 of 33 and 9 of 130 hypotheses read 603 (the maximum) where the screen's run reads -1, all of them beaten ties; no
other entry of hyp_count, and nothing of best, F and the match list, differs anywhere."""
import numpy as np
import pytest

import ref64
from test_gpu_prune import _env, _evaluate
from test_gpu_ransac import _beaten, _compare, _find, assert_caps, bits
from test_gpu_ransac_headstart import HEAD, _identity_pairs, accept_rule, ranked_head

from vslam_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [8, 127, 128, 129, 160, 700]          # all head, one short of a tile border, the head exactly, one and a tile behind it
HYPS = [31, 33, 128, 130]                     # a partial wave, one lane into the second, a full workgroup, two lanes into the next
KEYS = ("hyp_count", "best", "F", "mask")     # after ransac_ties: the counts, the winner (with its count and sum), F, the match list
THR = 10.0


def head_inputs(oracle, Hy):
    """Twelve pairs: every size once with 30 % inliers (no sample of eight is clean: every pilot is garbage and the hypotheses
    have to miss hundreds of matches) and once with 95 % exact inliers (some pilot reaches nearly every match)."""
    K = max(SIZES)
    sizes = SIZES + SIZES
    B = len(sizes)
    xy1 = np.zeros((B, K, 2), np.float32); xy2 = np.zeros((B, K, 2), np.float32)
    for b in range(B):
        if b < len(SIZES):
            xy1[b], xy2[b], _ = synth.two_view_points(8100 + b, K, 1280, 720, inlier_frac=0.30)
        else:
            xy1[b], xy2[b], _ = synth.two_view_points(8200 + b, K, 1280, 720, inlier_frac=0.95, noise_px=0.0, integer=False)
    pairs = _identity_pairs(B, K)
    m = np.array(sizes, np.int32)
    sets = np.stack([oracle.ransac_sets(700 + b, n, Hy) for b, n in enumerate(sizes)])
    return xy1, xy2, pairs, m, sets, THR


def _same(a, b, tag, beaten=None, top=None):
    """KEYS of two runs bit for bit.  beaten (batch x hyp bool) and top (batch: the pair's maximum count), both from the
    oracle: a pair without a beaten tie is compared bit for bit like everything else; in a pair that has some, hyp_count may
    differ at those hypotheses only, and only as -1 against the oracle's maximum.  Returns the pairs compared strictly."""
    strict = []
    for k in KEYS:
        x, y = (bits(a[k]), bits(b[k])) if a[k].dtype == np.float32 else (a[k], b[k])
        if k == "hyp_count" and beaten is not None:
            diff = x != y
            print("%s: hyp_count differs at %d hypotheses, %d of them beaten ties" % (tag, diff.sum(), (diff & beaten).sum()))
            for p in range(len(x)):
                if not beaten[p].any():      # no tie plateau: nothing of this pair is excepted
                    assert np.array_equal(x[p], y[p]), (tag, k, p, np.argwhere(diff[p])[:4])
                    strict.append(p)
            assert not (diff & ~beaten).any(), (tag, k, np.argwhere(diff & ~beaten)[:4])
            t = np.asarray(top).reshape(-1, 1)
            assert (((x == -1) & (y == t)) | ((y == -1) & (x == t)))[diff].all(), (tag, k)
        else:
            assert np.array_equal(x, y), (tag, k)
    return strict


_RUNS = {}


def _runs(ctx_exp, oracle, Hy):
    """The three routings of one batch through the experiments build, each with pot0 and the routing word as the head's kernels
    left them; computed once per hypothesis count."""
    if Hy not in _RUNS:
        inp = head_inputs(oracle, Hy)
        runs = {}
        for name, env in (("default", {}), ("on", {"VSLAM_RANSAC_HEAD_ROUTE": 1}), ("off", {"VSLAM_RANSAC_HEAD_ROUTE": 0})):
            with _env(**env):
                out = _find(ctx_exp, oracle, *inp)
                pot0, route = ctx_exp.debug_ransac_head(len(inp[3]), Hy)
                ctx_exp.synchronize()
            out["pot0"], out["route"] = pot0.cpu().numpy(), route.cpu().numpy()
            runs[name] = out
        _RUNS[Hy] = (inp, runs)
    return _RUNS[Hy]


def _head_inliers(oracle, xy1, xy2, pairs, hypF, thr):
    """Per hypothesis: the matches of the ranked head that the oracle's exact sequence calls inliers."""
    head = ranked_head(oracle, xy1, xy2, pairs, hypF, thr)
    out = np.zeros(len(hypF), np.int64)
    with np.errstate(all="ignore"):
        for h in range(len(hypF)):
            mask, _, _ = oracle.residual(xy1, xy2, pairs, hypF[h], thr)
            out[h] = int((np.asarray(mask[:len(pairs)]) != 0)[head].sum())
    return out


@pytest.mark.parametrize("Hy", HYPS)
def test_both_routes_in_one_launch(ctx_exp, oracle, Hy):
    """(a) the default routing sends pairs both ways; a pair the prune gate opens with the FINAL bound (the oracle's maximum
    count, never below the pilots' bound the routing uses) is always on the certificate; forcing sends every pair one way."""
    (xy1, xy2, pairs, m, sets, thr), runs = _runs(ctx_exp, oracle, Hy)
    route = runs["default"]["route"]
    print("H = %d: routing word %s" % (Hy, route.tolist()))
    assert set(route.tolist()) == {0, 1}, route
    for b in range(len(m)):
        n = int(m[b])
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        if n - int(ref["hyp_count"].max()) + 1 > min(n, HEAD):
            assert route[b] == 1, (b, n, int(ref["hyp_count"].max()))
    assert (runs["on"]["route"] == 1).all() and (runs["off"]["route"] == 0).all()
    # m = 700: no pilot of the 30 % pair comes near 573 inliers (certificate); some pilot of the exact 95 % pair does (cheap evaluation)
    assert route[SIZES.index(700)] == 1 and route[len(SIZES) + SIZES.index(700)] == 0, route


@pytest.mark.parametrize("Hy", HYPS)
def test_pot0_bounds_the_heads_inliers(ctx_exp, oracle, Hy):
    """(b) for every hypothesis of a routed pair: exact head inliers <= pot0 <= n0 -- with every pair routed (forced) and
    with the default routing."""
    (xy1, xy2, pairs, m, sets, thr), runs = _runs(ctx_exp, oracle, Hy)
    hypF = runs["on"]["hypF"]
    slack = 0
    for b in range(len(m)):
        n = int(m[b])
        n0 = min(n, HEAD)
        exact = _head_inliers(oracle, xy1[b], xy2[b], pairs[b, :n], hypF[b], thr)
        for name in ("on", "default"):
            if runs[name]["route"][b] != 1:
                continue
            pot0 = runs[name]["pot0"][b]
            assert (pot0 >= exact).all(), (name, b, n, np.argwhere(pot0 < exact)[:4])
            assert (pot0 <= n0).all(), (name, b, n)
        slack += int((runs["on"]["pot0"][b] - exact).sum())
    print("H = %d: pot0 - exact head inliers sums to %d over %d hypotheses" % (Hy, slack, len(m) * Hy))
    # where the default leaves a pair to the screen, pot0 is the screen's, untouched by the new kernel
    keep = runs["default"]["route"] == 0
    assert np.array_equal(runs["default"]["pot0"][keep], runs["off"]["pot0"][keep])


def test_pot0_of_a_hypothesis_the_certificate_does_not_cover(ctx_exp, oracle):
    """(b) |f| > 2^10 and a NaN in F: nothing of the head is certified, pot0 == n0 -- and the stage's result still equals the
    screen's."""
    Hy = 33
    (xy1, xy2, pairs, m, sets, thr), runs = _runs(ctx_exp, oracle, Hy)
    hypF = runs["on"]["hypF"].copy()
    big, nan = [1, 32], [5, 31]
    hypF[:, big] *= np.float32(4096.0)
    assert (np.abs(hypF[:, big]).max(axis=2) > 1024.0).all()
    hypF[:, nan[0], 4] = np.float32("nan")
    hypF[:, nan[1]] = np.float32("nan")
    with _env(VSLAM_RANSAC_HEAD_ROUTE=1):
        on = _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, thr)
        pot0, route = ctx_exp.debug_ransac_head(len(m), Hy)
        ctx_exp.synchronize()
    with _env(VSLAM_RANSAC_HEAD_ROUTE=0):
        off = _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, thr)
    pot0 = pot0.cpu().numpy()
    assert (route.cpu().numpy() == 1).all()
    n0 = np.minimum(m, HEAD)
    for h in big + nan:
        assert np.array_equal(pot0[:, h], n0), (h, pot0[:, h], n0)
    beaten = np.zeros(pot0.shape, bool)
    top = np.zeros(len(m), np.int64)
    for b in range(len(m)):
        n = int(m[b])
        counts, sums, _, _ = accept_rule(oracle, xy1[b], xy2[b], pairs[b, :n], hypF[b], thr)
        beaten[b], top[b] = _beaten(counts, sums), counts.max()
    _same(on, off, "uncovered hypotheses, on / off", beaten, top)


@pytest.mark.parametrize("Hy", HYPS)
def test_nothing_changes_with_the_route(ctx, ctx_exp, oracle, Hy):
    """(c) hyp_count, the winner, F as uint32 and the match list after ransac_ties: default routing, route forced off and the
    product, all equal; route forced on equal to them but for which beaten ties read -1 (the module's docstring); the
    forced-on run against the oracle and tests/ref64.py."""
    inp, runs = _runs(ctx_exp, oracle, Hy)
    xy1, xy2, pairs, m, sets, thr = inp
    product = _find(ctx, oracle, *inp)
    _same(runs["default"], runs["off"], "default / off")
    _same(product, runs["off"], "product / off")
    stats = ref64.new_ransac_stats()
    beaten = np.zeros(runs["on"]["hyp_count"].shape, bool)
    top = np.zeros(len(m), np.int64)
    for b in range(len(m)):
        n = int(m[b])
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        beaten[b], top[b] = _beaten(ref["hyp_count"], ref["hyp_sum"]), ref["hyp_count"].max()
        _compare(runs["on"], ref, b, n, "ties", (xy1, xy2, pairs, sets, thr), stats)
    strict = _same(runs["on"], runs["off"], "H = %d, on / off" % Hy, beaten, top)
    # the exception covers the tie plateaus only: pairs without one are compared bit for bit, on both kinds of data and
    # among them one the default routing itself sends to the certificate
    print("H = %d: pairs compared bit for bit on / off: %s" % (Hy, strict))
    assert len(strict) >= 3 and min(strict) < len(SIZES) <= max(strict), strict
    assert any(runs["default"]["route"][p] == 1 for p in strict), (strict, runs["default"]["route"])
    assert_caps(stats, len(m), "head on the certificate, H = %d" % Hy)
