"""ransac_prune_mfma_kernel (ransac_prune.hip): hypotheses ruled out on the f32 matrix cores before the count kernel walks them.
(a) nothing the RANSAC stage returns changes with it (VSLAM_RANSAC_NO_PRUNE, experiments build), and both are held to the oracle;
(b) what it certifies is true: X[h], its certified misses behind the ranked head, never exceeds the oracle's outliers there;
(c) it happens on the data it is for, and never to a hypothesis at the maximum count; (d) the operand / accumulator mapping of
v_mfma_f32_32x32x2_f32 that the kernel is written to, against a scalar loop on one tile."""
import os

import numpy as np
import pytest
import torch

import ref64
from test_gpu_ransac import _compare, _find, assert_caps, bits, check_counts, check_sums, hold  # noqa: F401
from test_gpu_ransac_headstart import (EDGE_SIZES, HEAD, accept_rule, edge_exit_inputs, edge_inputs, first_exit_inputs,  # noqa: F401
                                       plateau_inputs, ranked_head, uncertified_inputs)

pytestmark = pytest.mark.gpu

KEYS = ("best", "F", "mask", "hyp_count", "hyp_sum")
INPUTS = {
    "edges 3": lambda o: edge_inputs(o, 3), "edges 129": lambda o: edge_inputs(o, 129), "edges 257": lambda o: edge_inputs(o, 257),
    "first exit exact": lambda o: first_exit_inputs(o, True), "first exit noisy": lambda o: first_exit_inputs(o, False),
    "edge exit": edge_exit_inputs, "plateau": plateau_inputs,
}


def _env(**kw):
    class E:
        def __enter__(self):
            for k in kw:
                assert k not in os.environ, k
                os.environ[k] = str(kw[k])

        def __exit__(self, *a):
            for k in kw:
                os.environ.pop(k, None)
    return E()


def _same(a, b, tag):
    for k in KEYS:
        view = bits if a[k].dtype == np.float32 else (lambda v: v)
        assert np.array_equal(view(a[k]), view(b[k])), (tag, k)


def _evaluate(ctx, xy1, xy2, pairs, m, hypF, thr):
    t = lambda a: torch.from_numpy(a).cuda()
    out = ctx.ransac_evaluate(t(xy1), t(xy2), t(pairs), t(m), t(hypF), thr)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["hypF"] = hypF
    return out


@pytest.mark.parametrize("name", list(INPUTS))
def test_nothing_changes_with_the_prune_kernel(ctx, ctx_exp, oracle, name):
    """(a) hyp_count, hyp_sum, best, F and the mask: the product, the experiments build, and the experiments build without the
    prune kernel, bit for bit; the product's held to the oracle and to tests/ref64.py.

    Why hyp_count can be compared bit for bit: a pruned hypothesis lies below the pair's maximum count, and ransac_ties_kernel
    writes -1 for every such hypothesis whatever ransac_count_kernel found for it (its exact count, or -1 after abandoning
    it).  The count kernel's own output, before ransac_ties, may differ between the two runs -- a certified miss of the prune
    kernel need not be a certain outlier of the cheap evaluation -- and is not what is compared here.  At the maximum count
    nothing is pruned; which beaten tied hypotheses the sum rule reports as -1 does not depend on the prune kernel."""
    xy1, xy2, pairs, m, sets, thr = INPUTS[name](oracle)
    out = _find(ctx, oracle, xy1, xy2, pairs, m, sets, thr)
    with_prune = _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr)
    X = ctx_exp.debug_ransac_prune_x(len(m), sets.shape[1])
    ctx_exp.synchronize()
    with _env(VSLAM_RANSAC_NO_PRUNE=1):
        without = _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr)
    with _env(VSLAM_RANSAC_PRUNE_GATE=0):      # every pair walked, also those the gate leaves to the screen
        ungated = _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr)
        X0 = ctx_exp.debug_ransac_prune_x(len(m), sets.shape[1])
        ctx_exp.synchronize()
    print("%s: X > 0 at %d of %d hypotheses (without the gate: %d)"
          % (name, int((X.cpu().numpy() > 0).sum()), X.numel(), int((X0.cpu().numpy() > 0).sum())))
    _same(with_prune, without, name + ": with / without")
    _same(ungated, without, name + ": without the gate / without")
    _same(out, without, name + ": product / without")
    stats = ref64.new_ransac_stats()
    for b in range(len(m)):
        n = int(m[b])
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        for o in (out, without):
            _compare(o, ref, b, n, "ties", (xy1, xy2, pairs, sets, thr) if o is out else None, stats if o is out else None)
    assert_caps(stats, len(m), name)


@pytest.mark.parametrize("thr", [10.0, 3e6, 1e-7])
def test_nothing_changes_on_uncertified_hypotheses(ctx, ctx_exp, oracle, thr):
    """(a) on hypotheses scaled by 1e-18, all NaN, with a zero first row, and thresholds outside the stated range."""
    xy1, xy2, pairs, m, sets, hypF = uncertified_inputs(oracle)
    out = _evaluate(ctx, xy1, xy2, pairs, m, hypF, thr)
    with_prune = _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, thr)
    with _env(VSLAM_RANSAC_NO_PRUNE=1):
        without = _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, thr)
    with _env(VSLAM_RANSAC_PRUNE_GATE=0):
        ungated = _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, thr)
    _same(with_prune, without, "with / without")
    _same(ungated, without, "without the gate / without")
    _same(out, without, "product / without")
    stats = ref64.new_ransac_stats()
    for b in range(2):
        n = int(m[b])
        counts, sums, winner, best = accept_rule(oracle, xy1[b], xy2[b], pairs[b, :n], hypF[b], thr)
        for o in (out, without):
            check_counts(o["hyp_count"][b], counts, "ties", b, sums)
            check_sums(o["hyp_sum"][b], counts, sums, "ties", b, o["hyp_count"][b])
            assert o["best"][b, 0] == winner, (b, o["best"][b], winner, best)
        hold(xy1, xy2, pairs, sets, thr, out, b, n, "ties", stats, solve=False)


def _outliers_behind_the_head(oracle, xy1, xy2, pairs, hypF, thr):
    """Per hypothesis: the matches behind the ranked head that the oracle does not call inliers."""
    n = len(pairs)
    head = ranked_head(oracle, xy1, xy2, pairs, hypF, thr)
    behind = np.ones(n, bool)
    behind[head] = False
    out = np.zeros(len(hypF), np.int64)
    with np.errstate(all="ignore"):
        for h in range(len(hypF)):
            mask, _, _ = oracle.residual(xy1, xy2, pairs, hypF[h], thr)
            out[h] = int((np.asarray(mask[:n]) == 0)[behind].sum())
    return out


@pytest.mark.parametrize("name", ["edges 129", "first exit exact", "plateau", "uncertified"])
def test_certified_misses_are_misses(ctx_exp, oracle, name):
    """(b) X[h] <= the number of matches behind the ranked head that the oracle calls outliers, for every hypothesis."""
    with _env(VSLAM_RANSAC_PRUNE_GATE=0):      # every pair walked
        if name == "uncertified":
            xy1, xy2, pairs, m, sets, hypF = uncertified_inputs(oracle)
            thr = 10.0
            _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, thr)
        else:
            xy1, xy2, pairs, m, sets, thr = INPUTS[name](oracle)
            hypF = _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr)["hypF"]
        X = ctx_exp.debug_ransac_prune_x(len(m), hypF.shape[1])
        ctx_exp.synchronize()
    X = X.cpu().numpy()
    for b in range(len(m)):
        n = int(m[b])
        if n <= HEAD:
            assert (X[b] == 0).all(), (b, n)
            continue
        miss = _outliers_behind_the_head(oracle, xy1[b], xy2[b], pairs[b, :n], hypF[b], thr)
        print("%s m = %d: X sums to %d, the oracle's outliers behind the head to %d" % (name, n, X[b].sum(), miss.sum()))
        assert (X[b] <= miss).all(), (b, n, np.argwhere(X[b] > miss)[:4])
        assert (X[b] <= n - HEAD).all(), (b, n)


def _payload_run(ctx_exp, oracle, inp, **knobs):
    xy1, xy2, pairs, m, sets, thr = inp
    with _env(VSLAM_RANSAC_COUNT_EXIT_PAYLOAD=1):
        with _env(VSLAM_RANSAC_NO_PRUNE=1):
            without = _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr)
        with _env(**knobs):
            with_prune = _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr)
    # never walked by the count kernel: the payload is all ones, or none at all where a whole workgroup had nobody left (an
    # abandoned walk carries the matches it had seen, at least 129)
    pay = lambda o: bits(o["hyp_sum"]) & 0x3FFFFF
    early = lambda o: (o["hyp_count"] < 0) & ((pay(o) == 0x3FFFFF) | (pay(o) == 0))
    return early(with_prune) & ~early(without), with_prune


def test_it_prunes_the_hard_data(ctx_exp, oracle):
    """(c) first_exit_inputs(exact=True): the count kernel abandons 99.97 % of such hypotheses and their |n| lies orders of
    magnitude beyond the band, so at least half of all hypotheses are ruled out before it."""
    inp = first_exit_inputs(oracle, True)
    pruned, _ = _payload_run(ctx_exp, oracle, inp)
    share = pruned.mean(axis=1)
    print("pruned share per pair:", share, "overall %.3f" % pruned.mean())
    assert pruned.mean() >= 0.5, share


def test_no_maximum_count_hypothesis_is_pruned(ctx_exp, oracle):
    """(c) plateau_inputs: 130 to 150 hypotheses tie at the maximum count; none of them is pruned -- with the pair-level gate
    off, so that the kernel walks these pairs at all."""
    inp = plateau_inputs(oracle)
    xy1, xy2, pairs, m, sets, thr = inp
    pruned, _ = _payload_run(ctx_exp, oracle, inp, VSLAM_RANSAC_PRUNE_GATE=0)
    for b in range(len(m)):
        n = int(m[b])
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        top = ref["hyp_count"] == ref["hyp_count"].max()
        print("m = %d: %d at the maximum, %d pruned in all" % (n, top.sum(), pruned[b].sum()))
        assert not (pruned[b] & top).any(), b


def test_mfma_tile_layout_against_a_scalar_loop(ctx_exp):
    """(d) one 32 x 32 tile through the kernel's own operand and accumulator mapping.  Small integers, every F and coordinate
    different (nothing symmetric between hypotheses and matches): all sums are exact, so the comparison is equality."""
    rng = np.random.default_rng(5)
    F = rng.integers(-9, 10, (32, 9)).astype(np.float32)
    F += np.arange(32, dtype=np.float32)[:, None] * 4           # row h is recognisable
    xy = rng.integers(1, 30, (4, 32)).astype(np.float32)
    xy[0] += np.arange(32, dtype=np.float32) * 8                # so is column j
    n, a0 = ctx_exp.debug_ransac_prune_tile(torch.from_numpy(F).cuda(), torch.from_numpy(xy).cuda())
    ctx_exp.synchronize()
    want_n = np.zeros((32, 32)); want_a0 = np.zeros((32, 32)); largest = 0.0
    for h in range(32):
        for j in range(32):
            x1, y1, x2, y2 = (float(v) for v in xy[:, j])
            phi = (x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0)
            want_n[h, j] = sum(float(F[h, k]) * phi[k] for k in range(9))
            want_a0[h, j] = float(F[h, 0]) * x1 + float(F[h, 1]) * y1 + float(F[h, 2])
            largest = max(largest, sum(abs(float(F[h, k]) * phi[k]) for k in range(9)))
    assert largest < 2 ** 24                                    # every partial sum in any order is an integer f32 holds
    assert np.array_equal(n.cpu().numpy().astype(np.float64), want_n)
    assert np.array_equal(a0.cpu().numpy().astype(np.float64), want_a0)
