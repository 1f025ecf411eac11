"""The counting kernel's walk begins behind the 128 matches the screen has evaluated (ransac_count.hip, "Mapping of the count
kernel"): what that moves -- the block edges, the first exit, who evaluates the head, the sum rule's first use -- held to the
oracle bit for bit and to tests/ref64.py, the way tests/test_gpu_ransac.py holds the rest.  The input builders are plain
functions so that the oracle alone can be put through the same holds on a CPU."""
import os

import numpy as np
import pytest
import torch

import ref64
from ransac_inputs import batch as _batch
from test_gpu_ransac import _beaten, _compare, _find, assert_caps, bits, check_counts, check_sums, hold, sums_mode  # noqa: F401

from vslam_amd import synth

pytestmark = pytest.mark.gpu

HEAD = 128      # kScreenMatches
EDGE_SIZES = [8, 100, 128, 129, 130, 383, 384, 385, 639, 640, 641, 897]


def _identity_pairs(B, K):
    return np.tile(np.stack([np.arange(K), np.arange(K)], 1)[None], (B, 1, 1)).astype(np.int32)


def edge_inputs(oracle, Hy):
    """Head = everything (8, 100, 128), head + 1 and + 2, the first block behind the head one short / full / one over
    (383, 384, 385), the same for the second block (639, 640, 641), and a third, partial one (897)."""
    K = 900
    xy1, xy2, pairs, m = _batch(5200 + Hy, EDGE_SIZES, K, 1280, 720)
    sets = np.stack([oracle.ransac_sets(21 + b, n, Hy) for b, n in enumerate(EDGE_SIZES)])
    return xy1, xy2, pairs, m, sets, 10.0


def first_exit_inputs(oracle, exact):
    """55 % inliers: a hypothesis may be abandoned after D = m - bound + 1 certain outliers.  exact (no noise, sub-pixel
    coordinates; sample sets that contain a clean hypothesis): the maximum count is the number of true correspondences and
    D = 309, 345, 362, inside (256, 384] -- the first block behind the head is where hypotheses leave.  Otherwise (half a
    pixel of noise, integer coordinates) 512 hypotheses reach about a quarter of the matches and D is around 500, beyond it."""
    sizes, Hy = [600, 700, 760], 512
    K = max(sizes)
    xy1 = np.zeros((3, K, 2), np.float32); xy2 = np.zeros((3, K, 2), np.float32)
    for b in range(3):
        if exact:
            xy1[b], xy2[b], _ = synth.two_view_points(6100 + b, K, 1280, 720, inlier_frac=0.55, noise_px=0.0, integer=False)
        else:
            xy1[b], xy2[b], _ = synth.two_view_points(6100 + b, K, 1280, 720, inlier_frac=0.55)
    pairs = _identity_pairs(3, K)
    m = np.array(sizes, np.int32)
    seeds = (303, 308, 306) if exact else (300, 301, 302)
    sets = np.stack([oracle.ransac_sets(seeds[b], n, Hy) for b, n in enumerate(sizes)])
    return xy1, xy2, pairs, m, sets, 10.0


def edge_exit_inputs(oracle):
    """The same kind of data (55 % inliers, exact) with match counts at which, with the oracle, D = m - maximum + 1 is 384
    (m = 791: six hypotheses at the maximum; m = 794: one), 385 (m = 796) and 388 (m = 800, three at the maximum): at D = 384 a
    hypothesis without a single potential inlier among its first 384 matches is the only kind that may leave there, at 385 none."""
    sizes, Hy, K = [791, 794, 796, 800], 512, 900
    B = len(sizes)
    xy1 = np.zeros((B, K, 2), np.float32); xy2 = np.zeros((B, K, 2), np.float32)
    for b in range(B):
        xy1[b], xy2[b], _ = synth.two_view_points(6103, K, 1280, 720, inlier_frac=0.55, noise_px=0.0, integer=False)
    pairs = _identity_pairs(B, K)
    m = np.array(sizes, np.int32)
    sets = np.stack([oracle.ransac_sets(320, n, Hy) for n in sizes])
    return xy1, xy2, pairs, m, sets, 10.0


def plateau_inputs(oracle, sizes=(385, 400, 641)):
    """The data of test_sum_rule_on_a_plateau_of_tied_hypotheses (its third item: with the oracle, 130 to 150 of the 512
    hypotheses tie at each of these sizes), with match counts that put the sum rule's first use (one block behind the head:
    384 matches seen) at the last match but one, a few before the end, and in the middle."""
    K, Hy = 1500, 512
    B = len(sizes)
    xy1 = np.zeros((B, K, 2), np.float32); xy2 = np.zeros((B, K, 2), np.float32)
    for b in range(B):
        xy1[b], xy2[b], _ = synth.two_view_points(4102, K, 1280, 720, inlier_frac=0.85, noise_px=0.0, integer=False)
    pairs = _identity_pairs(B, K)
    m = np.array(sizes, np.int32)
    sets = np.stack([oracle.ransac_sets(902, int(m[b]), Hy) for b in range(B)])
    return xy1, xy2, pairs, m, sets, 10.0


def uncertified_inputs(oracle):
    """m = 100 (all head) and m = 300, hypotheses solved by the oracle, then edited: the oracle's winner scaled by 1e-18
    (dd = a0^2 underflows: the screen certifies nothing of its head, yet it keeps a large count), an all-NaN hypothesis, a
    hypothesis with a zero first row.  Returns the inputs and the edited hypF."""
    K, Hy = 300, 96
    sizes = [100, 300]
    xy1, xy2, pairs, m = _batch(7300, sizes, K, 1280, 720)
    sets = np.stack([oracle.ransac_sets(13 + b, n, Hy) for b, n in enumerate(sizes)])
    hypF = np.zeros((2, Hy, 9), np.float32)
    for b, n in enumerate(sizes):
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], 10.0)
        hypF[b] = ref["hypF"]
        w = int(ref["winner"])
        hypF[b, w] *= np.float32(1e-18)
        hypF[b, (w + 1) % Hy] = np.float32("nan")
        hypF[b, (w + 2) % Hy, 0:3] = 0
    return xy1, xy2, pairs, m, sets, hypF


def accept_rule(oracle, xy1, xy2, pairs, hypF, thr):
    """counts, sums, winner, best count of hand-made hypotheses: oracle.residual and src/RansacFilter.cpp:59."""
    Hy = len(hypF)
    counts = np.zeros(Hy, np.int32); sums = np.zeros(Hy, np.float32)
    best, best_sum, winner = 0, np.float32(0.0), -1
    with np.errstate(all="ignore"):
        for h in range(Hy):
            _, c, s_ = oracle.residual(xy1, xy2, pairs, hypF[h], thr)
            counts[h], sums[h] = c, s_
            if c > best or (c == best and s_ > best_sum):
                best, best_sum, winner = c, s_, h
    return counts, sums, winner, best


def float_e(oracle, xy1, xy2, pairs, F, i):
    """The oracle's float e of match i under F: the smallest threshold at which the oracle calls it an inlier (e <= thr),
    found on the bit patterns of the positive floats."""
    lo, hi = 0, 0x7F800000          # +0 .. +inf
    one = pairs[i:i + 1]
    while lo < hi:
        mid = (lo + hi) // 2
        mask, _, _ = oracle.residual(xy1, xy2, one, F, float(np.uint32(mid).view(np.float32)))
        if mask[0]:
            hi = mid
        else:
            lo = mid + 1
    return float(np.uint32(lo).view(np.float32))


def ranked_head(oracle, xy1, xy2, pairs, hypF, thr):
    """The matches ransac_rank_kernel puts in front: ordered by how many of the 8 pilot hypotheses (h = H w / 8) miss them,
    most-missed first, original order among equals; the first 128."""
    Hy, n = len(hypF), len(pairs)
    npil = min(8, Hy)
    missed = np.zeros(n, np.int64)
    for w in range(npil):
        mask, _, _ = oracle.residual(xy1, xy2, pairs, hypF[(Hy * w) // npil], thr)
        missed += (np.asarray(mask[:n]) == 0)
    return np.argsort(-missed, kind="stable")[:HEAD]


def tie_thresholds(oracle, xy1, xy2, pairs, sets, n):
    """Thresholds that are exactly the float e of a match under the F that wins at threshold 10: four of them, from the
    quartiles of that F's residuals and from its largest ones.  Returns [(thr, match)]."""
    ref = oracle.find_fundamental(xy1, xy2, pairs[:n], sets, 10.0)
    F = ref["F"]
    e64 = ref64.residuals(F.reshape(1, 9), xy1, xy2, pairs[:n], 10.0, keep=[0])["e"][0]
    order = np.argsort(e64)
    picks = [int(order[n // 4]), int(order[n // 2]), int(order[(3 * n) // 4]), int(order[n - 5])]
    return [(float_e(oracle, xy1, xy2, pairs[:n], F, i), i) for i in picks], F


@pytest.mark.parametrize("Hy", [3, 129, 257])
def test_new_block_edges(ctx, oracle, sums_mode, Hy):
    xy1, xy2, pairs, m, sets, thr = edge_inputs(oracle, Hy)
    out = _find(ctx, oracle, xy1, xy2, pairs, m, sets, thr)
    stats = ref64.new_ransac_stats()
    for b, n in enumerate(EDGE_SIZES):
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        _compare(out, ref, b, n, sums_mode, (xy1, xy2, pairs, sets, thr), stats)
    assert_caps(stats, len(EDGE_SIZES), "block edges, H = %d" % Hy)


@pytest.mark.parametrize("data", ["inside", "edge", "beyond"])
def test_the_exit_that_now_comes_first(ctx, oracle, data):
    """D = m - bound + 1 inside (256, 384], at its edge (384, 385) and beyond it: the first block behind the head is, or is not
    yet, the first at which a hypothesis can be abandoned.  Every hypothesis at the maximum count must be counted: the count
    exit may never take one.  Asserted: every hypothesis at the maximum that is not beaten on the oracle's float residual sum
    (the only ones the sum rule may report as -1) carries the maximum, the beaten ones carry it or read -1, the winner carries
    it, and D is where the case wants it."""
    xy1, xy2, pairs, m, sets, thr = (edge_exit_inputs(oracle) if data == "edge" else first_exit_inputs(oracle, data == "inside"))
    out = _find(ctx, oracle, xy1, xy2, pairs, m, sets, thr)
    stats = ref64.new_ransac_stats()
    Ds = []
    for b in range(len(m)):
        n = int(m[b])
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        top = ref["hyp_count"] == ref["hyp_count"].max()
        beaten = _beaten(ref["hyp_count"], ref["hyp_sum"])
        got = out["hyp_count"][b]
        Ds.append(n - int(ref["count"]) + 1)
        print("m = %d: maximum count %d, D = %d, %d at the maximum (%d beaten on the sum), %d of them reported -1"
              % (n, ref["count"], Ds[-1], top.sum(), (top & beaten).sum(), (top & (got == -1)).sum()))
        _compare(out, ref, b, n, "ties", (xy1, xy2, pairs, sets, thr), stats)
        assert (got[top & ~beaten] == ref["count"]).all(), b
        assert ((got[top & beaten] == ref["count"]) | (got[top & beaten] == -1)).all(), b
        assert got[ref["winner"]] == ref["count"], b
    if data == "inside":
        assert all(256 < D <= 384 for D in Ds), Ds
    elif data == "edge":
        assert Ds == [384, 384, 385, 388], Ds
    else:
        assert all(D > 384 for D in Ds), Ds
    assert_caps(stats, len(m), "first exit, " + data)


@pytest.mark.parametrize("thr", [10.0, 3e6, 1e-7])
def test_a_head_that_certifies_nothing(ctx, oracle, sums_mode, thr):
    """Survivors whose head the screen could not certify (tiny dd, NaN, a threshold outside [2^-20, 2^20]) evaluate the head
    themselves, through the exact sequence; at threshold 10 the maximum-count hypothesis is such a one."""
    xy1, xy2, pairs, m, sets, hypF = uncertified_inputs(oracle)
    t = lambda a: torch.from_numpy(a).cuda()
    out = ctx.ransac_evaluate(t(xy1), t(xy2), t(pairs), t(m), t(hypF), thr)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["hypF"] = hypF
    stats = ref64.new_ransac_stats()
    for b in range(2):
        n = int(m[b])
        hold(xy1, xy2, pairs, sets, thr, out, b, n, sums_mode, stats, solve=False)
        counts, sums, winner, best = accept_rule(oracle, xy1[b], xy2[b], pairs[b, :n], hypF[b], thr)
        check_counts(out["hyp_count"][b], counts, sums_mode, b, sums)
        check_sums(out["hyp_sum"][b], counts, sums, sums_mode, b, out["hyp_count"][b])
        assert out["best"][b, 0] == winner, (b, out["best"][b], winner, best)
        if thr == 10.0:      # the scaled hypothesis still wins: the maximum belongs to an uncertified head
            scaled = int(np.nonzero(np.abs(hypF[b]).max(axis=1) < 1e-15)[0][0])
            assert counts[scaled] == counts.max(), (b, counts[scaled], counts.max())
        if winner >= 0:
            assert out["best"][b, 1] == best, b
            mask, _, _ = oracle.residual(xy1[b], xy2[b], pairs[b, :n], hypF[b, winner], thr)
            assert np.array_equal(out["mask"][b, :n], mask), b
    print("uncertified heads (only what is decided is asserted)", ref64.ransac_shares(stats))


@pytest.mark.parametrize("b", [0, 1])
def test_in_band_evaluations_inside_the_head(ctx, oracle, sums_mode, b):
    """The threshold is the float e of a match under a hypothesis of the batch: that evaluation is an exact tie, decided by
    `<=`, and lies inside the cheap evaluation's band.  m = 100: every match is head; m = 300: at least one of the tied matches
    is among the 128 in front (checked with a restatement of the ranking)."""
    K, Hy = 300, 64
    sizes = [100, 300]
    xy1, xy2, pairs, m = _batch(7500, sizes, K, 1280, 720)
    n = sizes[b]
    sets = np.stack([oracle.ransac_sets(17 + i, s, Hy) for i, s in enumerate(sizes)])
    ties, _ = tie_thresholds(oracle, xy1[b], xy2[b], pairs[b], sets[b], n)
    in_head = 0
    for thr, i in ties:
        out = _find(ctx, oracle, xy1, xy2, pairs, m, sets, thr)
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        _compare(out, ref, b, n, sums_mode)
        in_head += int(i in ranked_head(oracle, xy1[b], xy2[b], pairs[b, :n], ref["hypF"], thr))
    assert in_head >= 1, ties


def test_sum_rule_across_the_hand_over(ctx, oracle):
    """The sum rule's first use comes one block behind the head, with the screen's sum over the head in it."""
    xy1, xy2, pairs, m, sets, thr = plateau_inputs(oracle)
    out = _find(ctx, oracle, xy1, xy2, pairs, m, sets, thr)
    stats = ref64.new_ransac_stats()
    for b in range(len(m)):
        n = int(m[b])
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        _compare(out, ref, b, n, "ties", (xy1, xy2, pairs, sets, thr), stats)
        tied = ref["hyp_count"] == ref["hyp_count"].max()
        print("m = %d: %d tied, %d of them abandoned on the sum" % (n, tied.sum(), (tied & (out["hyp_count"][b] == -1)).sum()))
        assert tied.sum() >= 40, (n, int(tied.sum()))
    assert_caps(stats, len(m), "plateau across the hand-over")


@pytest.mark.parametrize("data", ["hard", "plateau"])
def test_both_walks_give_the_same_arrays(ctx_exp, oracle, data):
    """The experiments build keeps the walk from ranked match 0 (VSLAM_RANSAC_COUNT_FROM_ZERO): hyp_count, hyp_sum, best, F
    and mask are equal bit for bit between the two walks, and between two calls of each.

    Which tied hypotheses the sum rule abandons must not depend on where a walk's sub-blocks end: the rule is applied once
    more over the whole walk, which is at least as tight as every earlier use of it."""
    xy1, xy2, pairs, m, sets, thr = first_exit_inputs(oracle, True) if data == "hard" else plateau_inputs(oracle, (1500, 641, 400))
    keys = ("best", "F", "mask", "hyp_count", "hyp_sum")
    runs = {}
    assert "VSLAM_RANSAC_COUNT_FROM_ZERO" not in os.environ
    try:
        for walk in ("head", "zero"):
            if walk == "zero":
                os.environ["VSLAM_RANSAC_COUNT_FROM_ZERO"] = "1"
            runs[walk] = [_find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr) for _ in range(2)]
    finally:
        os.environ.pop("VSLAM_RANSAC_COUNT_FROM_ZERO", None)
    for k in keys:
        view = (lambda a: bits(a)) if runs["head"][0][k].dtype == np.float32 else (lambda a: a)
        for walk in ("head", "zero"):
            assert np.array_equal(view(runs[walk][0][k]), view(runs[walk][1][k])), (walk, k)
    # the figures first: where the two walks differ, and whether only in what the sum rule may abandon
    ch, cz = runs["head"][0]["hyp_count"], runs["zero"][0]["hyp_count"]
    top = np.maximum(ch, cz) == np.maximum(ch, cz).max(axis=1, keepdims=True)
    print("%s: hyp_count differs at %d of %d hypotheses (%d abandoned by the walk behind the head only, %d by the walk from zero "
          "only; %d of the differences at the pair's maximum count), hyp_sum bits at %d"
          % (data, (ch != cz).sum(), ch.size, ((ch == -1) & (cz != -1)).sum(), ((cz == -1) & (ch != -1)).sum(),
             ((ch != cz) & top).sum(), (bits(runs["head"][0]["hyp_sum"]) != bits(runs["zero"][0]["hyp_sum"])).sum()))
    for k in keys:
        view = (lambda a: bits(a)) if runs["head"][0][k].dtype == np.float32 else (lambda a: a)
        assert np.array_equal(view(runs["head"][0][k]), view(runs["zero"][0][k])), k
