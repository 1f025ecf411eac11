"""A wider net for rare events: a few dozen frame pairs at the headline shape (1280x720, 2000 keypoints,
4096 hypotheses), at a mid-size shape and at the largest configured shape (1920x1080, 4000 keypoints, 8192
hypotheses), every output compared with the oracle bit for bit.  The oracle runs
in a process pool (about 0.1 s per pair and core), so the whole test stays within seconds.

What this is for: the code paths that only fire on unusual values — the slow branch of the correctly rounded
square root, the out-of-range branch of the short f64 division / square root in the Jacobi rotation,
near-tie convergence tests, strip-edge candidates that fail their completed 3x3 test, Lemire rejections — are
each covered by a directed test; this one checks that nothing else hides in the bulk (about 10^8 rotations and
10^8 responses per run)."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import torch

import ref64
import ref_int
from vslam_amd import shard, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def hold_every_fourth_pair(ctx, out, ref, seeds, K, H, P, tag, caps):
    """Pairs 0, 4, 8, ... of a front-end batch are also held to the definitions of tests/ref_int.py and tests/ref64.py, which
    were not written from the oracle.  Every fourth and not every pair: the hold costs 0.4 s (640 x 480, 1024 hypotheses),
    2.5 s (1280 x 720, 4096) and 10.5 s (1920 x 1080, 8192: 27 million float64 evaluations, chunked) of one core per pair,
    the oracle 0.1, 0.45 and 1.2 s; all 54 pairs of test_many_pairs_bit_exact would add 130 s to the 20 s the oracle needs.
    The front-end returns no per-hypothesis outputs, so the RANSAC stage runs once more on the matches and sets that the
    definitions give from the front-end's own keypoints and descriptors; its winner, F and matches must be the front-end's,
    and its outputs go through ref64.hold_ransac.
    caps=True (the hard regime: rotation + parallax, sub-pixel resampling -- a proper two-view geometry) asserts the caps of
    the regular inputs: at most 1 % of the evaluations undecided, at least half of the solves decided, every winner check
    held.  caps=False (the plain synthetic frames): corners sit on integer pixels and move little between the two frames, so
    many 8-point samples are ill-conditioned (a quarter to two thirds of the solves are decided) and on a pair without
    parallax a fifth of the evaluations lies within its bound of the threshold; what is decided is asserted, the shares are
    printed, and most winner checks must be held."""
    held = [q for q in ref if q[0] % 4 == 0]
    prs = np.zeros((len(held), K, 2), np.int32); pm = np.zeros(len(held), np.int32); sets = np.zeros((len(held), H, 8), np.int32)
    for i, (p, a, b, m) in enumerate(held):
        na, nb = int(out["n"][p]), int(out["n"][P + p])
        pr = ref_int.ratio_pairs(out["desc"][p, :na], out["desc"][P + p, :nb])
        assert len(pr) == m["prelim"], p
        prs[i, :len(pr)] = pr; pm[i] = len(pr)
        if len(pr) >= 8:
            sets[i] = ref_int.lemire_sets(int(seeds[p]), len(pr), H)
    xa = np.stack([out["xy"][p] for p, _, _, _ in held]); xb = np.stack([out["xy"][P + p] for p, _, _, _ in held])
    t = lambda v: torch.from_numpy(v).cuda()
    stage = ctx.ransac_fundamental(t(xa), t(xb), t(prs), t(pm), t(sets), 10.0)
    ctx.synchronize()
    stage = {k: v.cpu().numpy() for k, v in stage.items()}
    stats = ref64.new_ransac_stats()
    for i, (p, a, b, m) in enumerate(held):
        if pm[i] < 8:
            continue
        k = int(stage["best"][i, 3])
        assert np.array_equal(stage["best"][i], out["best"][p]) and stage["F"][i].tobytes() == out["F"][p].tobytes(), p
        assert np.array_equal(stage["matches"][i, :k], out["matches"][p, :k]), p
        ref64.add_ransac_stats(stats, ref64.hold_ransac(xa[i], xb[i], prs[i, :pm[i]], sets[i], 10.0,
                                                        {k_: v[i] for k_, v in stage.items()}, "ties"))
    print("%s: %d of %d pairs held to ref_int / ref64:" % (tag, len(held), P), ref64.ransac_shares(stats))
    assert stats["pairs"] > stats["pairs_undecided"], stats
    if caps:
        assert stats["evals_undecided"] <= 0.01 * (stats["evals"] + stats["evals_undecided"]), stats
        assert stats["solves"] >= stats["solves_undecided"] and stats["pairs_undecided"] == 0, stats


def _oracle_pair(args):
    w, h, K, H, seed, n_pairs, p = args
    sys.path.insert(0, HERE)
    from oracle_lib import Oracle
    o = Oracle()
    bgr = synth.frames_numpy(seed, n_pairs, w, h)
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    a = o.extract_features(bgr[p], K, ca, sa, pat)
    b = o.extract_features(bgr[n_pairs + p], K, ca, sa, pat)
    s = int(shard.pair_seeds(seed, p, p + 1)[0])
    m = o.match_features(a["xy"], a["desc"], b["xy"], b["desc"], s, H, 10.0)
    return p, a, b, m


@pytest.mark.parametrize("w,h,K,H,P,seed", [(1280, 720, 2000, 4096, 24, 0x50AC0001), (640, 480, 1000, 1024, 24, 0x50AC0002),
                                             (1920, 1080, 4000, 8192, 6, 0x50AC0005)])   # C3, C2 and C5's shape (BASELINE.json configs[4])
def test_many_pairs_bit_exact(ctx, w, h, K, H, P, seed):
    bgr = synth.frames_numpy(seed, P, w, h)
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    seeds = shard.pair_seeds(seed, 0, P)
    out = ctx.frontend_pairs(torch.from_numpy(bgr).cuda(), P, K, ca, sa, torch.from_numpy(pat).cuda(),
                             torch.from_numpy(seeds.view(np.int32)).cuda(), H, 10.0)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    procs = max(1, min(len(os.sched_getaffinity(0)), 12))
    with mp.get_context("spawn").Pool(procs) as pool:
        ref = pool.map(_oracle_pair, [(w, h, K, H, seed, P, p) for p in range(P)])
    for p, a, b, m in ref:
        for f, r in ((p, a), (P + p, b)):
            n = len(r["xy"])
            assert out["n"][f] == n, (p, f)
            assert np.array_equal(out["xy"][f, :n], r["xy"]), (p, f)
            assert np.array_equal(out["desc"][f, :n], r["desc"]), (p, f)
            assert np.array_equal(out["nodes"][f, :n], r["nodes"]), (p, f)
        k = len(m["matches"])
        assert out["best"][p, 3] == k, p
        assert np.array_equal(out["matches"][p, :k], m["matches"]), p
        if m["rc"] == 0:
            assert out["F"][p].tobytes() == m["F"].tobytes(), p
    hold_every_fourth_pair(ctx, out, ref, seeds, K, H, P, "soak %dx%d" % (w, h), caps=False)


def _oracle_pair_frames(args):
    fa, fb, K, H, s, p = args
    sys.path.insert(0, HERE)
    from oracle_lib import Oracle
    o = Oracle()
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    a = o.extract_features(fa, K, ca, sa, pat)
    b = o.extract_features(fb, K, ca, sa, pat)
    return p, a, b, o.match_features(a["xy"], a["desc"], b["xy"], b["desc"], s, H, 10.0)


@pytest.mark.parametrize("w,h,K,H,P,seed", [(1280, 720, 2000, 4096, 16, 0x4A2D0001), (640, 480, 1000, 1024, 16, 0x4A2D0002)])
def test_hard_regime_pairs_bit_exact(ctx, w, h, K, H, P, seed):
    """The harder data regime of SURVEY.md 8(d) (synth.frames_torch_hard: rotation + parallax, sub-pixel resampling,
    40-45 % outlier matches — RANSAC has far fewer inliers to go on, the bail-out bounds of the counting kernel are
    learnt late, and the responses are those of an interpolated image): every output against the oracle on the same
    bytes (the frames are generated on the device and copied back)."""
    bgr = synth.frames_torch_hard(seed, P, w, h, "cuda")
    host = bgr.cpu().numpy()
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    seeds = shard.pair_seeds(seed, 0, P)
    out = ctx.frontend_pairs(bgr, P, K, ca, sa, torch.from_numpy(pat).cuda(), torch.from_numpy(seeds.view(np.int32)).cuda(), H, 10.0)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    procs = max(1, min(len(os.sched_getaffinity(0)), 12))
    with mp.get_context("spawn").Pool(procs) as pool:
        ref = pool.map(_oracle_pair_frames, [(host[p], host[P + p], K, H, int(seeds[p]), p) for p in range(P)])
    outlier_share = []
    for p, a, b, m in ref:
        for f, r in ((p, a), (P + p, b)):
            n = len(r["xy"])
            assert out["n"][f] == n, (p, f)
            assert np.array_equal(out["xy"][f, :n], r["xy"]), (p, f)
            assert np.array_equal(out["desc"][f, :n], r["desc"]), (p, f)
            assert np.array_equal(out["nodes"][f, :n], r["nodes"]), (p, f)
        k = len(m["matches"])
        assert out["best"][p, 3] == k, p
        assert np.array_equal(out["matches"][p, :k], m["matches"]), p
        if m["rc"] == 0:
            assert out["F"][p].tobytes() == m["F"].tobytes(), p
        outlier_share.append(1.0 - k / max(m["prelim"], 1))
    assert np.mean(outlier_share) > 0.25, outlier_share     # the regime really is the harder one
    hold_every_fourth_pair(ctx, out, ref, seeds, K, H, P, "hard regime %dx%d" % (w, h), caps=True)


@pytest.mark.parametrize("w,h,pad,maxc", [(3840, 2160, 0, 5000), (4096, 1200, 4, 3000), (2560, 1440, 0, 8000), (1284, 2200, 0, 2000)])
def test_large_frames_from_bgr_rows(ctx, oracle, w, h, pad, maxc):
    """Frames well beyond the bench shapes (4K: 15 column strips, 24 row segments per frame; a 4096-wide one with padded rows;
    8000 corners) through the whole of extract_features, against the oracle."""
    rng = np.random.default_rng(w + h)
    n = 2
    g = rng.integers(0, 256, (n, h // 8 + 1, w // 8 + 1), dtype=np.uint8)
    g = np.kron(g, np.ones((8, 8), np.uint8))[:, :h, :w]      # a blocky texture: real corners
    bgr = np.clip(g[..., None].astype(np.int64) + rng.integers(-6, 7, (n, h, w, 3)), 0, 255).astype(np.uint8)
    rows = np.zeros((n, h, 3 * w + pad), np.uint8)
    rows[:, :, :3 * w] = bgr.reshape(n, h, 3 * w)
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    out = ctx.extract_features(torch.from_numpy(rows).cuda(), maxc, ca, sa, torch.from_numpy(pat).cuda(), width=w)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for f in range(n):
        r = oracle.extract_features(bgr[f], maxc, ca, sa, pat)
        k = r["n"]
        assert out["n_detected"][f] == r["n_detected"] and out["n"][f] == k, (w, h, f)
        assert np.array_equal(out["xy"][f, :k], r["xy"]) and np.array_equal(out["desc"][f, :k], r["desc"]), (w, h, f)
        assert np.array_equal(out["nodes"][f, :k], r["nodes"]), (w, h, f)


def test_repeated_steps_are_deterministic():
    """The same batch through the whole front-end 400 times on two contexts whose runs overlap on the device: every output of
    every run equals the first run's (tools/determinism_soak.py is the long form).  A race, a stale workspace or a
    timing-dependent pipeline hazard shows up here as a difference in some run; a comparison with the oracle of one run
    would not see it."""
    from vslam_amd import Context
    w, h, K, H, P = 640, 480, 1000, 1024, 32
    dev = torch.device("cuda:0")
    bgr = synth.frames_torch(0x50AC0004, P, w, h, dev)
    ca, sa = synth.keypoint_rotation()
    seeds = torch.from_numpy(shard.pair_seeds(0x50AC0004, 0, P).view(np.int32)).to(dev)
    ctxs = [Context(0, use_torch_stream=False) for _ in range(2)]
    ref = ctxs[0].frontend_pairs(bgr, P, K, ca, sa, None, seeds, H, 10.0)
    ctxs[0].synchronize()
    ref = {k: v.clone() for k, v in ref.items()}
    assert int(ref["best"][:, 1].min()) >= 8          # real models, not an empty batch
    outs = [None, None]
    for i in range(400):
        c = i & 1
        if outs[c] is not None:
            ctxs[c].synchronize()
            for k, v in ref.items():
                assert torch.equal(outs[c][k], v), (i - 2, k)
        outs[c] = ctxs[c].frontend_pairs(bgr, P, K, ca, sa, None, seeds, H, 10.0, out=outs[c])
    for c in range(2):
        ctxs[c].synchronize()
        for k, v in ref.items():
            assert torch.equal(outs[c][k], v), k
