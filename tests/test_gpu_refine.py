"""vslam_refine_pairs (two-view bundle adjustment of each pair's pose and points, on the device) against tests/ref_refine.py,
and VSLAM_OPT_POSE_REFINE through the pose chain, a pipeline ticket and the tracking loop.

Comparison, per entry: |dev - ref| <= 2^-23 scale + 16 delta_ref scale, scale = 1 for R and t and the array's largest magnitude
for c2 and the points: one f32 rounding on each side, and 16 times the disagreement two correct float64 formulations already
show (ref_refine.delta_ref(), 9.8e-8 as measured on the CPU: tests/test_ref_refine.py; never measured from the device).
d_stats[0] is compared exactly; d_stats[3] (accepted steps) exactly where every decision of the reference run is at least
ref_refine.DECIDED_MARGIN away from a tie (every comparison input is chosen so); d_stats[1] to 1e-9 relative; d_stats[2] to 1e-9
against the reference's expression on the device's own f32 outputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_refine as rr
import ref_refit
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
KD = rr.KMAT.astype(np.float64)


def run(ctx, xy1, xy2, matches, best, R, tt, P, gate_sq=rr.GATE_SQ, iters=rr.MAX_ITERATIONS):
    """Batched numpy inputs -> numpy (R (B, 9), t, c2 (B, 12), points4d, stats)."""
    B = len(best)
    dR, dt, dP = t(np.asarray(R, np.float32).reshape(B, 9)), t(np.asarray(tt, np.float32).reshape(B, 3)), t(np.asarray(P, np.float32))
    out = ctx.refine_pairs(t(xy1), t(xy2), t(matches), t(best), rr.KMAT, dR, dt, dP, gate_sq, iters)
    ctx.synchronize()
    assert out[0] is dR and out[3] is dP                        # in place by design
    return [o.cpu().numpy() for o in out]


def stack(cases):
    return [np.stack([c[i] for c in cases]) for i in range(1, 8)]


def c2_bound(c2, K=KD):
    """c2 is formed from the f64 R and t and rounded once; K [R | t] of the WRITTEN f32 R and t differs by the rounding of c2
    (2^-24 of the largest entry) and by K times the roundings of R and t (entries <= 1: 2^-25 each)."""
    return 2.0 ** -24 * np.abs(c2).max() + np.abs(K).sum(1).max() * 2.0 ** -25


def hold_properties(R, tt, c2, P, st, case, tag, K=KD):
    """What every refined (not left alone) output has.  K: the camera matrix in float64 (the comparison cases' by default)."""
    xy1, xy2, matches, best = case[:4]
    R64, t64 = R.astype(np.float64).reshape(3, 3), tt.astype(np.float64)
    assert np.isfinite(R).all() and np.isfinite(tt).all() and np.isfinite(c2).all(), tag
    assert np.abs(R64.T @ R64 - np.eye(3)).max() <= 2.0 ** -21 and np.linalg.det(R64) > 0, tag
    assert abs(np.sqrt(t64 @ t64) - 1.0) <= 2.0 ** -22, tag
    want = rr.camera(K, R64, t64)
    assert np.abs(c2.astype(np.float64).reshape(3, 4) - want).max() <= c2_bound(c2, K), tag
    if st is not None:                                          # the pose chain passes no stats pointer
        assert st[2] < st[1], (tag, st)
    n = int(best[3])
    m = matches[:n]
    inr = (m >= 0).all(1) & (m < len(xy1)).all(1)
    X = P[:n, :3].astype(np.float64)
    ms = np.where(inr[:, None], m, 0)
    ok, _, _ = rr.participants(K, R64, t64, X, xy1[ms[:, 0]].astype(np.float64), xy2[ms[:, 1]].astype(np.float64), np.inf)
    return ok & inr


def hold_arrays_to_reference(name, dev, ref, case, delta, st=None, K=KD):
    """The array part: R, t, c2 and the participating points within tolerance, every other slot's bits kept.  dev = (R, t, c2,
    points4d); returns the largest err / tol."""
    R, tt, c2, P = dev[:4]
    Rr, tr, c2r, Pr, info = ref
    assert not info["left_alone"] and info["comparable"], name
    part = info["part"]
    front = hold_properties(R, tt, c2, P, st, case, name, K)
    assert front[part].all(), (name, "every participating point has positive depth in both cameras")
    worst = 0.0
    for nm, a, b, scale in (("R", R.reshape(3, 3), Rr, 1.0), ("t", tt, tr, 1.0), ("c2", c2.reshape(3, 4), c2r, np.abs(c2r).max()),
                            ("points", P[:len(part)][part], Pr[:len(part)][part], np.abs(Pr[:len(part)][part]).max())):
        err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max()
        tol = (2.0 ** -23 + 16 * delta) * scale
        worst = max(worst, err / tol)
        print(f"{name} {nm}: max err {err:.3e}, tol {tol:.3e}")
        assert err <= tol, (name, nm)
    rest = np.ones(len(P), bool); rest[:len(part)][part] = False
    assert np.array_equal(bits(P[rest]), bits(case[6][rest])), (name, "slots of matches that do not participate keep their bits")
    return worst


def hold_to_reference(name, dev, ref, case, delta):
    R, tt, c2, P, st = dev
    Rr, tr, c2r, Pr, info = ref
    assert st[0] == info["stats"][0], (name, st, info["stats"])
    worst = hold_arrays_to_reference(name, dev, ref, case, delta, st)
    part = info["part"]
    assert abs(st[1] - info["stats"][1]) <= 1e-9 * info["stats"][1], name
    s2 = rr.mean_error(rr.KMAT, R, tt, P[:len(part)][part, :3], info["o1"][part], info["o2"][part])
    print(f"{name}: stats {st}, ref {info['stats']}, margin {info['margin']:.1e}, worst err / tol {worst:.3f}")
    assert abs(st[2] - s2) <= 1e-9 * s2, name
    if info["margin"] >= rr.DECIDED_MARGIN:
        assert st[3] == info["stats"][3], name


@pytest.fixture(scope="module")
def refs():
    return {c[0]: c for c in rr.comparison_cases()}, rr.comparison_results(), rr.delta_ref()


@pytest.mark.parametrize("K,n", rr.COMPARISON_SHAPES)
def test_refine_matches_reference(ctx, refs, K, n):
    cases, res, delta = refs
    name = f"K{K}_n{n}"
    out = run(ctx, *stack([cases[name]]))
    hold_to_reference(name, [o[0] for o in out], res[name], cases[name][1:], delta)
    if n in (3200, 3201):
        assert n - 2 <= out[4][0, 0] <= n, (name, out[4][0])


def test_refine_mixed_batch_matches_reference(ctx, refs):
    cases, res, delta = refs
    names = [k for k in cases if k.startswith("mixed")]
    assert len(names) == len(rr.MIXED_BATCH[1])
    out = run(ctx, *stack([cases[k] for k in names]))
    for b, name in enumerate(names):
        hold_to_reference(name, [o[b] for o in out], res[name], cases[name][1:], delta)


def test_refine_lds_and_arena_pairs_in_one_launch(ctx, refs):
    """n = 3200 keeps its f64 point state in LDS and n = 3201 in the arena; the choice is per pair inside a launch.  Both sides of
    the seam and a small pair as ONE batch of stride 4096, each held as when it runs alone."""
    cases, res, delta = refs
    K, ns = rr.SEAM_BATCH
    names = [f"K{K}_n{n}" for n in ns]
    out = run(ctx, *stack([cases[k] for k in names]))
    for b, (name, n) in enumerate(zip(names, ns)):
        hold_to_reference(name, [o[b] for o in out], res[name], cases[name][1:], delta)
        assert n - 2 <= out[4][b, 0] <= n, (name, out[4][b])      # what the seeds were chosen for: the pair is full to the seam


def test_left_alone_rules_bit_for_bit(ctx, refs):
    K, n = 64, 64
    base = rr.case(rr.SHAPE_SEEDS[(K, n)], K, n)
    xy1, xy2, matches, best, R, tt, P = [np.stack([a] * 7) for a in base]
    best[0] = [-1, 0, 0, n]                                     # no winner
    best[1] = [0, 7, 0, 7]                                      # 7 participants
    tt[2] = -tt[2]                                              # negated t: the points end up behind camera 2
    P[3, 5, 1] = np.inf                                         # item 3: one non-finite point: excluded, the rest refined
    matches[4, 3, 0] = K; matches[4, 9, 1] = -1                 # item 4: two indices out of range (ignored)
    keep = np.ones(n, bool); keep[[3, 9]] = False               # item 5: the same pair without those two matches
    matches[5, :n - 2] = base[2][:n][keep]; P[5, :n - 2] = base[6][:n][keep]; best[5] = [0, n - 2, 0, n - 2]
    Ro, to, c2, Po, st = run(ctx, xy1, xy2, matches, best, R, tt, P)
    neg = rr.refine(xy1[2], xy2[2], matches[2, :n], rr.KMAT, R[2], tt[2], P[2], kp_stride=K)[4]
    assert neg["left_alone"] and neg["stats"][0] < 8
    for b, cnt in ((0, n), (1, 7), (2, neg["stats"][0])):
        assert np.array_equal(bits(Ro[b]), bits(R[b].reshape(9))) and np.array_equal(bits(to[b]), bits(tt[b])), b
        assert np.array_equal(bits(Po[b]), bits(P[b])), b
        want = rr.camera(KD, R[b].astype(np.float64), tt[b].astype(np.float64)).astype(np.float32)
        assert np.array_equal(bits(c2[b]), bits(want.reshape(12))), (b, "c2 = K [R | t] of the inputs")
        if b:
            assert st[b, 0] == cnt, (b, st[b])
        assert np.isnan(st[b, 1:]).all(), (b, st[b])
    # a gate so small that nothing participates
    out = run(ctx, xy1[6:], xy2[6:], matches[6:], best[6:], R[6:], tt[6:], P[6:], gate_sq=1e-12)
    assert np.array_equal(bits(out[0][0]), bits(R[6].reshape(9))) and np.array_equal(bits(out[3][0]), bits(P[6]))
    assert out[4][0, 0] == 0 and np.isnan(out[4][0, 1:]).all()
    delta = rr.delta_ref()
    for b in (3, 4, 5, 6):
        nb = int(best[b, 3])
        ref = rr.refine(xy1[b], xy2[b], matches[b, :nb], rr.KMAT, R[b], tt[b], P[b], kp_stride=K)
        assert not ref[4]["left_alone"]
        part = hold_properties(Ro[b], to[b], c2[b], Po[b], st[b], (xy1[b], xy2[b], matches[b], best[b]), b)
        assert st[b, 0] == ref[4]["stats"][0], (b, st[b], ref[4]["stats"])
        assert part[ref[4]["part"]].all(), (b, "positive depth in both cameras")
        assert np.abs(Ro[b].reshape(3, 3).astype(np.float64) - ref[0]).max() <= 2.0 ** -23 + 16 * delta, b
        assert np.abs(to[b].astype(np.float64) - ref[1]).max() <= 2.0 ** -23 + 16 * delta, b
    assert st[3, 0] == n - 1 and np.array_equal(bits(Po[3, 5]), bits(P[3, 5])), "the non-finite point keeps its bits"
    assert st[4, 0] == n - 2 and st[5, 0] == n - 2
    assert np.array_equal(bits(Po[4, [3, 9]]), bits(P[4, [3, 9]])), "slots of ignored matches keep their bits"
    # item 4 is item 5's correspondences with two holes among its slots: the same fit, in another summation order
    assert np.abs(Ro[4].astype(np.float64) - Ro[5]).max() <= 2.0 ** -23 + 16 * delta
    assert np.abs(to[4].astype(np.float64) - to[5]).max() <= 2.0 ** -23 + 16 * delta


def test_determinism_across_batch_slots_and_runs(ctx, refs):
    cases, _, _ = refs
    target = cases["K1024_n257"]
    others = [cases[k] for k in cases if k.startswith("mixed")][:6]
    alone = run(ctx, *stack([target]))
    first = run(ctx, *stack([target] + others))
    last = run(ctx, *stack(others + [target]))
    again = run(ctx, *stack(others + [target]))
    for got, slot in ((first, 0), (last, 6), (again, 6)):
        for k in range(4):
            assert np.array_equal(bits(got[k][slot]), bits(alone[k][0])), (slot, k)
        assert np.array_equal(got[4][slot].view(np.uint64), alone[4][0].view(np.uint64)), slot


def test_accuracy_on_held_out_correspondences(ctx):
    """The CPU test's 32 pairs: per pair the same verdict (better or worse held-out RMS Sampson distance of the F implied by
    (R, t)) as the reference, except where the reference's ratio is within 1e-6 of 1."""
    pairs = rr.accuracy_inputs()
    n = len(pairs[0][0])
    best = np.tile(np.array([0, n, 0, n], np.int32), (len(pairs), 1))
    Ro, to, c2, Po, st = run(ctx, *[np.stack([p[i] for p in pairs]) for i in (0, 1, 2)], best, *[np.stack([p[i] for p in pairs]) for i in (3, 4, 5)])
    same = 0
    for k, (p1, p2, m, R, tt, P, h1, h2) in enumerate(pairs):
        before = ref_refit.rms_sampson(rr.F_of(rr.KMAT, R, tt), h1, h2)
        ref = rr.refine(p1, p2, m, rr.KMAT, R, tt, P, rr.GATE_SQ, rr.MAX_ITERATIONS)
        r_ref = ref_refit.rms_sampson(rr.F_of(rr.KMAT, ref[0], ref[1]), h1, h2) / before
        r_dev = ref_refit.rms_sampson(rr.F_of(rr.KMAT, Ro[k].reshape(3, 3), to[k]), h1, h2) / before
        print(f"pair {k}: ratio device {r_dev:.4f} reference {r_ref:.4f}")
        if abs(r_ref - 1.0) > 1e-6:
            assert (r_dev < 1) == (r_ref < 1), k
            same += 1
    assert same >= 30
    assert (st[:, 2] < st[:, 1]).all()


def test_abi_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    z = C.c_void_p(0)
    K = 16
    xy = torch.zeros((1, K, 2), device="cuda"); m = torch.zeros((1, K, 2), dtype=torch.int32, device="cuda")
    best = torch.tensor([[0, 9, 0, 9]], dtype=torch.int32, device="cuda")
    R = torch.full((1, 9), 5.0, device="cuda"); tt = torch.full((1, 3), 6.0, device="cuda")
    c2 = torch.full((1, 12), 7.0, device="cuda"); P = torch.full((1, K, 4), 8.0, device="cuda")
    Kh = np.ascontiguousarray(rr.KMAT.reshape(9))
    p = lambda a: C.c_void_p(a.data_ptr())
    good = [p(xy), p(xy), p(m), p(best), 1, K, Kh.ctypes.data_as(C.c_void_p), C.c_float(16.0), 20, p(R), p(tt), p(c2), p(P), z]
    assert lib.vslam_refine_pairs(C.c_void_p(0), *good) == -1
    for i in (0, 1, 2, 3, 6, 9, 10, 11, 12):                    # every required pointer
        args = list(good); args[i] = z
        assert lib.vslam_refine_pairs(h, *args) == -1, i
    for i, v in ((4, 0), (4, -1), (5, 0), (5, -3), (8, 0), (8, 65), (7, C.c_float(0.0)), (7, C.c_float(-1.0)),
                 (7, C.c_float(float("nan"))), (7, C.c_float(float("inf")))):
        args = list(good); args[i] = v
        assert lib.vslam_refine_pairs(h, *args) == -1, (i, v)
    ctx.synchronize()
    assert (R == 5.0).all() and (tt == 6.0).all() and (c2 == 7.0).all() and (P == 8.0).all()   # nothing was queued
    with pytest.raises(capi.VslamError):
        ctx.set_option(capi.Context.OPT_POSE_REFINE, 2)


# ------------------------------------------------------------------------------------------------ VSLAM_OPT_POSE_REFINE
W, H, MAXC, HYP, THR, P_ = 320, 240, 300, 64, 10.0, 3           # the pose-ticket shape of tests/test_gpu_refit.py
KMAT = np.array([[525.0, 0, W // 2], [0, 525.0, H // 2], [0, 0, 1]], np.float32)


def by_hand_pairs(ctx, frames, seeds):
    ca, sa = synth.keypoint_rotation()
    o = ctx.frontend_pairs(frames, P_, MAXC, ca, sa, None, seeds, HYP, THR)
    xy1, xy2 = o["xy"][:P_].contiguous(), o["xy"][P_:].contiguous()
    o["R"], o["t"], c2 = ctx.extract_Rt(o["F"], o["best"], KMAT)
    o["points4d"] = ctx.triangulate(xy1, xy2, o["matches"], o["best"], KMAT, c2)
    _, _, o["c2"], _, _ = ctx.refine_pairs(xy1, xy2, o["matches"], o["best"], KMAT, o["R"], o["t"], o["points4d"], 16.0, 20)
    ids = torch.full((P_, MAXC), -1, dtype=torch.int32, device="cuda")
    o["inlier_idx"], o["n_inliers"], o["error"] = ctx.reprojection_filter(o["points4d"], xy1, xy2, o["matches"], o["best"], KMAT,
                                                                          o["c2"], ids, 4.0)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def same_pose_outputs(got, ref, tag):
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    b8 = lambda a: np.ascontiguousarray(a).view(np.uint8)
    for k in ("n", "best", "F", "R", "t", "c2", "n_inliers", "error"):
        assert np.array_equal(b8(g[k]), b8(ref[k])), (tag, k)
    for b in range(P_):
        m, ni = int(ref["best"][b, 3]), int(ref["n_inliers"][b])
        assert np.array_equal(g["matches"][b, :m], ref["matches"][b, :m]), (tag, "matches", b)
        if ref["best"][b, 0] >= 0:
            assert np.array_equal(b8(g["points4d"][b, :m]), b8(ref["points4d"][b, :m])), (tag, "points4d", b)
            assert np.array_equal(g["inlier_idx"][b, :ni], ref["inlier_idx"][b, :ni]), (tag, "inlier_idx", b)


def test_option_through_the_pose_chain_and_a_ticket(ctx):
    ca, sa = synth.keypoint_rotation()
    frames = torch.from_numpy(synth.frames_numpy(900, P_, W, H)).cuda()
    seeds = torch.from_numpy(np.arange(P_, dtype=np.int32)).cuda()
    ref = by_hand_pairs(ctx, frames, seeds)
    assert (ref["best"][:, 0] >= 0).any() and int(ref["n_inliers"].sum()) > 0
    off = ctx.frontend_pairs_pose(frames, P_, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)
    ctx.synchronize()
    off = {k: v.cpu().numpy() for k, v in off.items()}
    fresh = capi.Context(0)                                     # option off: what an untouched context gives
    try:
        plain = fresh.frontend_pairs_pose(frames, P_, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)
        fresh.synchronize()
        same_pose_outputs(plain, off, "option off")
    finally:
        fresh.close()
    ctx.set_option(capi.Context.OPT_POSE_REFINE, 1)
    try:
        got = ctx.frontend_pairs_pose(frames, P_, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)
        ctx.synchronize()
    finally:
        ctx.set_option(capi.Context.OPT_POSE_REFINE, 0)
    same_pose_outputs(got, ref, "one call")
    print(f"n_inliers summed over the pairs: option off {int(off['n_inliers'].sum())}, on {int(ref['n_inliers'].sum())}")
    assert not np.array_equal(bits(off["R"]), bits(ref["R"])), "the adjustment should move R"
    again = ctx.frontend_pairs_pose(frames, P_, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)
    ctx.synchronize()
    same_pose_outputs(again, off, "option off again")
    pipe = capi.Pipeline(0, 2)
    try:
        pipe.set_option(capi.Context.OPT_POSE_REFINE, 1)
        out = capi.Pipeline.alloc_pose_outputs(torch, 2 * P_, P_, MAXC, frames.device)
        torch.cuda.synchronize()
        ticket = pipe.submit_pairs_pose(frames, P_, MAXC, ca, sa, None, seeds, HYP, THR, KMAT, out)
        assert pipe.wait_status(ticket)[0] == 0
        same_pose_outputs(out, ref, "ticket")
    finally:
        pipe.close()


def test_option_through_track_sequences(ctx):
    T, FR, KP = 2, 3, 448
    ca, sa = synth.keypoint_rotation()
    bgr = torch.from_numpy(synth.sequences_numpy(2, T, FR, W, H)).cuda()
    seeds = torch.from_numpy((np.arange(T * (FR - 1), dtype=np.int32) * 7919 + 5).reshape(T, FR - 1)).cuda()
    flat_seeds = torch.zeros(T * FR - 1, dtype=torch.int32, device="cuda")
    for tr in range(T):
        flat_seeds[tr * FR: tr * FR + FR - 1] = seeds[tr]
    a = capi.PointMap(ctx, T, FR, KP, 4000, 12000)
    b = capi.PointMap(ctx, T, FR, KP, 4000, 12000)
    c = capi.PointMap(ctx, T, FR, KP, 4000, 12000)
    try:
        ctx.track_sequences(c, bgr, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)      # option off
        ctx.synchronize()
        seq = ctx.frontend_sequence(bgr.view(T * FR, H, W, 3), MAXC, ca, sa, None, flat_seeds, HYP, THR, kp_stride=KP)
        ctx.synchronize()
        ctx.set_option(capi.Context.OPT_POSE_REFINE, 1)
        try:
            ctx.track_sequences(a, bgr, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)

            def frame(f):
                pick = lambda x: x.view(T, FR, *x.shape[1:])[:, f].contiguous()
                return {k: pick(seq[k]) for k in ("xy", "desc", "nodes", "n")}

            def pair(f):
                full = lambda x: torch.cat([x, torch.zeros_like(x[:1])]).view(T, FR, *x.shape[1:])[:, f - 1].contiguous()
                return {k: full(seq[k]) for k in ("matches", "best", "F")}
            b.reset()
            for f in range(1, FR):
                b.step(frame(f - 1), frame(f), pair(f), bgr[:, f].contiguous(), KMAT)
            ctx.synchronize()
        finally:
            ctx.set_option(capi.Context.OPT_POSE_REFINE, 0)
        va, vb, vc = a.view(), b.view(), c.view()
        assert int(va["sizes"].sum()) > 0, "the scenes should triangulate"
        for k in va:
            assert np.array_equal(np.asarray(va[k]), np.asarray(vb[k])), k
        print(f"map sizes: option off {np.asarray(vc['sizes']).tolist()}, on {np.asarray(va['sizes']).tolist()}")
        assert any(not np.array_equal(np.asarray(va[k]), np.asarray(vc[k])) for k in va), "the adjustment should move the map"
    finally:
        a.close(); b.close(); c.close()


# ------------------------------------------------------------------------------------------------ C++ surface
def test_cpp_surfaces_match_the_c_entry_point(ctx, tmp_path):
    """tests/native/refine_demo.cpp: vslam::refine_pairs (device arrays) and optimizer::optimize (the reference's three
    members, host matrices) give the bits of vslam_refine_pairs."""
    import struct
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path / "refine_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "refine_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    n = 64
    xy1, xy2, matches, best, R, tt, P = rr.case(rr.SHAPE_SEEDS[(64, 64)], 64, n)
    a, b = xy1[matches[:n, 0]], xy2[matches[:n, 1]]            # the keypoints in match order: match i = (i, i)
    ident = np.stack([np.arange(n)] * 2, 1).astype(np.int32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", n))
        for x in (rr.KMAT, a, b, R, tt, P[:n]):
            f.write(np.ascontiguousarray(x, np.float32).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    f32 = np.frombuffer(raw[:-32], np.float32)
    st_opt = np.frombuffer(raw[-32:], np.float64)
    assert f32.size == 24 + 4 * n + 12 + 4 * n
    Ro, to, c2, Po, st = run(ctx, a[None], b[None], ident[None], best[None], R[None], tt[None], P[None, :n])
    assert st[0, 3] > 0, "the pair should be refined"
    dev, opt = f32[:24 + 4 * n], f32[24 + 4 * n:]
    for nm, got, want in (("R", dev[:9], Ro[0]), ("t", dev[9:12], to[0]), ("c2", dev[12:24], c2[0]), ("points", dev[24:], Po[0]),
                          ("optimizer R", opt[:9], Ro[0]), ("optimizer t", opt[9:12], to[0]), ("optimizer points", opt[12:], Po[0])):
        assert np.array_equal(bits(got), bits(want).reshape(-1)), nm
    assert np.array_equal(st_opt.view(np.uint64), st[0].view(np.uint64)), "optimizer stats"


def test_the_pose_chain_example_with_refine():
    """examples/pose_chain.py --refine: the option on a pipeline, and per pair of batch 0 the error before and after."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pose_chain.py"), "--refine"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("refine, batch 0 pair")]
    assert len(lines) == 4, r.stdout
    refined = 0
    for ln in lines:
        before, after = (float(x) for x in ln.split("error ")[1].split(" px")[0].split(" -> "))
        if np.isnan(before) and np.isnan(after):                # a pair left alone (extract_Rt's pick may fail the cheirality check)
            continue
        assert np.isfinite(before) and np.isfinite(after) and after <= before, ln
        refined += 1
    assert refined >= 1, r.stdout
