"""vslam_refit_fundamental (the RANSAC winner refitted over all its inliers, on the device) against tests/ref_refit.py, and
VSLAM_OPT_POSE_REFIT through the pose chain, a pipeline ticket and the tracking loop.

Comparison: per entry |F_dev - F_ref| <= 2^-23 |F_ref| + 16 delta_ref -- the two final f32 roundings, and the float64
disagreement two correct formulations already show (ref_refit.delta_ref(), 3.6e-12 as measured: tests/test_ref_refit.py) with a
margin for a third.  d_stats[1] (mean true Sampson distance under F_in) is held to 1e-9 relative against the reference's value;
d_stats[2] is the same quantity under F_out AS WRITTEN, so it is held to 1e-9 against the reference's Sampson expression
evaluated on the device's own nine f32 words (F_dev and F_ref may differ by one f32 rounding, which moves that mean by far more
than 1e-9).  The inputs are noisy on purpose: on exact correspondences the residual e = x2^t F x1 cancels to its last bits and no
two float64 evaluations of its square agree to 1e-9."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import ref_refit
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ctx, xy1, xy2, matches, best, F_in, alias=False):
    """Batched numpy inputs -> (F_out (B, 9) f32, stats (B, 4) f64)."""
    dF = t(np.asarray(F_in, np.float32).reshape(len(best), 9))
    out, st = ctx.refit_fundamental(t(xy1), t(xy2), t(matches), t(best), dF, out=dF if alias else None)
    ctx.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def stack(cases):
    return [np.stack([c[i] for c in cases]) for i in (1, 2, 3, 4, 5)]


def hold_properties(F_out, F_in, tag):
    """What every output that was not left alone has, whatever the geometry."""
    F = F_out.astype(np.float64).reshape(3, 3)
    assert np.isfinite(F).all(), tag
    assert abs(np.sqrt((F * F).sum()) - 1.0) <= 2.0 ** -22, tag
    assert np.linalg.svd(F, compute_uv=False)[2] <= 2.0 ** -22, tag
    assert (F * F_in.astype(np.float64).reshape(3, 3)).sum() >= 0, tag


def hold_F_to_reference(name, F_dev, ref, F_in, delta):
    """The F part (the pose chain passes no stats pointer): the properties always, the entries where the reference is
    comparable.  Returns whether the entries were compared."""
    F_ref, rs = ref
    hold_properties(F_dev, F_in, name)
    if not rs["comparable"]:
        print(f"{name}: gap {rs['gap']:.2e} below the bound: properties only")
        return False
    err = np.abs(F_dev.astype(np.float64).reshape(3, 3) - F_ref.astype(np.float64))
    tol = 2.0 ** -23 * np.abs(F_ref.astype(np.float64)) + 16 * delta
    print(f"{name}: max err {err.max():.3e} (worst err / tol {(err / tol).max():.3f})")
    assert (err <= tol).all(), name
    return True


def hold_to_reference(name, F_dev, st_dev, ref, F_in, delta):
    F_ref, rs = ref
    compared = hold_F_to_reference(name, F_dev, ref, F_in, delta)
    assert st_dev[0] == rs["stats"][0], name
    if not compared:
        return
    s2 = ref_refit.sampson(F_dev.astype(np.float64), rs["p1"], rs["p2"]).mean()
    print(f"{name}: stats {st_dev}, ref {rs['stats']}, sampson(F_dev) {s2!r}")
    assert abs(st_dev[1] - rs["stats"][1]) <= 1e-9 * rs["stats"][1], name
    assert abs(st_dev[2] - s2) <= 1e-9 * s2, name
    # lambda_9 is known to eps * lambda_1, lambda_8 >= 1e-6 lambda_1 for a comparable case: the ratio to about 64 eps / 1e-6
    assert abs(st_dev[3] - rs["stats"][3]) <= 1e-7, name


@pytest.fixture(scope="module")
def refs():
    cases = {c[0]: c for c in ref_refit.comparison_cases()}
    return cases, ref_refit.comparison_results(), ref_refit.delta_ref()


@pytest.mark.parametrize("K,n", ref_refit.COMPARISON_SHAPES)
def test_refit_matches_reference(ctx, refs, K, n):
    cases, res, delta = refs
    name = f"K{K}_n{n}"
    F, st = run(ctx, *stack([cases[name]]))
    assert res[name][1]["comparable"], "every named shape is a comparison"
    hold_to_reference(name, F[0], st[0], res[name], cases[name][5], delta)


def test_refit_mixed_batch_matches_reference(ctx, refs):
    cases, res, delta = refs
    names = [k for k in cases if k.startswith("mixed")]
    assert len(names) == len(ref_refit.MIXED_BATCH[1])
    F, st = run(ctx, *stack([cases[k] for k in names]))
    for b, name in enumerate(names):
        hold_to_reference(name, F[b], st[b], res[name], cases[name][5], delta)


def test_skip_rules_alias_and_out_of_range(ctx):
    K = 64
    base = ref_refit.case(11, K, 40)
    xy1, xy2, matches, best, F_in = [np.stack([a] * 6) for a in base]
    best[0] = [-1, 0, 0, 40]                                   # no winner
    best[1] = [0, 7, 0, 7]                                     # n = 7
    matches[2, :12] = matches[2, 0]; best[2] = [0, 12, 0, 12]  # all matches on one point: d == 0 in both images
    # item 3: as it is.  item 4: two indices out of range (ignored, not counted).  item 5: the same without those two matches
    matches[4, 3, 0] = K; matches[4, 7, 1] = -1
    keep = np.ones(40, bool); keep[[3, 7]] = False
    matches[5, :38] = base[2][:40][keep]; best[5] = [0, 38, 0, 38]
    F_in[3:] = F_in[3:] * np.float32(-3.0)                     # any scale and sign of F_in: the output is unit and follows the sign
    F, st = run(ctx, xy1, xy2, matches, best, F_in)
    for b, cnt in ((0, 40), (1, 7), (2, 12)):
        assert np.array_equal(bits(F[b]), bits(F_in[b])), b
        assert st[b, 0] == cnt and np.isnan(st[b, 1:]).all(), (b, st[b])
    delta = ref_refit.delta_ref()
    for b in (3, 4, 5):
        n = int(best[b, 3])
        Fr, rs = ref_refit.refit(xy1[b], xy2[b], matches[b, :n], F_in[b], kp_stride=K)
        hold_to_reference(f"item {b}", F[b], st[b], (Fr, rs), F_in[b], delta)
    # item 4 is item 5's 38 correspondences with two holes among its 40 slots: the same fit (both are held to one reference
    # above), though not the same summation order -- the bits are a function of the slots walked, which differ
    assert st[4, 0] == 38 and st[5, 0] == 38
    assert np.abs(F[4].astype(np.float64) - F[5]).max() <= 2.0 ** -23 * np.abs(F[5]).max()
    # d_F_out = d_F_in gives the same bits
    Fa, sta = run(ctx, xy1, xy2, matches, best, F_in, alias=True)
    assert np.array_equal(bits(Fa), bits(F)) and np.array_equal(sta.view(np.uint64), st.view(np.uint64))


def test_properties_on_degenerate_geometry(ctx):
    """Collinear points in both images (the null space of A has more than one dimension), all points on a grid of four spots,
    coordinates of 1e6, and the noise-free scene: whatever comes out is finite, unit, rank 2 and on F_in's side -- or F_in."""
    K, n = 64, 48
    rng = np.random.default_rng(3)
    xy1 = np.zeros((4, K, 2), np.float32); xy2 = np.zeros((4, K, 2), np.float32)
    s = rng.uniform(0, 600, K)
    xy1[0] = np.c_[s, 0.5 * s + 20]; xy2[0] = np.c_[s + 3, 0.5 * s + 21]
    xy1[1] = np.c_[rng.integers(0, 2, K) * 100.0, rng.integers(0, 2, K) * 50.0]; xy2[1] = xy1[1] + 2
    p1, p2, _, _, _ = ref_refit.two_view(77, K, 0, sigma=0.0)
    xy1[2], xy2[2] = p1 * 2000, p2 * 2000
    xy1[3], xy2[3] = p1, p2
    matches = np.stack([np.stack([np.arange(K)] * 2, 1)] * 4).astype(np.int32)
    best = np.tile(np.array([0, n, 0, n], np.int32), (4, 1))
    F_in = rng.normal(size=(4, 9)).astype(np.float32)
    F, st = run(ctx, xy1, xy2, matches, best, F_in)
    for b in range(4):
        if np.array_equal(bits(F[b]), bits(F_in[b])):
            assert np.isnan(st[b, 1:]).all(), b           # left alone
            continue
        hold_properties(F[b], F_in[b], b)
        assert st[b, 0] == n
    assert not np.array_equal(bits(F[3]), bits(F_in[3])), "the regular scene is refitted"


def test_determinism_across_batch_slots_and_runs(ctx, refs):
    cases, _, _ = refs
    target = cases["K1024_n257"]
    others = [cases[k] for k in cases if k.startswith("mixed")][:6]
    alone, st_alone = run(ctx, *stack([target]))
    first, st_first = run(ctx, *stack([target] + others))
    last, st_last = run(ctx, *stack(others + [target]))
    again, st_again = run(ctx, *stack(others + [target]))
    for F, st, slot in ((first, st_first, 0), (last, st_last, 6), (again, st_again, 6)):
        assert np.array_equal(bits(F[slot]), bits(alone[0])), slot
        assert np.array_equal(st[slot].view(np.uint64), st_alone[0].view(np.uint64)), slot


def test_accuracy_on_held_out_correspondences(ctx):
    """The CPU test's 32 pairs: the device refit has the lower held-out RMS Sampson distance in at least 28."""
    pairs = ref_refit.accuracy_pairs()
    n = len(pairs[0][0])
    xy1 = np.stack([p[0] for p in pairs]); xy2 = np.stack([p[1] for p in pairs])
    matches = np.stack([np.stack([np.arange(n)] * 2, 1)] * len(pairs)).astype(np.int32)
    best = np.tile(np.array([0, n, 0, n], np.int32), (len(pairs), 1))
    F_in = np.stack([p[4].reshape(9) for p in pairs])
    F, st = run(ctx, xy1, xy2, matches, best, F_in)
    ratios = np.array([ref_refit.rms_sampson(F[k], p[2], p[3]) / ref_refit.rms_sampson(p[4], p[2], p[3]) for k, p in enumerate(pairs)])
    print(f"better in {(ratios < 1).sum()} of {len(ratios)}, median ratio {np.median(ratios):.3f}, worst {ratios.max():.3f}")
    assert (ratios < 1).sum() >= 28
    assert (st[:, 2] < st[:, 1]).sum() >= 28       # and on the inliers themselves, by its own statistics


def test_abi_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    z = C.c_void_p(0)
    K = 16
    xy = torch.zeros((1, K, 2), device="cuda"); m = torch.zeros((1, K, 2), dtype=torch.int32, device="cuda")
    best = torch.tensor([[0, 9, 0, 9]], dtype=torch.int32, device="cuda")
    F = torch.full((1, 9), 5.0, device="cuda"); out = torch.full((1, 9), 6.0, device="cuda")
    p = lambda a: C.c_void_p(a.data_ptr())
    good = [p(xy), p(xy), p(m), p(best), 1, K, p(F), p(out), z]
    assert lib.vslam_refit_fundamental(C.c_void_p(0), *good) == -1
    for i in (0, 1, 2, 3, 6, 7):                                # every required pointer
        args = list(good); args[i] = z
        assert lib.vslam_refit_fundamental(h, *args) == -1, i
    for i, v in ((4, 0), (4, -1), (5, 0), (5, -3)):
        args = list(good); args[i] = v
        assert lib.vslam_refit_fundamental(h, *args) == -1, (i, v)
    ctx.synchronize()
    assert (out == 6.0).all() and (F == 5.0).all()              # nothing was queued
    with pytest.raises(capi.VslamError):
        ctx.set_option(capi.Context.OPT_POSE_REFIT, 2)


# ------------------------------------------------------------------------------------------------ VSLAM_OPT_POSE_REFIT
W, H, MAXC, HYP, THR, P = 320, 240, 300, 64, 10.0, 3            # the pose-ticket shape of tests/test_gpu_pipeline.py
KMAT = np.array([[525.0, 0, W // 2], [0, 525.0, H // 2], [0, 0, 1]], np.float32)


def by_hand_pairs(ctx, frames, seeds):
    ca, sa = synth.keypoint_rotation()
    o = ctx.frontend_pairs(frames, P, MAXC, ca, sa, None, seeds, HYP, THR)
    half = P
    xy1, xy2 = o["xy"][:half].contiguous(), o["xy"][half:].contiguous()
    o["F"], _ = ctx.refit_fundamental(xy1, xy2, o["matches"], o["best"], o["F"])
    o["R"], o["t"], o["c2"] = ctx.extract_Rt(o["F"], o["best"], KMAT)
    o["points4d"] = ctx.triangulate(xy1, xy2, o["matches"], o["best"], KMAT, o["c2"])
    ids = torch.full((P, MAXC), -1, dtype=torch.int32, device="cuda")
    o["inlier_idx"], o["n_inliers"], o["error"] = ctx.reprojection_filter(o["points4d"], xy1, xy2, o["matches"], o["best"], KMAT,
                                                                          o["c2"], ids, 4.0)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def same_pose_outputs(got, ref, tag):
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    b8 = lambda a: np.ascontiguousarray(a).view(np.uint8)
    for k in ("n", "best", "F", "R", "t", "c2", "n_inliers", "error"):
        assert np.array_equal(b8(g[k]), b8(ref[k])), (tag, k)
    for f in range(2 * P):
        n = int(ref["n"][f])
        for k in ("xy", "desc", "nodes"):
            assert np.array_equal(b8(g[k][f, :n]), b8(ref[k][f, :n])), (tag, k, f)
    for b in range(P):
        m, ni = int(ref["best"][b, 3]), int(ref["n_inliers"][b])
        assert np.array_equal(g["matches"][b, :m], ref["matches"][b, :m]), (tag, "matches", b)
        if ref["best"][b, 0] >= 0:
            assert np.array_equal(b8(g["points4d"][b, :m]), b8(ref["points4d"][b, :m])), (tag, "points4d", b)
            assert np.array_equal(g["inlier_idx"][b, :ni], ref["inlier_idx"][b, :ni]), (tag, "inlier_idx", b)


def test_option_through_the_pose_chain_and_a_ticket(ctx):
    ca, sa = synth.keypoint_rotation()
    frames = torch.from_numpy(synth.frames_numpy(900, P, W, H)).cuda()
    seeds = torch.from_numpy(np.arange(P, dtype=np.int32)).cuda()
    ref = by_hand_pairs(ctx, frames, seeds)
    assert (ref["best"][:, 0] >= 0).any() and int(ref["n_inliers"].sum()) > 0
    plain = ctx.frontend_pairs(frames, P, MAXC, ca, sa, None, seeds, HYP, THR)
    ctx.synchronize()
    assert not np.array_equal(bits(plain["F"].cpu().numpy()), bits(ref["F"])), "the refit should move F"
    ctx.set_option(capi.Context.OPT_POSE_REFIT, 1)
    try:
        got = ctx.frontend_pairs_pose(frames, P, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)
        ctx.synchronize()
    finally:
        ctx.set_option(capi.Context.OPT_POSE_REFIT, 0)
    same_pose_outputs(got, ref, "one call")
    pipe = capi.Pipeline(0, 2)
    try:
        pipe.set_option(capi.Context.OPT_POSE_REFIT, 1)
        out = capi.Pipeline.alloc_pose_outputs(torch, 2 * P, P, MAXC, frames.device)
        rec = torch.zeros((P, 13 + MAXC), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ticket = pipe.submit_pairs_pose(frames, P, MAXC, ca, sa, None, seeds, HYP, THR, KMAT, out, records=rec)
        assert pipe.wait_status(ticket)[0] == 0
        same_pose_outputs(out, ref, "ticket")
        assert np.array_equal(rec.cpu().numpy()[:, :9].view(np.uint32), bits(ref["F"]))   # the records carry the refitted F
    finally:
        pipe.close()


def test_option_through_track_sequences(ctx):
    T, FR, KP = 2, 3, 448
    ca, sa = synth.keypoint_rotation()
    bgr = torch.from_numpy(synth.sequences_numpy(2, T, FR, W, H)).cuda()
    seeds = torch.from_numpy((np.arange(T * (FR - 1), dtype=np.int32) * 7919 + 5).reshape(T, FR - 1)).cuda()
    flat_seeds = torch.zeros(T * FR - 1, dtype=torch.int32, device="cuda")     # pair (t, f) at t * FR + f; the straddling pairs get 0
    for tr in range(T):
        flat_seeds[tr * FR: tr * FR + FR - 1] = seeds[tr]
    a = capi.PointMap(ctx, T, FR, KP, 4000, 12000)
    b = capi.PointMap(ctx, T, FR, KP, 4000, 12000)
    try:
        ctx.set_option(capi.Context.OPT_POSE_REFIT, 1)
        try:
            out = ctx.track_sequences(a, bgr, MAXC, ca, sa, None, seeds, HYP, THR, KMAT)
            ctx.synchronize()
        finally:
            ctx.set_option(capi.Context.OPT_POSE_REFIT, 0)
        # by hand: the flattened front end, the refit over all its pairs, then the map steps
        seq = ctx.frontend_sequence(bgr.view(T * FR, H, W, 3), MAXC, ca, sa, None, flat_seeds, HYP, THR, kp_stride=KP)
        plain_F = seq["F"].clone()
        seq["F"], _ = ctx.refit_fundamental(seq["xy"][:-1].contiguous(), seq["xy"][1:].contiguous(), seq["matches"], seq["best"], seq["F"])
        ctx.synchronize()
        own = [tr * FR + f for tr in range(T) for f in range(FR - 1)]            # the pairs inside a track
        for k in ("matches", "best", "F"):
            assert np.array_equal(out[k].cpu().numpy()[own].view(np.uint8), seq[k].cpu().numpy()[own].view(np.uint8)), k
        assert not torch.equal(plain_F[own], seq["F"][own]), "the refit should move F"

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
        va, vb = a.view(), b.view()
        assert int(va["sizes"].sum()) > 0, "the scenes should triangulate"
        for k in va:
            assert np.array_equal(np.asarray(va[k]), np.asarray(vb[k])), k
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ C++ surface
def test_cpp_surface_matches_the_c_entry_point(ctx, tmp_path):
    """tests/native/refit_demo.cpp: RansacFilter::refit_fundamental (host vectors in, F refitted in place over the flagged
    matches) and vslam::refit_fundamental (device arrays) give the bits of vslam_refit_fundamental."""
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path / "refit_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "refit_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    K, n = 96, 60
    xy1, xy2, matches, best, F_in = ref_refit.case(31, K, n)
    flags = np.ones(n, np.uint8); flags[::5] = 0                 # the matches RANSAC did not keep
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("2i", K, n))
        f.write(xy1.tobytes()); f.write(xy2.tobytes()); f.write(matches[:n].tobytes()); f.write(flags.tobytes()); f.write(F_in.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    got = np.fromfile(fout, np.float32)
    assert got.size == 18
    kept = matches[:n][flags != 0]
    m = np.full((1, K, 2), -1, np.int32); m[0, :len(kept)] = kept
    F, st = run(ctx, xy1[None], xy2[None], m, np.array([[0, len(kept), 0, len(kept)]], np.int32), F_in[None])
    assert not np.array_equal(bits(F[0]), bits(F_in))
    assert np.array_equal(bits(got[:9]), bits(F[0])), "RansacFilter::refit_fundamental"
    assert np.array_equal(bits(got[9:]), bits(F[0])), "vslam::refit_fundamental"


def test_the_pose_chain_example_with_refit():
    """examples/pose_chain.py --refit: the option on a pipeline, and the stage's statistics per pair."""
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pose_chain.py"), "--refit"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert sum(ln.startswith("batch ") for ln in lines) == 12, r.stdout
    refit = [ln for ln in lines if ln.startswith("refit, batch 0 pair")]
    assert len(refit) == 4, r.stdout
    before_after = [tuple(float(x) for x in ln.split("distance ")[1].split(" px")[0].split(" -> ")) for ln in refit]
    assert all(np.isfinite(v) and v >= 0 for ba in before_after for v in ba), r.stdout
