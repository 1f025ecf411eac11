"""CPU checks of the grid ORB/FAST oracle (oracle/vso_orb.cpp) against the definitional reference tests/ref_orb.py: each
stage on its own, then orb_detect and extract_features_grid end to end.  Every bounded quantity prints its largest observed
error / bound ratio (the constants keep a margin of at least 4x)."""
import numpy as np
import pytest

import ref_orb as R
from orb_cases import COUNT_SCENES, blocks, checker, count_scene, fast_bruteforce, noise, photos, search_count_scene
from vslam_amd import synth


def _grays():
    out = [("synth", synth.frames_numpy(8, 1, 320, 240)[0, :, :, 1]),
           ("noise", noise(1, 200, 160)[:, :, 0]),
           ("checker", checker(256, 192, 8)[:, :, 0]),
           ("checker5", checker(333, 250, 5, 40, 220)[:, :, 0]),
           ("flat", np.full((120, 150), 90, np.uint8))]
    out += [("photo%d" % i, np.ascontiguousarray(p[:300, :400, 1])) for i, p in enumerate(photos())]
    return out


# -------------------------------------------------------------------------------------------------- stage by stage
def test_level_sizes_pinned_and_decided(oracle):
    undecided = 0
    for w in list(range(63, 700)) + [1241, 1278, 1280, 1920, 1944, 2052]:
        sizes = [lv.shape[1] for lv in oracle.orb_pyramid(np.zeros((64, w), np.uint8))]
        assert sizes == [s[0] for s in R.level_sizes(w, 64)], w
        for l in range(R.NLEVELS):
            pinned, exact, decided = R.level_size(w, l)
            num, den = w * 5 ** l, 6 ** l
            is_half = (2 * num) % den == 0 and (2 * num // den) % 2 == 1
            # only where w / 1.2^l is exactly x.5 does 1.2f's last bit leave the rounding to the implementation; every
            # other size is the rounded exact quotient
            assert decided or is_half, (w, l)
            if decided:
                assert pinned == exact, (w, l, pinned, exact)
            else:
                undecided += 1
                assert pinned in (num // den, num // den + 1)
    assert undecided > 100
    assert R.level_size(9, 1)[1] is None and R.level_size(9, 1)[0] in (7, 8)
    assert not R.level_size(333, 1)[2]          # the fuzzer's 333-pixel cells: 277.5


@pytest.mark.parametrize("w,l,size", [(324, 3, 187), (756, 3, 437), (1188, 3, 687), (2052, 3, 1187), (1944, 4, 937),
                                      (980, 7, 273)])
def test_level_sizes_from_the_float_scale_factor(oracle, w, l, size):
    """src/Frame.cpp passes scaleFactor = 1.2f, a float: (float)pow((double)1.2f, l) is one ulp above (float)pow(1.2, l) at
    these levels, and w * (1.f / scale) rounds one lower than it would from 1.2."""
    assert R.level_size(w, l)[0] == size == R.level_size(w, l, scale=1.2)[0] - 1
    assert oracle.orb_pyramid(np.zeros((64, w), np.uint8))[l].shape[1] == size
    assert oracle.orb_pyramid(np.zeros((w, 64), np.uint8))[l].shape[0] == size


def test_level_budget(oracle):
    assert R.level_budget() == [109, 90, 75, 63, 52, 44, 36, 31]
    assert list(oracle.orb_level_budget()) == R.level_budget()


def test_pyramid_against_float64_bilinear(oracle):
    worst = 0.0
    for name, g in _grays():
        errs = R.resize_errors(oracle.orb_pyramid(g))
        worst = max(worst, max(errs))
        assert max(errs) <= R.RESIZE_BOUND, (name, errs)
    print(f"pyramid: max |oracle - f64 bilinear| = {worst:.3f}, ratio {worst / R.RESIZE_BOUND:.3f}")
    # a 2:1 ratio has exact coefficients (positions at x.5): the result is the f64 value rounded half up
    src = np.random.default_rng(2).integers(0, 256, (64, 96), dtype=np.uint8)
    assert np.array_equal(oracle.resize_linear_exact(src, 48, 32), np.floor(R.bilinear(src, 48, 32) + 0.5).astype(np.uint8))
    # the check tells a level resized from level 0 from one resized from its predecessor
    levels = oracle.orb_pyramid(noise(4, 320, 240)[:, :, 0])
    for l in range(2, 5):
        alt = np.floor(R.bilinear(levels[0], levels[l].shape[1], levels[l].shape[0]) + 0.5)
        assert np.abs(alt - R.bilinear(levels[l - 1], levels[l].shape[1], levels[l].shape[0])).max() > R.RESIZE_BOUND


def test_fast_levels_match_definition(oracle):
    small = synth.frames_numpy(5, 1, 64, 48)[0, :, :, 1]
    for t in (5, 20):
        x, y, s = R.fast(small, t)
        assert np.array_equal(np.c_[x, y, s].astype(np.float32), fast_bruteforce(small, t))
    for name, g in _grays():
        for lv in oracle.orb_pyramid(g)[:4]:
            best = R.fast_arc_score(lv)
            for t in (5, 20):
                x, y, s = R.fast(lv, t, best)
                assert np.array_equal(np.c_[x, y, s].astype(np.float32), oracle.fast9_16(lv, t)), (name, lv.shape, t)


def test_border_filter():
    x = np.array([30, 31, 32, 68, 69, 31]); y = np.array([40, 40, 40, 40, 40, 30])
    assert list(R.border_mask(x, y, 100, 100)) == [False, True, True, True, False, False]
    assert not R.border_mask(x, y, 62, 100).any() and R.border_mask(np.array([31]), np.array([31]), 63, 63).all()


def test_retain_best_set_rule():
    r = np.array([5, 3, 3, 3, 1, 7])
    keep, dec = R.retain_best(r, 3)
    assert dec and list(keep) == [True, True, True, True, False, True]   # ties at the cut all kept
    keep, dec = R.retain_best(r.astype(float), 3, np.full(6, 0.1))
    assert dec and keep.sum() == 5
    keep, dec = R.retain_best(np.array([5.0, 3.0, 2.95, 1.0]), 2, np.full(4, 0.1), np.arange(4)[:, None])
    assert not dec


def test_umax_disc(oracle):
    u = oracle.orb_umax(R.HALF)
    v = np.arange(R.HALF + 1)
    # the disc's edge lies within one pixel of the circle: across it below 45 degrees, along the radius everywhere
    # (at v = r the digital circle's top is 7 px wide: umax[15] = 3 at radius 15.3)
    low = v <= R.HALF / np.sqrt(2)
    assert np.all(np.abs(u - np.sqrt(R.HALF ** 2 - v ** 2))[low] <= 1), u
    assert np.all(np.abs(np.hypot(u, v) - R.HALF) <= 1), u
    du, dv = R.disc_offsets(u)
    pts = set(zip(du.tolist(), dv.tolist()))
    assert pts == set(zip(dv.tolist(), du.tolist())), "disc not symmetric under u <-> v"
    assert np.array_equal(u, R.umax_reference())


def test_fast_atan2_bound(oracle):
    """fastAtan2 against atan2 over the reachable moment range (|m| <= 255 * sum |u| over the disc)."""
    du, _ = R.disc_offsets(R.umax_reference())
    mmax = 255 * int(np.abs(du).sum())
    rng = np.random.default_rng(7)
    e = 0.0
    for scale in (mmax, 5000, 50):
        y = rng.integers(-scale, scale + 1, 400000); x = rng.integers(-scale, scale + 1, 400000)
        got = oracle.fast_atan2(y.astype(np.float32), x.astype(np.float32))
        assert np.all((got >= 0) & (got <= 360))
        e = max(e, float(R.angle_diff(got, R.angle_deg(y, x)).max()))
    print(f"fastAtan2: max error {e:.5f} deg over |m| <= {mmax}, ratio {e / R.ATAN_BOUND:.3f}")
    assert 4 * e <= R.ATAN_BOUND
    assert oracle.fast_atan2(np.zeros(1), np.zeros(1))[0] == 0


# ---------------------------------------------------------------------------------------------------- orb_detect
def _check_detect(oracle, gray, t, st):
    k = oracle.orb_detect(gray, 500, t)
    ref = R.detect(oracle.orb_pyramid(gray), t)
    lo, hi = ref["count_range"]
    assert lo <= len(k) <= hi, (len(k), lo, hi)
    oc = k[:, 5].astype(int)
    assert np.all(np.diff(oc) >= 0)
    for l, L in enumerate(ref["levels"]):
        kk = k[oc == l]
        sc = R.SCALE ** l
        xl = np.floor(kk[:, 0] / sc + 0.5).astype(np.int64); yl = np.floor(kk[:, 1] / sc + 0.5).astype(np.int64)
        for v, vl in ((kk[:, 0], xl), (kk[:, 1], yl)):
            r = np.abs(v - vl * sc) / (R.C_XY * R.EPS * np.abs(v.astype(np.float64)))
            st["xy"] = max(st["xy"], float(r.max(initial=0)))
            assert np.all(r <= 1), ("pt *= scale", l)
        assert np.allclose(kk[:, 2], 31 * sc, rtol=1e-6)
        cand = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(L["x"], L["y"]))}
        got = list(zip(xl.tolist(), yl.tolist()))
        assert all(p in cand for p in got), ("keypoints outside the candidates", l)
        if L["decided"]:
            want = set((int(a), int(b)) for a, b in zip(L["x"][L["keep"]], L["y"][L["keep"]]))
            assert set(got) == want and len(got) == len(want), ("level set", l, len(got), len(want))
        else:
            st["undecided"] += 1
        idx = np.array([cand[p] for p in got], np.int64)
        if len(idx):
            rr = np.abs(kk[:, 4] - L["resp"][idx]) / L["rb"][idx]
            rr = rr[np.isfinite(rr)]
            st["harris"] = max(st["harris"], float(rr.max(initial=0)))
            assert np.all(rr <= 1), ("Harris response", l)
            d = R.angle_diff(kk[:, 3], L["angle"][idx])
            st["angle"] = max(st["angle"], float(d.max()) / R.ATAN_BOUND)
            assert np.all(d <= R.ATAN_BOUND), ("angle", l)
    return len(k)


def test_orb_detect_against_reference(oracle):
    st = dict(xy=0.0, harris=0.0, angle=0.0, undecided=0)
    for name, g in _grays():
        for t in (20, 5):
            _check_detect(oracle, g, t, st)
    print("orb_detect: ratios xy %.3f harris %.3f angle %.3f, undecided levels %d" % (st["xy"], st["harris"], st["angle"],
                                                                                     st["undecided"]))
    assert st["xy"] <= 0.25 and st["harris"] <= 0.25 and st["angle"] <= 0.25


# --------------------------------------------------------------------------------------------- extract_features_grid
GRID_CASES = [
    ("synth", lambda: synth.frames_numpy(9, 1, 320, 240)[0], 2, 2),
    ("synth_w333", lambda: synth.frames_numpy(11, 1, 333, 250)[0], 1, 1),      # 333 = 3 mod 6: level 1 is 277.5
    ("synth_w645", lambda: synth.frames_numpy(12, 1, 645, 301)[0], 2, 3),      # width off the 4-pixel path, odd cells
    ("synth_w501", lambda: synth.frames_numpy(13, 1, 501, 243)[0], 1, 1),      # 501 = 3 mod 6
    ("noise", lambda: noise(3, 400, 300), 2, 2),
    ("blocks", lambda: blocks(4, 322, 240), 1, 2),
    ("checker8", lambda: checker(320, 240, 8), 1, 1),
    ("checker7", lambda: checker(403, 300, 7, 30, 210), 2, 2),
    ("flat", lambda: np.full((200, 250, 3), 77, np.uint8), 1, 1),
    ("synth_cell324", lambda: synth.frames_numpy(14, 1, 648, 324)[0], 1, 2),   # level 3 of a 324-px cell: 187 from 1.2f
]


def run_grid(oracle, bgr, nrows, ncols, st):
    pat = synth.brief_pattern()
    img, xy, desc, ao = oracle.extract_features_grid(bgr, nrows, ncols, pat)
    ref = R.grid_reference(bgr, nrows, ncols, oracle)
    assert np.array_equal(img, ref["img"]), "outlines"
    for c in ref["cells"]:
        assert max(R.resize_errors(c["levels"])) <= R.RESIZE_BOUND
    R.check_grid(ref, xy, desc, ao, oracle, pat, stats=st)
    assert max(R.resize_errors(ref["flevels"])) <= R.RESIZE_BOUND
    return ref, len(xy)


def report(st, tag):
    print(f"{tag}: {st['points']} keypoints, ratios xy {st['xy']:.3f} angle {st['angle']:.3f}; undecided: "
          f"{st['undecided_cells']} cells, {st['undecided_levels']} levels, {st['undecided_rows']} rows, "
          f"{st['undecided_bits']} of {st['bits']} bits")
    assert st["xy"] <= 0.25 and st["angle"] <= 0.25
    # only descriptor rows and bits may sit on a boundary; every cell's detector choice and every level's set is decided
    assert st["undecided_cells"] == 0 and st["undecided_levels"] == 0
    assert st["undecided_rows"] <= 0.2 * max(st["points"], 1)
    assert st["undecided_bits"] <= 0.01 * max(st["bits"], 1)


@pytest.mark.parametrize("name,make,nrows,ncols", GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_grid_against_reference(oracle, name, make, nrows, ncols):
    st = R.new_stats()
    ref, n = run_grid(oracle, make(), nrows, ncols, st)
    assert (n == 0) == (name == "flat"), n
    report(st, name)


@pytest.mark.parametrize("target", [499, 500, 501])
def test_grid_fallback_at_the_count_boundary(oracle, target):
    """src/Frame.cpp:34: the threshold-5 detector replaces a threshold-20 result of fewer than 500 keypoints, counted after
    its own ties: 499 falls back, 500 and 501 do not."""
    st = R.new_stats()
    ref, n = run_grid(oracle, count_scene(target), 1, 1, st)
    c = ref["cells"][0]
    assert c["decided"] and c["fallback"] == (target < 500)
    if target >= 500:
        assert c["res"]["count_range"] == (target, target) and n == target
    else:
        assert R.detect(c["levels"], 20)["count_range"] == (499, 499)
    report(st, f"count {target}")


def test_count_scenes_are_the_search_results(oracle):
    for target, found in COUNT_SCENES.items():
        assert search_count_scene(oracle, target) == found, target


def test_grid_photographs_against_reference(oracle):
    st = R.new_stats()
    for p in photos():
        run_grid(oracle, p, 2, 2, st)
        run_grid(oracle, np.ascontiguousarray(p[:333, :501]), 1, 1, st)
    report(st, "photographs")
