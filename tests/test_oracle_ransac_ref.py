"""The oracle's RANSAC against references that were not written from it: tests/ref64.py (float64, with error bounds) and
tests/ref_int.py (sets, accept rule), both restated from src/RansacFilter.cpp.  The bit-exact GPU tests show that the kernels
equal oracle/vso_ransac.cpp; these show that oracle/vso_ransac.cpp computes what the reference defines -- and, through the
planted errors at the end, that the holds the GPU tests call would notice if it did not."""
import numpy as np
import pytest

import ref64
import ref_int
from ransac_inputs import batch as _batch
from vslam_amd import synth


def _identity_pairs(K, n):
    return np.stack([np.arange(K), np.arange(K)], 1).astype(np.int32)[:n]


def regular_cases(oracle):
    """(name, xy1, xy2, pairs, sets, thr): the inputs of test_fundamental_bit_exact, two rows of
    test_counts_first_path_at_scale (thresholds 3 and 40), test_sum_rule_on_a_plateau_of_tied_hypotheses, and coordinates
    scaled by 4e6 (test_threshold_and_scale_outside_certified_range)."""
    sizes = [300, 8, 9, 600, 150]
    xy1, xy2, pairs, _ = _batch(500, sizes + [5], 600, 1280, 720)
    for b, n in enumerate(sizes):
        yield "fundamental-%d" % n, xy1[b], xy2[b], pairs[b, :n], oracle.ransac_sets(40 + b, n, 192), 10.0
    for K, sizes, Hy, thr in ((2304, [1800, 700], 130, 3.0), (2304, [1200, 2000], 64, 40.0)):
        xy1, xy2, pairs, _ = _batch(900 + Hy, sizes, K, 1280, 720)
        for b, n in enumerate(sizes):
            yield "scale-%d-thr%g" % (n, thr), xy1[b], xy2[b], pairs[b, :n], oracle.ransac_sets(70 + b, n, Hy), thr
    K, Hy = 1500, 512
    for b, n in enumerate((K, K - 100, 1100)):
        a, c, _ = synth.two_view_points(4100 + b, K, 1280, 720, inlier_frac=0.85, noise_px=0.0, integer=False)
        # the first 160 of the GPU test's 512 hypotheses: the oracle's own time on all of them is most of this file's
        yield "plateau-%d" % n, a, c, _identity_pairs(K, n), oracle.ransac_sets(900 + b, n, Hy)[:160], 10.0
    xy1, xy2, pairs, m = _batch(1200, [300, 77], 300, 1280, 720)
    for b in range(2):
        n = int(m[b])
        yield ("coordinates-4e6-%d" % n, xy1[b] * np.float32(4e6), xy2[b] * np.float32(4e6), pairs[b, :n],
               oracle.ransac_sets(5 + b, n, 96), 10.0)


def degenerate_cases(oracle):
    """Collinear, one repeated point, identity on a 4 x 4 grid (test_degenerate_geometry_still_bit_exact), coordinates x 1e-9."""
    K, Hy = 64, 128
    xs = np.arange(K, dtype=np.float32)
    a = np.stack([xs, 2 * xs], 1)
    yield "collinear", a, a.copy(), _identity_pairs(K, K), oracle.ransac_sets(60, K, Hy), 10.0
    a = np.tile(np.float32([100, 50]), (K, 1)); c = np.tile(np.float32([101, 50]), (K, 1))
    yield "repeated", a, c, _identity_pairs(K, K), oracle.ransac_sets(61, K, Hy), 10.0
    a = np.rint(np.random.default_rng(3).uniform(0, 4, size=(K, 2))).astype(np.float32)
    yield "grid-identity", a, a.copy(), _identity_pairs(K, K), oracle.ransac_sets(62, K, Hy), 10.0
    xy1, xy2, pairs, m = _batch(1200, [300, 77], 300, 1280, 720)
    for b in range(2):
        n = int(m[b])
        yield ("coordinates-1e-9-%d" % n, xy1[b] * np.float32(1e-9), xy2[b] * np.float32(1e-9), pairs[b, :n],
               oracle.ransac_sets(5 + b, n, 96), 10.0)


def oracle_out(oracle, a, c, pr, sets, thr):
    """The oracle's find_fundamental in the layout of the device's outputs (all-sums mode)."""
    with np.errstate(all="ignore"):
        r = oracle.find_fundamental(a, c, pr, sets, thr)
    keep = pr[r["mask"] != 0] if r["winner"] >= 0 else pr[:0]
    return dict(hypF=r["hypF"], hyp_count=r["hyp_count"], hyp_sum=r["hyp_sum"], F=r["F"], mask=r["mask"],
                best=np.array([r["winner"], r["count"], int(np.float32(r["sum"]).view(np.uint32)), len(keep)], np.int64),
                matches=keep)


def test_oracle_ransac_is_held_on_regular_inputs(oracle):
    """Every decided solve, count, sum, winner and mask bit of the oracle agrees with the float64 references; the caps: at
    most 1 % of the evaluations undecided, at least half of the solves decided, every pair's winner check held; and the
    calibration of ref64's constants: worst error / bound ratio <= 1 (asserted inside the hold) and > 0.001 (not vacuous)."""
    total = ref64.new_ransac_stats()
    for name, a, c, pr, sets, thr in regular_cases(oracle):
        st = ref64.hold_ransac(a, c, pr, sets, thr, oracle_out(oracle, a, c, pr, sets, thr), "all")
        print(name, ref64.ransac_shares(st))
        assert st["pairs"] == 1, name
        ref64.add_ransac_stats(total, st)
    print("total", ref64.ransac_shares(total))
    assert total["evals_undecided"] <= 0.01 * (total["evals"] + total["evals_undecided"]), total
    assert total["solves"] >= total["solves_undecided"], total
    assert 0.001 < total["worst_F"] <= 1.0 and 0.001 < total["worst_sum"] <= 1.0, total
    assert 4 * total["worst_F"] <= 1.0 and 4 * total["worst_sum"] <= 1.0, total      # the 4x margin of the calibration


def test_oracle_ransac_on_degenerate_inputs_reports_its_shares(oracle):
    """Nothing is promised about how much is decided here; what is decided still has to agree."""
    for name, a, c, pr, sets, thr in degenerate_cases(oracle):
        st = ref64.hold_ransac(a, c, pr, sets, thr, oracle_out(oracle, a, c, pr, sets, thr), "all")
        print(name, ref64.ransac_shares(st))


def test_residual_per_evaluation(oracle):
    """oracle.residual one match at a time is the oracle's e itself: |e - e64| within the evaluation's own bound, on the
    first pair of test_fundamental_bit_exact and at coordinates x 4e6 / x 1e-9."""
    worst = 0.0
    for cases in (regular_cases(oracle), degenerate_cases(oracle)):
        for name, a, c, pr, sets, thr in cases:
            if not name.startswith(("fundamental-300", "coordinates")):
                continue
            hyp = [0, 1, 2]
            F = np.stack([oracle.compute_fundamental(a[pr[sets[h], 0]], c[pr[sets[h], 1]]) for h in hyp])
            r = ref64.residuals(F, a, c, pr, thr, keep=list(range(len(hyp))))
            for k in range(len(hyp)):
                for i in range(0, len(pr), 3):
                    with np.errstate(all="ignore"):
                        m, cnt, e = oracle.residual(a, c, pr[i:i + 1], F[k], thr)
                    if r["decided"][k, i]:
                        assert bool(m[0]) == bool(r["inlier"][k, i]) and cnt == int(m[0]), (name, k, i)
                    if np.isfinite(r["tol"][k, i]) and np.isfinite(e):
                        ratio = abs(float(e) - r["e"][k, i]) / r["tol"][k, i]
                        assert ratio <= 1.0, (name, k, i, float(e), r["e"][k, i], r["tol"][k, i])
                        worst = max(worst, ratio)
    print("worst |e - e64| / bound", worst)
    assert 0.001 < worst <= 0.25


def test_every_decided_evaluation_agrees_with_the_oracles_mask(oracle):
    """oracle.residual's mask for EVERY hypothesis of two regular inputs (300 matches x 192 noisy-integer hypotheses, 1100
    x 160 exact sub-pixel ones) against residuals(keep=all): a count inside [lo, hi] could hide two wrong decisions that
    cancel; this cannot."""
    for name, a, c, pr, sets, thr in regular_cases(oracle):
        if name not in ("fundamental-300", "plateau-1100"):
            continue
        F = np.stack([oracle.compute_fundamental(a[pr[s, 0]], c[pr[s, 1]]) for s in sets])
        r = ref64.residuals(F, a, c, pr, thr, keep=list(range(len(sets))))
        masks = np.stack([oracle.residual(a, c, pr, F[h], thr)[0] for h in range(len(sets))]) != 0
        bad = np.argwhere(r["decided"] & (masks != r["inlier"]))
        assert bad.size == 0, (name, bad[:5])
        assert r["decided"].mean() > 0.99, name


def test_compute_fundamental_against_the_float64_solve(oracle):
    """oracle.compute_fundamental (the public entry, not find_fundamental's copy) on the same sets."""
    for name, a, c, pr, sets, thr in regular_cases(oracle):
        sets = sets[:48]
        ref = ref64.fundamental_8pt(a[pr[sets, 0]], c[pr[sets, 1]])
        F = np.stack([oracle.compute_fundamental(a[pr[s, 0]], c[pr[s, 1]]) for s in sets])
        err = ref64.fundamental_error(F, ref)
        d = ref["decided"]
        assert (err[d] <= ref["tol"][d]).all(), (name, float((err[d] / ref["tol"][d]).max()))
        s = np.linalg.svd(F.reshape(-1, 3, 3).astype(np.float64), compute_uv=False)
        assert (s[d, 2] <= ref["tol"][d] + 4 * ref64.EPS).all(), name      # rank 2 (:99)


@pytest.mark.parametrize("kind", ["regular", "degenerate"])
def test_accept_rule(oracle, kind):
    """find_fundamental's winner / count / sum == the sequential scan of :44-66 on its own per-hypothesis counts and sums,
    the degenerate batch and hundreds of ties (plateau) included."""
    nan_seen = tied = 0
    for name, a, c, pr, sets, thr in (regular_cases if kind == "regular" else degenerate_cases)(oracle):
        with np.errstate(all="ignore"):
            r = oracle.find_fundamental(a, c, pr, sets, thr)
        w, cnt, s = ref_int.accept_rule(r["hyp_count"], r["hyp_sum"])
        assert (w, cnt) == (r["winner"], r["count"]), name
        assert np.float32(s).view(np.uint32) == np.float32(r["sum"]).view(np.uint32), name
        nan_seen += int((~np.isfinite(r["hyp_sum"])).sum())
        tied = max(tied, int((r["hyp_count"] == r["hyp_count"].max()).sum()))
    print(kind, "non-finite sums", nan_seen, "largest tie", tied)      # NaN > x on hand-made sums: test_accept_rule_by_hand
    assert kind == "degenerate" or tied >= 40


def test_accept_rule_by_hand():
    nan = np.float32("nan")
    assert ref_int.accept_rule([0, 0], [0.0, -1.0])[0] == -1                    # nothing beats (0, 0.0f)
    assert ref_int.accept_rule([0, 0], [0.0, 2.0])[0] == 1                      # count 0 wins on a positive sum
    assert ref_int.accept_rule([3, 3, 3], [1.0, 5.0, 5.0])[0] == 1              # the first of equal sums
    assert ref_int.accept_rule([3, 3], [nan, 5.0])[0] == 0                      # 5 > NaN is false
    assert ref_int.accept_rule([3, 3], [5.0, nan])[0] == 0                      # NaN > 5 is false
    assert ref_int.accept_rule([2, 3, 2], [9.0, 1.0, 99.0])[:2] == (1, 3)
    a = np.float32(16777216.0)
    assert ref_int.accept_rule([1, 1], [a, 16777217.0])[0] == 0                 # compared as floats: 2^24 + 1 rounds to 2^24


@pytest.mark.parametrize("seed,n,H,mi", [(1, 8, 40, 8), (0x5EED0001, 37, 200, 8), (12345, 1100, 300, 8), (3, 9, 96, 1),
                                         (77, 5, 96, 5), (0xFFFFFFFF, 4000, 96, 7), (901, 15999, 8192, 8)])
def test_sets(oracle, seed, n, H, mi):
    got = oracle.ransac_sets(seed, n, H, min_items=mi)
    ref_int.hold_sets(seed, n, H, got, mi)
    if H == 8192:       # this stream has exactly one Lemire rejection: without it the plain multiply-shift gives other sets
        raw = np.random.RandomState(seed).randint(0, 2 ** 32, size=H * 8, dtype=np.uint64)
        rng = np.uint64(n) - (np.arange(H * 8, dtype=np.uint64) & np.uint64(7))
        rej = np.nonzero(((raw * rng) & np.uint64(0xFFFFFFFF)) < (np.uint64(2 ** 32) - rng) % rng)[0]
        assert len(rej) == 1
        h = int(rej[0]) // 8                                # every draw after it is shifted by one raw output
        assert got[h + 1, 0] == int((raw[8 * (h + 1) + 1] * np.uint64(n)) >> np.uint64(32))      # first draw of the next set
    assert not got[:, mi:].any() and got.min() >= 0 and got.max() < n
    assert all(len(set(r[:mi])) == mi for r in got.tolist())        # drawn without replacement


# ------------------------------------------------------------------------------------------------------ planted errors
def _sampson(F, a, c, pr, thr):
    F = F.reshape(3, 3).astype(np.float64)
    x1 = np.c_[a[pr[:, 0]].astype(np.float64), np.ones(len(pr))].T
    x2 = np.c_[c[pr[:, 1]].astype(np.float64), np.ones(len(pr))].T
    A = F @ x1; C = F.T @ x2
    n = (x2 * A).sum(0)
    e = n * n / (A[0] ** 2 + A[1] ** 2 + C[0] ** 2 + C[1] ** 2)
    return e <= thr, e


def test_planted_errors_are_caught(oracle):
    """The holds are fed the oracle's outputs with one thing changed at a time; each must raise."""
    name, a, c, pr, sets, thr = next(iter(regular_cases(oracle)))          # 300 matches, 192 hypotheses
    good = oracle_out(oracle, a, c, pr, sets, thr)
    ref64.hold_ransac(a, c, pr, sets, thr, good, "all")                    # unchanged: passes
    w = int(good["best"][0])
    r = ref64.residuals(good["hypF"], a, c, pr, thr, keep=[w])
    sol = ref64.fundamental_8pt(a[pr[sets, 0]], c[pr[sets, 1]])
    tight = int(np.argmin(sol["tol"]))
    assert sol["tol"][tight] < 1e-5
    planted = {}

    def remask(o, mask):
        o["mask"] = mask.astype(np.uint8); o["matches"] = pr[mask]; o["best"] = o["best"].copy(); o["best"][3] = int(mask.sum())

    o = dict(good); m = good["mask"] != 0                                   # 1. one decided mask bit flipped
    i = int(np.nonzero(r["decided"][0])[0][7]); m = m.copy(); m[i] = ~m[i]; remask(o, m)
    planted["mask bit flipped"] = (ref64.hold_ransac, (a, c, pr, sets, thr, o, "all"))

    o = dict(good)                                                          # 2. a winner with a smaller decided count
    h = int(np.nonzero(r["hi"] < r["lo"][w])[0][0])
    mh, ch, sh = oracle.residual(a, c, pr, good["hypF"][h], thr)
    o["best"] = np.array([h, ch, int(np.float32(sh).view(np.uint32)), 0]); o["F"] = good["hypF"][h]; remask(o, mh != 0)
    planted["winner with fewer inliers"] = (ref64.hold_ransac, (a, c, pr, sets, thr, o, "all"))

    o = dict(good); F = good["hypF"].copy()                                 # 3. one F scaled row-wise by 1 + 1e-3
    F[tight, 3:6] *= np.float32(1.001); o["hypF"] = F
    planted["F row scaled by 1 + 1e-3"] = (ref64.fundamental_check, (a, c, pr, sets, o["hypF"]))

    o = dict(good); F = good["hypF"].copy()                                 # 4. F transposed (src/RansacFilter.cpp:119-120)
    F[tight] = F[tight].reshape(3, 3).T.reshape(9); o["hypF"] = F
    planted["F transposed"] = (ref64.fundamental_check, (a, c, pr, sets, o["hypF"]))
    o = dict(good); cnt = good["hyp_count"].copy(); sm = good["hyp_sum"].copy()     # ... and in the residual: F.t() x1, F x2
    for h in range(len(sets)):
        _, cnt[h], sm[h] = oracle.residual(a, c, pr, good["hypF"][h].reshape(3, 3).T.reshape(9).copy(), thr)
    o["hyp_count"], o["hyp_sum"] = cnt, sm
    planted["residual with F and F.t() exchanged"] = (ref64.hold_ransac, (a, c, pr, sets, thr, o, "all", False))

    o = dict(good); cnt = good["hyp_count"].copy()                          # 5. Sampson's grouping of :126
    for h in range(len(sets)):
        cnt[h] = int(_sampson(good["hypF"][h], a, c, pr, thr)[0].sum())
    o["hyp_count"] = cnt
    planted["Sampson's grouping"] = (ref64.hold_ransac, (a, c, pr, sets, thr, o, "all", False))

    d1, d2, _ = synth.descriptors_pair(11, 150, 170)                        # 6. a knn tie resolved to the higher index
    d2[40] = d2[17]
    knn = np.stack(oracle.match_knn2(d1, d2), 1)
    ref_int.hold_match(d1, d2, knn=knn, pairs=oracle.match_knn2_ratio(d1, d2)[0])
    q = np.nonzero((knn[:, 0] == 17) & (knn[:, 2] == 40))[0]
    assert q.size
    bad = knn.copy(); bad[q[0], 0], bad[q[0], 2] = 40, 17
    planted["knn tie to the higher index"] = (ref_int.hold_match, (d1, d2, bad))

    rs = np.random.RandomState(99)                                          # 7. sets drawn with raw % n
    mod = np.zeros((64, 8), np.int32)
    for i in range(64):
        avail = list(range(300))
        for j in range(8):
            k = int(rs.randint(0, 2 ** 32, dtype=np.uint64)) % len(avail)
            mod[i, j] = avail[k]; avail[k] = avail[-1]; avail.pop()
    ref_int.hold_sets(99, 300, 64, oracle.ransac_sets(99, 300, 64))
    planted["sets by raw % n"] = (ref_int.hold_sets, (99, 300, 64, mod))

    caught = []
    for what, (fn, args) in planted.items():
        with pytest.raises(AssertionError):
            fn(*args)
        caught.append(what)
    print("planted errors caught:", caught)
    assert len(caught) == 8          # the seven of the list, the transposition planted in the solve and in the residual
