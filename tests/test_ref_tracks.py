"""tests/ref_tracks.py, the numpy restatement of include/vslam_tracks.h, held to what it alone has to meet (no GPU): the hand cases of
tests/tracks_cases.py, whose expected values are derived by hand there; the accuracy of the rule itself on exact scenes under their
true cameras.  The device is held to this reference bit for bit (tests/test_gpu_tracks.py), so the accuracy read here is the device's."""
import numpy as np
import pytest

import ref_adjust as ra
import ref_tracks as rt
import tracks_cases as tc


@pytest.mark.parametrize("variant", list(tc.HAND_VARIANTS))
def test_hand_cases(variant):
    """two rays that meet exactly; parallel rays; one usable observation; one ray several times over (LOW_PARALLAX by the order of the
    rules, DEGENERATE once the parallax test lets everything through); lines that meet behind both cameras; five observations with one
    far off (OK with four good ones, UNSUPPORTED when all must be good); the true point as input against the linear start of a
    problem with an outlier (WORSE), and against the refined result (OK); a NaN input row; rows past n."""
    c = tc.hand_cases()[variant]
    got = tc.reference(c)
    tc.check_hand(variant, got)
    behind = got["X"][list(got["live"]).index(tc.S["behind"])]
    assert np.abs(behind - (0.5, 0.0, -1.0)).max() < 1e-12, "the lines of `behind` meet at (0.5, 0, -1)"
    assert got["status"][tc.S["past_n"]] == rt.NO_PART and got["counts"][tc.S["past_n"]].tolist() == [0, 0]


def test_statuses_of_every_kind_occur_over_the_variants():
    seen = set()
    for c in tc.hand_cases().values():
        seen |= set(tc.reference(c)["status"].tolist())
    assert seen == {-1, 0, 1, 2, 3, 4, 5, 6}


def test_kinv_and_parameter_rules():
    K = tc.HAND_K.astype(np.float64).reshape(9)
    assert rt.kinv(K).tolist() == [2.0 ** -9, 0, -0.5, 0, 2.0 ** -9, -0.375, 0, 0, 1]
    Ks = K.copy()
    Ks[6:] = Ks[:3]
    assert rt.kinv(Ks) is None and rt.kinv(np.zeros(9)) is None
    assert rt.params_ok(rt.params()) and rt.params_ok(rt.params(cos_parallax_max=1.0, iterations=0, good10=0))
    for bad in (dict(cos_parallax_max=-1.0), dict(cos_parallax_max=np.nan), dict(huber_px=0.0), dict(inlier_px=np.inf), dict(iterations=65),
                dict(iterations=-1), dict(min_good=1), dict(good10=11)):
        assert not rt.params_ok(rt.params(**bad)), bad


def test_a_point_depends_on_itself_alone():
    """an item's rows in another order, among other rows and at another pt_stride give each point the same bits"""
    c = rt.random_track_item(11, 200, 6)
    whole = tc.reference(c)
    pick = np.random.default_rng(1).permutation(200)[:50]
    lens = np.diff(c["offsets"])[pick]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.arange(c["offsets"][i], c["offsets"][i + 1]) for i in pick]).astype(np.int64)
    sub = dict(c, points=c["points"][pick], n=50, offsets=off, cam=c["cam"][idx] if len(idx) else c["cam"][:1], kp=c["kp"][idx] if len(idx) else c["kp"][:1])
    part = tc.reference(sub)
    for k in ("out_points", "status", "counts", "info"):
        assert np.array_equal(np.ascontiguousarray(part[k]).view(np.uint8), np.ascontiguousarray(whole[k][pick]).view(np.uint8)), k
    assert {rt.OK, rt.TOO_FEW} <= set(part["status"].tolist())


@pytest.mark.parametrize("seed", ra.EXACT_SEEDS)
def test_exact_scenes_come_back(seed):
    """(a) true cameras, exact projections rounded to f32: every point OK, and within 4 x the worst error measured over the seeds
    (tools/tracks_cpu.py; ref_tracks.EXACT_WORST).  The error is the f32 rounding of the keypoints amplified by depth over baseline."""
    st, d = rt.distances(rt.from_problem(ra.problem(seed, **ra.EXACT_SHAPE, noise_px=0)))
    print(f"seed {seed}: worst |X - X_true| {d.max():.3e} (measured {rt.EXACT_WORST[seed]:.3e}, bound {rt.EXACT_BOUND:.3e})")
    assert (st == rt.OK).all()
    assert d.max() <= rt.EXACT_BOUND


@pytest.mark.parametrize("seed", ra.EXACT_SEEDS)
def test_six_views_beat_two_under_noise(seed):
    """(b) 0.5 px of keypoint noise: the median distance to truth of the six-view rows is below that of the two-view rows (c, c + 1) of
    tools/fuse_adjust_cpu.py's construction, both triangulated by this same rule."""
    pr = ra.problem(seed, **ra.EXACT_SHAPE, noise_px=0.5)
    st6, d6 = rt.distances(rt.from_problem(pr))
    st2, d2 = rt.distances(rt.from_problem(pr, two_view=True))
    m6, m2 = float(np.nanmedian(d6)), float(np.nanmedian(d2))
    print(f"seed {seed}: median |X - X_true| six views {m6:.5f}, two views {m2:.5f} (measured {rt.NOISY_MEDIANS[seed]})")
    assert (st6 == rt.OK).all() and np.isfinite(d2).sum() >= 0.9 * len(d2)
    assert m6 < m2
