"""tests/ref_resect.py, the numpy statement of the resection (include/vslam_resect.h), held to ground truth: exact scenes whose
lifted points and camera centres must come back within C_BOUND * 2^-23 * frames * max|X| although every pair after the first
arrives with R turned by 1 degree and t by 8 -- without and with 20 % of the links' keypoints replaced by random pixels --, the
plain world missing that bound on the same inputs, hand cases for every rule of the text, planted errors that these checks
must catch, and the second formulation (scipy, Huber loss) that delta_ref is measured from.  No GPU: this pins the reference
the device is held to (tests/test_gpu_resect.py)."""
import numpy as np
import pytest

import ref_resect as rr
import ref_world as rw


@pytest.fixture(scope="module")
def scenes():
    return {(seed, o): rr.scene_inputs(seed, outliers=o) for seed in rr.SCENE_SEEDS for o in (0.0, 0.2)}


@pytest.mark.parametrize("seed", rr.SCENE_SEEDS)
def test_exact_scenes_within_the_bound_and_the_plain_world_outside(scenes, seed):
    sc = scenes[(seed, 0.0)]
    assert sc["n"] == 60 and sc["frames"] == 8
    w, worst, unit = rr.run_scene(sc)
    _, plain, _ = rr.run_scene(sc, plain=True)
    print(f"seed {seed}: worst {worst:.3e}, unit {unit:.3e}, ratio {worst / unit:.4f}; plain world {plain / unit:.1f}")
    assert all(s[3] >= 1 for s in w.stats[2:]), "every pair after the first is resected"
    assert worst <= rr.C_BOUND * unit
    assert abs(worst / unit - rr.MEASURED_RATIOS[seed]) < 1e-3
    assert plain > rr.C_BOUND * unit, "the plain world keeps the pairs' errors"


@pytest.mark.parametrize("seed", rr.SCENE_SEEDS)
def test_exact_scenes_with_planted_outliers(scenes, seed):
    sc = scenes[(seed, 0.2)]
    w, worst, unit = rr.run_scene(sc)
    print(f"seed {seed}: ratio {worst / unit:.4f}, participants {[int(s[0]) for s in w.stats[2:]]} of {[len(i['links']) for i in w.infos[2:]]}")
    assert worst <= rr.C_BOUND * unit
    assert abs(worst / unit - rr.MEASURED_RATIOS_OUTLIERS[seed]) < 1e-3
    for f in range(2, sc["frames"]):
        info, p = w.infos[f], sc["pairs"][f - 1]
        assert info["moved"] and w.stats[f][0] >= rr.DEFAULTS["min_links"]
        seconds = np.array([b for _, _, b in info["links"]])
        planted = np.isin(seconds, p["planted"])
        assert planted.any(), "the step has outliers among its links"
        assert info["part"][~planted].all(), "no unplanted link is dropped"
        assert w.links[f] == len(info["links"]), "d_links stays L"


def test_calibration_is_four_times_the_worst_ratio():
    worst = max(max(rr.MEASURED_RATIOS.values()), max(rr.MEASURED_RATIOS_OUTLIERS.values()))
    assert 4 * worst <= rr.C_BOUND < 4 * worst + 0.5


# ------------------------------------------------------------------------------------------------ hand cases
def test_left_alone_below_min_links_and_moved_at_it():
    P, x, R, T, p = rr.comparison_cases()["n40"]
    keep = rr.comparison_results()["n40"][3]["part"].nonzero()[0]          # no outliers among them
    Ro, To, st, info = rr.resect(P[keep[:7]], x[keep[:7]], rr.kmat(), R, T)
    assert not info["moved"] and st[0] == 7 and np.isnan(st[1:]).all()
    assert np.array_equal(Ro, R) and np.array_equal(To, T)
    Ro, To, st, info = rr.resect(P[keep[:8]], x[keep[:8]], rr.kmat(), R, T)
    assert info["moved"] and st[0] == 8 and st[3] >= 1 and st[2] < st[1]


def test_a_round_below_min_links_keeps_the_previous_result():
    P, x, R, T, p = rr.comparison_cases()["n40"]
    one = rr.resect(P, x, rr.kmat(), R, T, rounds=1)
    gated = rr.resect(P, x, rr.kmat(), R, T, rounds=3, gate_px=1e-9)       # nobody passes this gate
    assert one[3]["moved"] and gated[3]["moved"]
    assert np.array_equal(one[0], gated[0]) and np.array_equal(one[1], gated[1]) and np.array_equal(one[2], gated[2])
    assert gated[2][0] == 40 and len(gated[3]["objective"]) == 1
    full = rr.resect(P, x, rr.kmat(), R, T)
    assert full[2][0] == 32 and not np.array_equal(full[0], one[0]), "with the default gate the later rounds drop the outliers"


def test_a_point_behind_the_camera_refuses_every_step():
    P, x, R, T, p = rr.comparison_cases()["n8"]
    Pb = np.vstack([P, [[0.3, -0.2, -5.0]]])
    xb = np.vstack([x, [[300.0, 200.0]]]).astype(np.float32)
    Ro, To, st, info = rr.resect(Pb, xb, rr.kmat(), R, T, rounds=1)
    assert not info["moved"] and np.array_equal(Ro, R) and np.array_equal(To, T) and np.isnan(st[3])
    assert rr.resect(P, x, rr.kmat(), R, T, rounds=1)[3]["moved"], "the same item without that point moves"
    # a later round's gate asks for Y_z > 0 under the previous result: the point leaves and the others move the pose
    Ro, To, st, info = rr.resect(Pb, xb, rr.kmat(), R, T, rounds=2)
    assert info["moved"] and st[0] == 8 and not info["part"][8] and len(info["objective"][0]) == 1


def test_non_finite_input_leaves_the_item_alone():
    P, x, R, T, p = rr.comparison_cases()["n40"]
    for what in ("P", "x", "R", "T"):
        a = dict(P=P.copy(), x=x.copy(), R=R.copy(), T=T.copy())
        a[what].reshape(-1)[2] = np.inf
        Ro, To, st, info = rr.resect(a["P"], a["x"], rr.kmat(), a["R"], a["T"])
        assert not info["moved"] and np.array_equal(Ro, a["R"]) and np.array_equal(To, a["T"]), what


def test_a_non_finite_keypoint_is_no_link(scenes):
    sc = scenes[(1, 0.0)]
    w = rr.World(sc["n"])
    p1, p2 = sc["pairs"][0], sc["pairs"][1]
    w.step(p1["matches"], p1["X"], p1["R"], p1["t"], 60, 60, xy_cur=p1["xy_cur"], K=rr.kmat())
    assert not w.infos[1]["moved"] and w.stats[1][0] == 0, "the first pair has no carry: the plain step"
    w2 = rr.World(sc["n"]); w2.carry, w2.valid = w.carry.copy(), w.valid.copy()
    w.step(p2["matches"], p2["X"], p2["R"], p2["t"], 60, 60, xy_cur=p2["xy_cur"], K=rr.kmat())
    links = w.infos[2]["links"]
    xy = p2["xy_cur"].copy()
    xy[links[3][2], 1] = np.nan
    w2.Twc, w2.scale, w2.links = w.Twc[:2], w.scale[:2], w.links[:2]
    w2.step(p2["matches"], p2["X"], p2["R"], p2["t"], 60, 60, xy_cur=xy, K=rr.kmat())
    assert w2.infos[-1]["links"] == links[:3] + links[4:]
    assert w2.links[-1] == w.links[2] == len(links), "d_links counts the links of the plain step"
    assert w2.infos[-1]["moved"]


def test_left_alone_step_is_the_plain_step(scenes):
    sc = scenes[(2, 0.0)]
    a, b = rr.World(sc["n"], resection=dict(min_links=1000)), rw.World(sc["n"])
    for p in sc["pairs"][:3]:
        a.step(p["matches"], p["X"], p["R"], p["t"], 60, 60, xy_cur=p["xy_cur"], K=rr.kmat())
        b.step(p["matches"], p["X"], p["R"], p["t"], 60, 60)
    assert all(np.array_equal(x, y) for x, y in zip(a.Twc, b.Twc)) and a.scale == b.scale and a.links == b.links
    assert np.array_equal(a.carry, b.carry) and np.array_equal(a.valid, b.valid)


# ------------------------------------------------------------------------------------------------ planted errors
@pytest.mark.parametrize("plant,outliers", [("skew_sign", 0.0), ("T_frozen", 0.0), ("carry_from_pair", 0.0), ("weight_inverted", 0.2)])
def test_planted_error_is_caught_by_the_exact_scenes(scenes, plant, outliers):
    sc = scenes[(rr.SCENE_SEEDS[0], outliers)]
    _, worst, unit = rr.run_scene(sc, plant=plant)
    print(f"{plant}: ratio {worst / unit:.1f}")
    assert worst > 10 * rr.C_BOUND * unit


# ------------------------------------------------------------------------------------------------ the second formulation
def test_the_two_formulations_agree_and_delta_ref_is_what_is_recorded():
    d = {n: rr.disagreement(n) for n in rr.DELTA_REF_CASES}
    print("disagreement", {n: f"{v:.2e}" for n, v in d.items()})
    worst = max(d.values())
    assert worst <= rr.DELTA_REF, "the recorded delta_ref covers what is measured here"
    assert worst >= rr.DELTA_REF / 10, "and is not a loose figure"


def test_decided_cases_are_decided():
    for name, (R, T, st, info) in rr.comparison_results().items():
        assert info["moved"] and info["gate_margin"] >= rr.DECIDED_MARGIN, name
        if name.startswith("decided"):
            assert info["margin"] >= rr.DECIDED_MARGIN and st[3] == 4, name
