"""tests/ref_search.py, the numpy statement of include/vslam_search.h, held to a second formulation (scipy.spatial.cKDTree for the
discs, np.unpackbits for the distances, a sort for the one-to-one step), to hand cases with outcomes known by hand, to planted
errors that each have to show, and to the conditions on the planted scenes.  CPU only."""
import numpy as np
import pytest

import ref_search as rs
import search_cases as sc

SEEDS = (1, 2, 3, 4, 5, 6)


def run(c, **kw):
    return rs.search_item(c["points"], c["n_points"], c["offsets"], c["obs_desc"], c["R"], c["T"], c["K"], c["width"], c["height"], c["xy"],
                          c["desc"], c["n_kp"], c.get("taken"), **dict(c.get("params", {}), **kw))


def second(c):
    return rs.second_formulation(c["points"], c["n_points"], c["offsets"], c["obs_desc"], c["R"], c["T"], c["K"], c["width"], c["height"],
                                 c["xy"], c["desc"], c["n_kp"], c.get("taken"), **c.get("params", {}))


@pytest.fixture(scope="module")
def scenes():
    return {s: rs.planted_scene(s) for s in SEEDS}


@pytest.fixture(scope="module")
def results(scenes):
    return {s: rs.run_scene(sc_) for s, sc_ in scenes.items()}


def test_hand_cases_have_the_outcomes_worked_out_by_hand():
    for name, c in sc.hand_cases().items():
        r = run(c)
        assert np.array_equal(r["kp_of_point"], c["expect"]), (name, r["kp_of_point"])
        found = r["kp_of_point"] >= 0
        assert r["n_corr"] == found.sum() == r["stats"][3] and np.array_equal(r["dist"] >= 0, found), name
        assert r["stats"][0] >= r["stats"][1] >= r["stats"][2] >= r["stats"][3], name
    h = sc.hand_cases()
    assert run(h["visibility"])["stats"].tolist() == [2, 2, 2, 2]
    assert run(h["last_observation"])["dist"].tolist() == [3]
    assert run(h["contest_no_second_choice"])["stats"].tolist() == [2, 2, 2, 1]
    assert run(h["threshold_64"])["stats"].tolist() == [1, 1, 0, 0]


def test_second_formulation_agrees(scenes, results):
    for s in SEEDS:
        k, d = second(scenes[s])
        assert np.array_equal(k, results[s]["kp_of_point"]) and np.array_equal(d, results[s]["dist"]), s
    for name, c in list(sc.hand_cases().items()) + list(sc.grid_cases().items()):
        r = run(c)
        k, d = second(c)
        assert np.array_equal(k, r["kp_of_point"]) and np.array_equal(d, r["dist"]), name


def test_the_grid_cases_exercise_the_rule():
    """not all empty, with rejections by ratio, by contest, taken and non-finite keypoints among them"""
    lost = bare = 0
    for name, c in sc.grid_cases().items():
        st = run(c)["stats"]
        print(name, st)
        assert st[3] > 0 and st[0] >= st[1] > st[2] >= st[3], (name, st)
        lost += st[2] - st[3]
        bare += st[0] - st[1]
    assert lost > 20 and bare > 20   # proposals that lost their keypoint to another point; visible points without a candidate


PLANT_SHOWS_ON = {"disc_open": ("disc_on_5", "disc_on_8.5", "disc_axis_8.5"), "first_observation": ("last_observation",),
                  "d1_over_all": ("ratio_8_11", "ratio_off"), "tie_to_higher_point": ("contest_lower_i",), "ratio_on_single": ("ratio_single",)}


@pytest.mark.parametrize("plant", rs.PLANTS)
def test_planted_errors_are_caught(plant, scenes, results):
    h = sc.hand_cases()
    for name in PLANT_SHOWS_ON[plant]:
        if plant == "d1_over_all" and name == "ratio_off":
            assert np.array_equal(run(h[name], plant=plant)["kp_of_point"], h[name]["expect"])   # no ratio test: d1 is not read
            continue
        assert not np.array_equal(run(h[name], plant=plant)["kp_of_point"], h[name]["expect"]), (plant, name)
    if plant in ("first_observation", "d1_over_all", "ratio_on_single"):   # and on every planted scene
        for s in SEEDS:
            r = rs.run_scene(scenes[s], plant=plant)
            assert not (np.array_equal(r["kp_of_point"], results[s]["kp_of_point"]) and np.array_equal(r["dist"], results[s]["dist"])), (plant, s)


def test_planted_scenes_meet_the_conditions(scenes, results):
    for s in SEEDS:
        found, wrong = rs.scene_shares(scenes[s], results[s])
        print(f"seed {s}: found / seen {found:.4f}, wrong / found {wrong:.4f}, stats {results[s]['stats']}")
        assert found >= 0.90 and wrong <= 0.05
        assert abs(found - rs.MEASURED_SHARES[s][0]) < 1e-4 and abs(wrong - rs.MEASURED_SHARES[s][1]) < 1e-4


def test_exact_scenes_resect_back_to_the_true_pose():
    worst = [0.0, 0.0]
    for s in SEEDS:
        ex = rs.planted_scene(s, exact=True)
        dR, dT, moved = rs.scene_resect(ex, rs.run_scene(ex))
        print(f"seed {s}: |R - R_true| {dR:.2e}, |T - T_true| {dT:.2e}")
        assert moved and dR <= rs.EXACT_BOUND_R and dT <= rs.EXACT_BOUND_T
        assert dR <= rs.MEASURED_EXACT[s][0] and dT <= rs.MEASURED_EXACT[s][1]   # the record (rounded up) still holds
        worst = [max(worst[0], dR), max(worst[1], dT)]
    # the bounds are 4 x the worst measured: neither stale nor slack
    assert rs.EXACT_BOUND_R <= 4.2 * worst[0] and rs.EXACT_BOUND_T <= 4.2 * worst[1]
    start = np.abs(rs.planted_scene(1, exact=True)["T"] - rs.planted_scene(1, exact=True)["T_true"]).max()
    assert start > 1e-2   # the start is 0.01 rad and 0.02 off: five orders above the bound
