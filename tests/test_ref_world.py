"""tests/ref_world.py, the numpy statement of the world frame, held to ground truth: exact scenes whose lifted points and
camera centres must come back within C_BOUND * 2^-23 * frames * max|X|, hand-worked cases for every rule of the text, and
planted errors that these checks must catch.  No GPU: this pins the reference the device is held to (tests/test_gpu_world.py)."""
import numpy as np
import pytest

import ref_world as rw
import world_cases as wc

CASES = wc.cases()


@pytest.mark.parametrize("seed", rw.SCENE_SEEDS)
def test_exact_scenes_within_the_bound(seed):
    sc = rw.scene(seed)
    assert sc["n"] == 40 and sc["frames"] == 6 and len(set(np.round(sc["base"], 3))) == 5, "baselines of different lengths"
    w, worst, unit = rw.run_scene(sc)
    print(f"seed {seed}: worst error {worst:.3e}, unit {unit:.3e}, ratio {worst / unit:.4f}, links {w.links}")
    assert all(L >= 8 for L in w.links[2:]), "every pair after the first has to find its scale"
    assert worst <= rw.C_BOUND * unit
    # the docstring's calibration is the one measured here
    assert abs(worst / unit - rw.MEASURED_RATIOS[seed]) < 1e-3
    # the recovered scales are the baselines' ratios
    for f in range(1, 6):
        assert abs(w.scale[f] * sc["base"][0] / sc["base"][f - 1] - 1) < 1e-6


def test_calibration_is_four_times_the_worst_ratio():
    worst = max(rw.MEASURED_RATIOS.values())
    assert 4 * worst <= rw.C_BOUND < 4 * worst + 0.1


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_case(name):
    case = CASES[name]
    st, ex = case["steps"][0], case["expect"]
    w = rw.World(wc.K)
    w.carry, w.valid = st["poke"][0].copy(), st["poke"][1].copy()
    w.step(st["matches"], st["X"], st["R"], st["t"], st["n_last"], st["n_cur"])
    assert w.links[1] == ex["links"]
    assert w.scale[1] == ex["scale"]
    for kp, v in ex.get("carry", {}).items():
        assert w.valid[kp] and np.array_equal(w.carry[kp], np.array(v, float)), kp
    for kp in ex.get("invalid", []):
        assert not w.valid[kp], kp
    if "Twc" in ex:
        assert np.array_equal(w.Twc[1], np.array(ex["Twc"], float))
    # exactly the seconds of the usable in-range matches are valid
    assert w.valid.sum() <= len(st["matches"])


def test_pair_without_a_winner_between_two_good_ones():
    w, _ = wc.run_reference(rw, CASES["odd_L9"]["steps"])
    assert w.frames == 5 and w.links[3] == -1
    assert np.array_equal(w.Twc[3], w.Twc[2]) and w.scale[3] == w.scale[2]
    assert w.links[2] == 9 and w.scale[2] != w.scale[1], "the step before it found its own scale from the carry"
    assert w.links[4] == 0 and w.scale[4] == w.scale[3], "the carry was dropped: the next pair has no links and keeps the scale"
    assert not np.array_equal(w.Twc[4], w.Twc[3]) and w.valid.sum() == 12


def test_lift_leaves_rows_outside_the_range():
    w, _ = wc.run_reference(rw, CASES["pose_by_hand"]["steps"])
    P = np.array([[1, 2, 3, 1], [0, 0, 1, 1], [4, 5, 6, 1]], np.float32)
    out = np.full((3, 4), 7, np.float32)
    w.lift(1, P, 1, 2, out)
    assert np.array_equal(out[[0, 2]], np.full((2, 4), 7, np.float32))
    assert np.array_equal(out[1], np.array([0, 0, 2, 1], np.float32))      # pair 1: Twc_0 = I, s_1 = 2


# ------------------------------------------------------------------------------------------------ planted errors
def test_planted_upper_median_is_caught():
    case = CASES["even_L8_lower_median"]
    w, _ = wc.run_reference(rw, case["steps"][:1], plant="upper_median")
    assert w.scale[1] == 5.0 != case["expect"]["scale"]
    w, _ = wc.run_reference(rw, CASES["odd_L9"]["steps"][:1], plant="upper_median")
    assert w.scale[1] == 5.0, "odd L: both medians agree, which is why the even case exists"


@pytest.mark.parametrize("plant", ["Rt_not_transposed", "wrong_side", "carry_by_first"])
def test_planted_geometry_error_is_caught_by_the_exact_scenes(plant):
    sc = rw.scene(rw.SCENE_SEEDS[0])
    _, worst, unit = rw.run_scene(sc, plant=plant)
    print(f"{plant}: ratio {worst / unit:.1f}")
    assert worst > 100 * rw.C_BOUND * unit


def test_planted_carry_by_first_is_caught_by_hand():
    case = CASES["two_onto_one_second"]
    w, _ = wc.run_reference(rw, case["steps"][:1], plant="carry_by_first")
    assert not w.valid[20]
