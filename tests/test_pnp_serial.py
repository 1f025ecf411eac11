"""What the kernels of vslam_pnp_ransac compile (vslam_amd/csrc/pnp_math.h: the sampler, P3P by Ferrari's quartic and two frames,
the inlier test, the key; the polish through resect_math.h) built for the host as a stand-alone program with
-fsanitize=address,undefined and walked serially (tests/native/pnp_serial.cpp), held to tests/ref_pnp.py -- numpy.roots and an SVD
orientation -- without a GPU.

Exact on every scene: the sets (through d_winner / 4, which names the first hypothesis reaching the winning count), the winner's
hypothesis, the inlier mask, the count and the compacted indices.  Not exact: the unpolished pose, two formulations of P3P on the
same three f32-rounded pixels.  Measured over the 100 planted scenes of ref_pnp.CONFIGS: at most 1.51e-9 entry-wise;
DELTA_PNP = 6.1e-9 = 4 x.  (The winner's slot d_winner % 4 and the counts of poses that are not the winner are this
formulation's own: a nearly double root of the quartic is one pose here and two or none there.)  The polished poses agree to the
resection's own tolerance (16 x ref_resect.DELTA_REF; measured 4.9e-12) and are held to the truth within POLISH_BOUND, as the
reference is."""
import numpy as np
import pytest

import pnp_cases as pc
import ref_pnp as rp
import ref_resect as rr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pc.build_serial(tmp_path_factory.mktemp("pnp_serial"))


def hold(name, c, got, ref):
    assert (got["winner"] >= 0) == ref["found"], name
    assert got["winner"] // 4 == ref["winner_h"] or not ref["found"], (name, got["winner"], ref["winner_h"])
    assert got["n_inliers"] == ref["n_inliers"], name
    assert np.array_equal(got["inlier"], ref["inlier"]), name
    assert np.array_equal(got["corr_index"], ref["corr_index"]), name
    if not ref["found"]:
        assert got["winner"] == -1 and (got["counts"] >= -1).all(), name
        for k in ("R_raw", "T_raw", "R", "T"):
            assert pc.same_bits(got[k], pc.KEEP_R if k[0] == "R" else pc.KEEP_T), (name, k)
        return 0.0
    assert got["counts"][got["winner"] // 4, got["winner"] % 4] == got["n_inliers"] == got["counts"].max(), name
    return max(float(np.abs(got["R_raw"] - ref["R_raw"]).max()), float(np.abs(got["T_raw"] - ref["T_raw"]).max()))


@pytest.mark.parametrize("k", range(len(rp.CONFIGS)))
def test_planted_scenes_on_the_serial_walk(exe, tmp_path, k):
    pairs = pc.planted_config(k)
    worst = pol = 0.0
    for (c, ref), got in zip(pairs, pc.run_serial(exe, tmp_path, [c for c, _ in pairs])):
        sc = c["scene"]
        worst = max(worst, hold((k, c["seed"]), c, got, ref))
        assert np.array_equal(got["inlier"].astype(bool), sc["planted"])
        assert rp.pose_error(got["R_raw"], got["T_raw"], sc) <= rp.RAW_BOUND
        pol = max(pol, rp.pose_error(got["R"], got["T"], sc) / (2.0 ** -23 * np.abs(sc["points"]).max()))
        assert got["stats"][3] >= 1
        assert max(np.abs(got["R"] - ref["R"]).max(), np.abs(got["T"] - ref["T"]).max()) <= 16 * rr.DELTA_REF
    print(f"config {rp.CONFIGS[k]}: unpolished serial against reference {worst:.2e}; polished against the truth, ratio {pol:.2f}")
    assert worst <= rp.DELTA_PNP and pol <= rp.POLISH_BOUND


def test_hand_cases_on_the_serial_walk(exe, tmp_path):
    hc = pc.hand_cases()
    for (name, (c, found)), got in zip(hc.items(), pc.run_serial(exe, tmp_path, [c for c, _ in hc.values()])):
        assert (got["winner"] >= 0) == found, name
        assert hold(name, c, got, pc.reference(c)) <= rp.DELTA_PNP, name
        # an item left alone, and degenerate samples, have no pose in any hypothesis -- and no NaN downstream
        assert (got["counts"] == -1).all() == (not found and name != "below_min_inliers"), name


def test_without_polish_the_statistics_are_nan_and_the_pose_is_the_winners(exe, tmp_path):
    c = pc.case(rp.planted(40, 0.5, 3), seed=3)
    got = pc.run_serial(exe, tmp_path, [c])[0]
    assert np.isnan(got["stats"]).all() and pc.same_bits(got["R"], got["R_raw"]) and pc.same_bits(got["T"], got["T_raw"])


def test_a_hypothesis_depends_on_seed_h_and_n_alone(exe, tmp_path):
    """the counts of hypothesis h are the same whatever the number of hypotheses"""
    sc = rp.planted(40, 0.5, 3)
    a, b = pc.run_serial(exe, tmp_path, [pc.case(sc, seed=3, hypotheses=64), pc.case(sc, seed=3, hypotheses=192)])
    assert np.array_equal(a["counts"], b["counts"][:64]) and a["winner"] == b["winner"]


def test_the_key_orders_counts_then_the_smaller_pose_index(tmp_path):
    """tests/native/pnp_key_check.cpp: pn_key exhaustively, the slot s of 4 h + s included, which no scene here exercises (no planted
    scene has two slots of one hypothesis at the winning count)."""
    import os
    import subprocess
    out = str(tmp_path / "pnp_key_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                    os.path.join(pc.ROOT, "tests", "native", "pnp_key_check.cpp")], check=True)
    assert subprocess.run([out], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_the_winner_is_the_first_pose_at_the_largest_count(exe, tmp_path):
    cases = [c for k in (0, 1) for c, _ in pc.planted_config(k)] + [pc.case(rp.planted(40, 0.0, 8), seed=8, hypotheses=64)]
    for c, got in zip(cases, pc.run_serial(exe, tmp_path, cases)):
        flat = got["counts"].ravel()
        assert got["winner"] == np.flatnonzero(flat == flat.max())[0]
