"""What the kernels of vslam_sim3_ransac / vslam_sim3_refine compile (vslam_amd/csrc/sim3_math.h: the 3-point model with M_a / M_b,
the division-free inlier test, the key, the rounds of the 7-parameter polish; the sampler and the frame by inclusion of pnp_math.h)
built for the host as a stand-alone program with -fsanitize=address,undefined -ffp-contract=off and walked serially
(tests/native/sim3_serial.cpp), held to tests/ref_sim3.py without a GPU.

Bit for bit on every scene: the sets, the models with M_a / M_b, every count, the winner, the mask, the compaction and the
unpolished (s, R, t).  The polish within 16 x ref_sim3.DELTA_REF (measured: 0 on every planted scene -- numpy adds the 35 sums row
by row, which is the serial order; the device's order is block_reduce.h's)."""
import numpy as np
import pytest

import ref_resect as rr
import ref_sim3 as r3
import sim3_cases as sc3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sc3.build_serial(tmp_path_factory.mktemp("sim3_serial"))


@pytest.mark.parametrize("k", range(len(r3.CONFIGS)))
def test_planted_scenes_on_the_serial_walk(exe, tmp_path, k):
    pairs = sc3.planted_config(k)
    H = r3.CONFIGS[k][2]
    worst = 0.0
    for (c, ref), got in zip(pairs, sc3.run_serial(exe, tmp_path, [c for c, _ in pairs])):
        sc3.hold_exact((k, c["seed"]), got, ref, H)
        assert np.array_equal(got["inlier"].astype(bool), c["scene"]["planted"])
        assert got["stats"][3] >= 1 and got["stats"][0] == ref["stats"][0]
        worst = max(worst, sc3.model_distance(got, ref))
        assert r3.model_error(got["s"], got["R"], got["t"], c["scene"]) <= r3.PLANTED_POLISH_BOUND
    print(f"config {r3.CONFIGS[k]}: polished serial against the reference {worst:.2e}")
    assert worst <= 16 * r3.DELTA_REF


def test_hand_cases_on_the_serial_walk(exe, tmp_path):
    hc = sc3.hand_cases()
    for (name, (c, found)), got in zip(hc.items(), sc3.run_serial(exe, tmp_path, [c for c, _ in hc.values()])):
        assert (got["winner"] >= 0) == found, name
        sc3.hold_exact(name, got, sc3.reference(c), c["params"]["hypotheses"])
        if not found:
            for k, keep in (("s", sc3.KEEP_S), ("R", sc3.KEEP_R), ("t", sc3.KEEP_T)):
                assert sc3.same_bits(got[k], keep) and sc3.same_bits(got[k + "_raw"], keep), (name, k)


def test_the_refinement_alone_on_the_serial_walk(exe, tmp_path):
    """vslam_sim3_refine from a start 1 degree / 3 % / 0.05 off, with a mask, and the items it leaves alone"""
    cases, refs = [], []
    for n, share, seed in r3.POLISH_CASES:
        sc, rows, start = r3.polish_case(n, share, seed)
        cases.append(sc3.refine_case((sc["A"], sc["xa"], sc["B"], sc["xb"]), sc["K"], start, mask=sc["planted"]))
    sc, rows, start = r3.polish_case(*r3.POLISH_CASES[0])
    cases.append(sc3.refine_case(rows, sc["K"], start, mask=np.arange(len(rows[0])) < 7))             # fewer than min_links
    cases.append(sc3.refine_case(rows, sc["K"], (0.0, start[1], start[2])))                             # s not > 0
    cases.append(sc3.refine_case(rows, sc["K"], (start[0], np.full(9, np.nan), start[2])))              # a NaN rotation
    worst = 0.0
    for i, (c, got) in enumerate(zip(cases, sc3.run_serial(exe, tmp_path, cases))):
        ref = sc3.reference(c)
        moved = i < len(r3.POLISH_CASES)
        assert ref["info"]["moved"] == moved, i
        if moved:
            assert np.array_equal(got["stats"][[0, 3]], ref["stats"][[0, 3]]), i
            assert np.abs(got["stats"][1:3] - ref["stats"][1:3]).max() <= 1e-9 * max(1.0, ref["stats"][1]), i
            worst = max(worst, sc3.model_distance(got, ref))
        else:
            assert np.isnan(got["stats"][1:]).all() and got["stats"][0] == ref["stats"][0], i
            assert sc3.same_bits(got["s"], c["keep"][0]) and sc3.same_bits(got["R"], c["keep"][1]) and sc3.same_bits(got["t"], c["keep"][2]), i
    print(f"the refinement alone: serial against the reference {worst:.2e}")
    assert worst <= 16 * r3.DELTA_REF


def test_without_polish_the_statistics_are_nan_and_the_model_is_the_winners(exe, tmp_path):
    c = sc3.case(r3.planted(40, 0.5, 3), seed=3)
    got = sc3.run_serial(exe, tmp_path, [c])[0]
    assert np.isnan(got["stats"]).all()
    assert sc3.same_bits(got["s"], got["s_raw"]) and sc3.same_bits(got["R"], got["R_raw"]) and sc3.same_bits(got["t"], got["t_raw"])


def test_a_hypothesis_depends_on_seed_h_and_n_alone(exe, tmp_path):
    sc = r3.planted(40, 0.5, 3)
    a, b = sc3.run_serial(exe, tmp_path, [sc3.case(sc, seed=3, hypotheses=64), sc3.case(sc, seed=3, hypotheses=192)])
    assert np.array_equal(a["counts"], b["counts"][:64]) and sc3.same_bits(a["models"], b["models"][:64]) and a["winner"] == b["winner"]
