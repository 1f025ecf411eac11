"""tests/ref_refine.py on the CPU: the two formulations of the two-view adjustment agree on every comparison input, every named
shape is a comparison, and the accuracy claim holds.

Measured here: delta_ref = 9.8e-8 (the points of K64_n8; R 3.9e-9, t 9.8e-9, c2 6.9e-9 at their largest) -- refine() stops on a
relative decrease of the objective below 2^-40, which leaves the unknowns about 1e-8 from the minimum that scipy's LM runs into.
The smallest eigenvalue ratio of the final reduced system over the comparison inputs is 4.6e-5 (EIG_BOUND = 1e-9 is far below:
a two-view problem with a baseline is never that flat; the bound catches pure rotations).  Accuracy: the refined (R, t) has the
lower held-out RMS Sampson distance in 32 of 32 pairs (median ratio 0.42, worst 0.97).
The second formulation starts from the inputs, independently of refine(), for n <= 100 (K64_n8, K64_n9, K64_n63, K64_n64,
mixed1_n8, mixed3_n77, mixed6_n40); for the larger shapes it starts from refine()'s result and confirms that result as a
minimum of the 6-dof problem, no more (tests/ref_refine.py says why).  delta_ref is set by an independently confirmed input.
Every run that converges ends on an accepted step within 2^-40 of ratio 1 and is therefore `marginal` in the 1e-9 sense; what is
asserted instead is that every decision of every comparison input is at least DECIDED_MARGIN = 1e-13 away from 1."""
import numpy as np
import pytest

import ref_refine as rr
import ref_refit


@pytest.fixture(scope="module")
def results():
    return rr.comparison_results()


def test_inputs_participate_and_are_comparable(results):
    cases = {c[0]: c for c in rr.comparison_cases()}
    seam = [f"K{rr.SEAM_BATCH[0]}_n{n}" for n in rr.SEAM_BATCH[1]]
    assert len(results) == len(set(f"K{K}_n{n}" for K, n in rr.COMPARISON_SHAPES) | set(seam)) + len(rr.MIXED_BATCH[1])
    assert all(name in results for name in seam) and sorted(rr.SEAM_BATCH[1])[-2:] == [3200, 3201]
    for name, out in results.items():
        info, n = out[4], int(cases[name][4][3])
        assert not info["left_alone"] and info["stats"][0] >= n - 2, name
        assert info["comparable"] and info["eig_ratio"] >= 1e-5, (name, info["eig_ratio"])
        assert info["last_rel"] < rr.REL_STOP, name                  # it converged inside its 20 iterations
        assert info["margin"] >= rr.DECIDED_MARGIN, (name, info["margin"])
    print("marginal in the 1e-9 sense:", sum(o[4]["marginal"] for o in results.values()), "of", len(results))


def test_two_formulations_agree(results):
    for name, out in results.items():
        print(name, {k: f"{v:.1e}" for k, v in out[4]["delta"].items()})
    d = rr.delta_ref()
    print("delta_ref", d)
    assert 3e-8 < d < 3e-7                                          # 9.8e-8 as measured: the device tolerance is 16 of these


def test_properties_of_the_reference(results):
    for name, (R, t, c2, P, info) in results.items():
        obj = info["objective"]
        assert all(b < a for a, b in zip(obj, obj[1:])), name
        assert len(obj) == info["stats"][3] + 1
        R64 = info["R64"]
        assert np.abs(R64.T @ R64 - np.eye(3)).max() <= 1e-13 and np.linalg.det(R64) > 0, name
        assert abs(np.sqrt(info["t64"] @ info["t64"]) - 1.0) <= 1e-15, name
        assert info["stats"][2] < info["stats"][1], name


def test_left_alone_inputs():
    c = rr.case(rr.SHAPE_SEEDS[(64, 64)], 64, 64)
    for kw, R, t in ((dict(winner=-1), c[4], c[5]), (dict(gate_sq=1e-12), c[4], c[5]), (dict(), c[4], -c[5]),
                     (dict(), c[4], np.zeros(3, np.float32))):
        Ro, to, c2, P, info = rr.refine(c[0], c[1], c[2][:64], rr.KMAT, R, t, c[6], kp_stride=64, **kw)
        assert info["left_alone"] and np.isnan(info["stats"][1:]).all()
        assert np.array_equal(Ro.view(np.uint32), np.asarray(R, np.float32).view(np.uint32))
        assert np.array_equal(P.view(np.uint32), c[6].view(np.uint32))


def test_accuracy_claim():
    better, ratios = 0, []
    for p1, p2, m, R, t, P, h1, h2 in rr.accuracy_inputs():
        Ro, to, _, _, info = rr.refine(p1, p2, m, rr.KMAT, R, t, P, rr.GATE_SQ, rr.MAX_ITERATIONS)
        ratios.append(ref_refit.rms_sampson(rr.F_of(rr.KMAT, Ro, to), h1, h2) / ref_refit.rms_sampson(rr.F_of(rr.KMAT, R, t), h1, h2))
    ratios = np.array(ratios)
    print(f"better in {(ratios < 1).sum()} of {len(ratios)}, median {np.median(ratios):.3f}, worst {ratios.max():.3f}")
    assert (ratios < 1).sum() >= 32 - 2


def test_singular_point_block_is_reported_not_raised(oracle):
    """Track 1, pair (0, 1) of the tracking-loop option tests with REFIT and REFINE on, built through the oracle front end
    (tests/ref_chain.py): three participating points run off to a depth of 5e9 .. 8e9 during the 20 iterations, where the depth
    direction of their undamped 3 x 3 block carries nothing in float64 (two of the blocks have an exact zero pivot).  The loop's damping floor keeps its own solves regular;
    the diagnostic after it has no damping and must report such a run, not raise."""
    import ref_chain as rc
    bgr, seeds = rc.sequence_inputs()
    c = rc.pairs_pose(oracle, bgr[1, 0], bgr[1, 1], seeds[1, 0], refit=1, refine=1)
    info = c["refine_info"]
    assert not info["left_alone"] and not info["comparable"] and info["eig_ratio"] == 0.0
    far = np.nonzero(np.abs(info["X64"]).max(1) > 1e8)[0]
    print(f"|X| of the runaway points: {np.abs(info['X64']).max(1)[far]}, singular {info['singular'].tolist()}")
    assert len(far) == 3 and np.array_equal(info["singular"], far)
    assert np.isfinite(c["points4d"]).all() and np.isfinite(c["R"]).all()
