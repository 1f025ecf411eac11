"""tests/ref_graph.py, the restatement of include/vslam_graph.h, held on the CPU: its analytic Jacobians against central differences,
its minimum against a second formulation (scipy.optimize.least_squares over 4 x 4 homogeneous products), the drifting loops of the
issue's prototype, every left-alone and unusable-edge rule, and -- a condition on the inputs of every test -- that no case runs
into cg_iterations or max_iterations.  No GPU."""
import numpy as np
import pytest

import graph_cases as gc
import ref_graph as rg


def test_analytic_jacobians_against_central_differences():
    worst = 0.0
    for seed in rg.JACOBIAN_CASES:
        rng = np.random.default_rng(seed)
        node = lambda: (float(rng.uniform(0.5, 2)), rg.random_rotation(rng, rng.uniform(0, 1.5)), rng.normal(size=3) * 3)
        one = lambda n: (np.array([n[0]]), n[1][None], n[2][None])
        a, b, Z = node(), node(), node()
        Ja, Jb = rg.jacobians(*one(a), *one(b), *one(Z))
        Na, Nb = rg.numeric_jacobian(a, b, Z)
        worst = max(worst, float(np.abs(Ja[0] - Na).max()), float(np.abs(Jb[0] - Nb).max()))
    print(f"analytic against central differences: {worst:.3e} (recorded {rg.JACOBIAN_WORST:.3e})")
    assert worst <= rg.JACOBIAN_BOUND


def test_consistent_graphs_against_the_second_formulation():
    worst = 0.0
    for N, loops, seed in rg.CONSISTENT_CASES:
        it, truth = rg.consistent(N, loops, seed)
        s, R, T, stats, info = rg.optimize(*rg.args(it), **rg.CONSISTENT_PRM)
        assert info["moved"] and not info["cg_capped"] and not info["lm_capped"], (N, seed)
        assert stats[0] == N - 1 + loops and stats[2] < stats[1]
        assert np.array_equal(info["written"], np.arange(N) > 0)
        s2, R2, T2 = rg.second_formulation(*rg.args(it))
        d = rg.distance((s, R, T), (s2, R2, T2), info["written"])
        worst = max(worst, d)
    print(f"optimize() against second_formulation(): {worst:.3e} (recorded {rg.DELTA_REF:.3e})")
    assert worst <= 4 * rg.DELTA_REF   # held at 4 x the recorded value, as the Jacobians are


def test_drifting_loops_come_back():
    worst = 0.0
    for N, seed in rg.DRIFT_CASES:
        it, truth = rg.drifting(N, seed)
        before = rg.centre_error(it["T"], truth)
        s, R, T, stats, info = rg.optimize(*rg.args(it))
        assert info["moved"] and not info["cg_capped"] and not info["lm_capped"], (N, seed)
        after = rg.centre_error(T, truth)
        print(f"N = {N} seed {seed}: centre error {before:.3f} -> {after:.3f}, cost {stats[1]:.3e} -> {stats[2]:.3e}, {int(stats[3])} steps, "
              f"CG {info['cg']}")
        assert stats[2] < stats[1]
        assert after <= rg.DRIFT_BOUND * before, (N, seed)
        worst = max(worst, after / before)
    print(f"worst after / before: {worst:.4f} (recorded {rg.DRIFT_WORST})")


def test_no_case_of_the_tests_runs_into_an_iteration_cap():
    for k in range(len(gc.SHAPES)):
        info = gc.reference(gc.shape_item(k))["info"]
        assert info["moved"] and not info["cg_capped"] and not info["lm_capped"], gc.SHAPES[k]
    for name, (it, moved, use) in gc.hand_cases().items():
        info = gc.reference(it)["info"]
        assert not info["cg_capped"], name
        assert not (moved and info["lm_capped"]), name


@pytest.mark.parametrize("name", sorted(gc.hand_cases()))
def test_hand_cases(name):
    it, moved, use = gc.hand_cases()[name]
    ref = gc.reference(it)
    assert ref["info"]["moved"] == moved and ref["stats"][0] == use
    S = len(it["scale"])
    got = dict(scale=ref["scale"], R=ref["R"].reshape(S, 9), T=ref["T"].reshape(S, 3))
    w = gc.written(got, it)
    if not moved:
        assert not w.any() and np.isnan(ref["stats"][1:]).all()
        return
    N = int(it["n_nodes"])
    usable = rg.usable_edges(N, int(it["n_edges"]), it["fixed"], it["ab"], it["zs"], it["zR"], it["zt"], it["zw"])
    touched = np.zeros(S, bool)
    touched[np.asarray(it["ab"])[:int(it["n_edges"])][usable].reshape(-1)] = True
    assert np.array_equal(w, touched & (it["fixed"] == 0))   # free nodes with a usable edge, and nothing else
    assert ref["stats"][2] < ref["stats"][1] and ref["stats"][3] >= 1
