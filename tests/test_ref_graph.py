"""tests/ref_graph.py, the restatement of include/vslam_graph.h, held on the CPU: its analytic Jacobians against central differences,
its minimum against a second formulation (scipy.optimize.least_squares over 4 x 4 homogeneous products), the drifting loops of the
issue's prototype, every left-alone and unusable-edge rule, and -- a condition on the inputs of every test -- that no case runs
into cg_iterations or max_iterations.  For the loops that disagree (graph_cases.LOOP_CASES) the opposite condition: under their
fixed flow every solve and the outer loop run exactly to their caps, the conjugate gradient still far above its floor; and the
reference's weights against scipy's where the weights decide where the minimum lies.  No GPU."""
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


# ------------------------------------------------------------------------------------------------ loops that disagree, weights that differ
def test_weighted_minimum_against_the_second_formulation():
    """optimize()'s weights against scipy's on scenes whose minimum costs > 0, where the weights decide where it lies: the same
    scenes under unit weights must end at least 1000 bounds away, or the check could not tell the weights at all."""
    worst, nearest = 0.0, np.inf
    for N, seed in rg.WEIGHT_CASES:
        it, truth = rg.weighted_drift(N, seed)
        E = it["n_edges"]
        assert it["zw"][:E].min() >= 0.25 and it["zw"][:E].max() <= 4.0 and len(np.unique(it["zw"][:E])) == 3 * E
        assert (it["ab"][:E, 0] > it["ab"][:E, 1]).sum() == 2   # both loops are written from the later frame to the earlier one
        s, R, T, stats, info = rg.optimize(*rg.args(it), **rg.CONVERGED)
        assert info["moved"] and not info["cg_capped"] and not info["lm_capped"], (N, seed)
        s2, R2, T2 = rg.second_formulation(*rg.args(it))
        unit = dict(it, zw=np.where(np.isnan(it["zw"]), np.nan, 1.0))
        s3, R3, T3, _, info3 = rg.optimize(*rg.args(unit), **rg.CONVERGED)
        d = rg.distance((s, R, T), (s2, R2, T2), info["written"])
        u = rg.distance((s3, R3, T3), (s2, R2, T2), info["written"])
        print(f"N = {N} seed {seed}: weighted {d:.3e}, under unit weights {u:.3e} from scipy's weighted minimum")
        worst, nearest = max(worst, d), min(nearest, u)
    print(f"optimize() against second_formulation(), weighted: {worst:.3e} (recorded {rg.WEIGHT_WORST:.3e})")
    assert worst <= rg.WEIGHT_BOUND
    assert nearest >= 1000 * rg.WEIGHT_BOUND


@pytest.mark.parametrize("name", [c[0] for c in gc.LOOP_CASES])
def test_fixed_flow_cases_run_exactly_to_their_caps(name):
    """The condition the fixed-flow comparisons rest on: every solve ends at cg_iterations with rho' / rho_0 >= FLOW_RATIO (cut
    far above the floor, not run past convergence), every outer step is accepted, so stats[3] == max_iterations; and the scene is
    what graph_cases says it is."""
    it = gc.loop_item(name)
    prm, ref = it["prm"], gc.reference(it)
    info = ref["info"]
    assert prm["cg_tolerance"] == 1e-30 and 1 <= prm["max_iterations"] <= 3
    assert info["moved"] and info["steps"] == info["accepted"] == prm["max_iterations"] == ref["stats"][3]
    assert info["cg"] == [prm["cg_iterations"]] * prm["max_iterations"]
    print(name, "rho' / rho_0 at each exit:", info["cg_ratio"])
    assert min(info["cg_ratio"]) >= rg.FLOW_RATIO
    assert ref["stats"][2] < ref["stats"][1] and ref["stats"][2] > 1e-6        # the minimum costs > 0: the loops disagree
    N, E = it["n_nodes"], it["n_edges"]
    w, ab = it["zw"][:E], it["ab"][:E]
    zero = [gc.ZERO_WEIGHT[1]] if name == gc.ZERO_WEIGHT[0] else []
    assert (w == 0).sum() == len(zero) and all(w[z] == 0 for z in zero)
    assert w[w > 0].min() >= 0.25 and w.max() <= 4.0 and len(np.unique(w)) >= 3 * E - 1
    assert rg.group_weights(it)[info["written"][:N]].min() > 0.25              # the damping floor 2^-40 stays out of play
    deg = np.bincount(ab.reshape(-1), minlength=N)
    pairs = len({(min(a, b), max(a, b)) for a, b in ab.tolist()})
    if name in gc.DRIFT_LOOPS:
        assert (ab[:, 0] > ab[:, 1]).sum() == 2 and ref["stats"][0] == E == N + 1
    if name == gc.ZERO_WEIGHT[0]:
        assert all(deg[n] >= 2 and not it["fixed"][n] for n in ab[zero[0][0]])
    if name == "hub":
        assert (N, E) == (8, 600) and deg[1] == 600 and it["fixed"][1] == 0 and pairs == 7
        assert (ab[:, 0] == 1).sum() > 250 and (ab[:, 1] == 1).sum() > 250
    if name == "hub257":
        assert (N, E) == (3, 257) and deg[1] == 257 and pairs == 2
    if name == "star300":
        assert (N, E) == (300, 700) and deg[299] == 600 and (deg == 0).sum() == 43 and not info["written"][deg == 0].any()
        assert info["written"].sum() == 256 and pairs < E
    if name == "capacity":
        assert (N, E) == (rg.MAX_NODES, rg.MAX_EDGES) == (len(it["scale"]), len(it["zs"])) and it["fixed"].sum() == 128
        assert ref["stats"][0] >= E - 8   # but the few loops that join two held nodes
