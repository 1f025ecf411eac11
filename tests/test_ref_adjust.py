"""tests/ref_adjust.py, the numpy restatement of include/vslam_adjust.h, held to conditions it alone has to meet (no GPU):
its Schur step is the step of the full damped normal equations; on exact problems it brings the camera centres and the
participating points back to the truth, with and without planted outliers, from a start that is off by orders of magnitude more;
it gates out few true observations; its result does not depend on the order of a point's observations or of the points beyond
rounding; and a second formulation (scipy) agrees with it within DELTA_REF.  Each planted fault in the reference misses at
least one of the first three."""
import numpy as np
import pytest

import ref_adjust as ra

REORDER_BOUND = 1e-8   # measured: 5.3e-10 at most (c3n9; 1.2e-14 and 3.1e-15 on the others) over the cases below (the reduced system's rounding, amplified by its condition)


def _start_state(name):
    pr, p = ra.cases()[name]
    K = ra.kmat().astype(np.float64).reshape(9)
    pid = np.repeat(np.arange(len(pr["X"])), np.diff(pr["off"]))
    slot = np.where(np.arange(len(pr["R"])) >= p["n_fixed"], np.arange(len(pr["R"])) - p["n_fixed"], -1)
    return K, pr["R"].copy(), pr["T"].copy(), pr["X"].copy(), pid, pr["cam"].astype(np.int64), pr["xy"].astype(np.float64), slot


@pytest.mark.parametrize("name,lam", [("c4n40", 1e-3), ("c8n257", 1e-3), ("c4n40", 10.0), ("c3n9", 1e-6)])
def test_schur_step_is_the_step_of_the_full_normal_equations(name, lam):
    a = _start_state(name)
    dc, dX, touched = ra.step(*a, 2.0, lam)
    dc2, dX2 = ra.dense_step(*a, 2.0, lam)
    scale = max(np.abs(dc2).max(), np.abs(dX2).max())
    d = max(np.abs(dc - dc2).max(), np.abs(dX - dX2).max()) / scale
    print(f"{name} lambda {lam}: Schur against dense {d:.1e} of the step's largest entry")
    assert touched.all() and d <= 1e-7
    dc3, dX3, _ = ra.step(*a, 2.0, lam, plant="schur_dropped")
    assert max(np.abs(dc3 - dc2).max(), np.abs(dX3 - dX2).max()) / scale > 1e-4, "the planted fault is seen"


@pytest.fixture(scope="module")
def exact():
    out = {}
    for o in (0.0, 0.2):
        for seed in ra.EXACT_SEEDS:
            pr = ra.problem(seed, outliers=o, **ra.EXACT_SHAPE)
            out[o, seed] = (pr, ra.run(pr))
    return out


def test_exact_problems_come_back_with_and_without_outliers(exact):
    for (o, seed), (pr, res) in exact.items():
        err, unit = ra.recovery(pr, res)
        start = max(np.abs(ra.centres(pr["R"], pr["T"]) - pr["centres_true"]).max(), np.abs(pr["X"] - pr["X_true"]).max())
        want = (ra.MEASURED_RATIOS_OUTLIERS if o else ra.MEASURED_RATIOS)[seed]
        print(f"outliers {o} seed {seed}: error / unit {err / unit:.4f} (recorded {want}), start off by {start:.1e}, accepted {res[3][3]:.0f}")
        assert res[4]["moved"] and err <= ra.C_BOUND * unit and start > 1e3 * err
        assert abs(err / unit - want) <= 0.05 * want, "the recorded ratio is what the reference gives"
        if o:
            assert pr["planted"].sum() >= 0.15 * len(pr["planted"]) and not (res[4]["part"] & pr["planted"]).any()
    assert ra.C_BOUND >= 4 * max(max(ra.MEASURED_RATIOS.values()), max(ra.MEASURED_RATIOS_OUTLIERS.values()))


@pytest.mark.parametrize("plant", ["fixed_moves", "gate_round0", "one_camera_rule", "schur_dropped"])
def test_planted_faults_miss_the_recovery(plant):
    missed = 0
    for seed in ra.EXACT_SEEDS[:3]:
        pr = ra.problem(seed, outliers=0.2, **ra.EXACT_SHAPE)
        res = ra.run(pr, plant=plant)
        err, unit = ra.recovery(pr, res)
        gated = (~res[4]["part"] & ~pr["planted"]).sum() / (~pr["planted"]).sum()
        print(f"{plant} seed {seed}: error / unit {err / unit:.3g}, true observations gated out {gated:.2f}")
        missed += int(not res[4]["moved"] or not err <= ra.C_BOUND * unit or gated >= 0.25)
    assert missed >= 1


def test_few_true_observations_are_gated_out(exact):
    runs = [(f"exact {k}", pr, res) for k, (pr, res) in exact.items()]
    runs += [(n, ra.cases()[n][0], ra.comparison_results()[n]) for n in ra.cases()]
    for name, pr, res in runs:
        true = ~pr["planted"]
        gated = (~res[4]["part"] & true).sum() / true.sum()
        print(f"{name}: {gated:.3f} of the true observations gated out")
        assert res[4]["moved"] and gated < 0.25


def _permuted(pr, rng, points=False):
    N = len(pr["X"])
    order = rng.permutation(N) if points else np.arange(N)
    idx = np.concatenate([rng.permutation(np.arange(pr["off"][i], pr["off"][i + 1])) for i in order])
    off = np.concatenate([[0], np.cumsum(np.diff(pr["off"])[order])]).astype(np.int32)
    return dict(pr, X=pr["X"][order], off=off, cam=pr["cam"][idx], xy=pr["xy"][idx]), order


@pytest.mark.parametrize("name", ["c3n9", "c4n40", "c8n257"])
def test_reordering_observations_and_points_moves_the_result_within_rounding(name):
    pr, p = ra.cases()[name]
    R, T, X, st, info = ra.comparison_results()[name]
    rng = np.random.default_rng(5)
    worst = 0.0
    for points in (False, True):
        q, order = _permuted(pr, rng, points)
        R2, T2, X2, st2, _ = ra.run(q, **p)
        d = max(np.abs(R2 - R).max(), np.abs(T2 - T).max() / max(1.0, np.abs(T).max()), np.abs(X2 - X[order]).max() / max(1.0, np.abs(X).max()))
        worst = max(worst, d)
        assert st2[0] == st[0]
    print(f"{name}: reordering moves the result by {worst:.1e}")
    assert worst <= REORDER_BOUND


def test_second_formulation_agrees_within_delta_ref():
    per = {n: ra.disagreement(n) for n in ra.DELTA_REF_CASES}
    print("disagreement per case:", {k: f"{v:.2e}" for k, v in per.items()}, "DELTA_REF", ra.DELTA_REF)
    assert max(per.values()) <= ra.DELTA_REF < 1e-6 and max(per.values()) >= 0.25 * ra.DELTA_REF
    for n in ra.cases():
        info = ra.comparison_results()[n][4]
        assert info["moved"] and info["gate_margin"] >= ra.DECIDED_MARGIN, n
        if n.startswith("decided"):
            assert info["margin"] >= ra.DECIDED_MARGIN, n
