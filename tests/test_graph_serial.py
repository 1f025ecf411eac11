"""vslam_amd/csrc/graph_math.h -- the code the kernel of vslam_graph_optimize runs -- walked serially by a stand-alone host program
(tests/native/graph_serial.cpp) built with -fsanitize=address,undefined -ffp-contract=off, against tests/ref_graph.py: the number of
usable edges, which nodes are written and every left-alone item's bits exactly, the optimised nodes within 16 x DELTA_REF.  The
program's workspace is exactly the bytes include/vslam_graph.h states, so a pass that ran past its part would be caught.  On
graph_cases.LOOP_CASES -- weighted, with a minimum that costs > 0 -- the walk is held under a fixed flow to 16 x DELTA_FLOW with
the integers and the CG total exact, run to convergence to the coarse bounds, and under weights scaled by a power of two to the
bit.  No GPU."""
import pytest

import graph_cases as gc
import ref_graph as rg


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("graph_serial")
    return gc.build_serial(tmp), tmp


def test_hand_cases(serial):
    exe, tmp = serial
    cases = gc.hand_cases()
    res = gc.run_serial(exe, tmp, [c[0] for c in cases.values()])
    for (name, (it, moved, use)), got in zip(cases.items(), res):
        assert got["stats"][0] == use, name
        gc.hold(name, got, it, 16 * rg.DELTA_REF)
        assert gc.written(got, it).any() == moved, name


def test_shapes(serial):
    exe, tmp = serial
    items = [gc.shape_item(k) for k in range(len(gc.SHAPES))]
    for k, got in enumerate(gc.run_serial(exe, tmp, items)):
        gc.hold(str(gc.SHAPES[k]), got, items[k], 16 * rg.DELTA_REF)


def test_workspace_bytes_are_the_headers():
    for N, E in ((1, 1), (7, 9), (256, 257), (4096, 8192)):
        words = 4 * N + 3 * E + 4
        assert 8 * (124 * N + 45 * E) + 4 * ((words + 1) // 2 * 2) == (1008 * N + 372 * E + 16 + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ loops that disagree, weights that differ
def test_loop_cases_under_a_fixed_flow(serial):
    """Both loops run exactly to their caps (test_ref_graph.py asserts that of the reference), so the two differ by rounding alone:
    the integers, the written set and the CG total are the reference's, the nodes and costs within 16 x DELTA_FLOW."""
    exe, tmp = serial
    items = [gc.loop_item(name) for name, _ in gc.LOOP_CASES]
    worst = 0.0
    for it, got in zip(items, gc.run_serial(exe, tmp, items)):
        assert got["cg"] == sum(gc.reference(it)["info"]["cg"]) == it["prm"]["max_iterations"] * it["prm"]["cg_iterations"], it["name"]
        worst = max(worst, gc.hold_flow(it["name"], got, it))
    print(f"serial walk against optimize() under a fixed flow: {worst:.3e} (recorded {rg.DELTA_FLOW:.3e})")


def test_loop_cases_converged(serial):
    """The coarse net: run to convergence the flows may part, and the nodes agree to CONVERGED_NODES only.  Measured over the
    converged cases and the weighted drift scenes of test_ref_graph.py; the drifting loops come back."""
    exe, tmp = serial
    items = [gc.loop_item(name, "converged") for name in gc.CONVERGED_CASES]
    for N, seed in rg.WEIGHT_CASES:
        it, truth = rg.weighted_drift(N, seed)
        items.append(dict(it, prm=dict(rg.CONVERGED), truth=truth, name=f"weighted_drift({N}, {seed})"))
    wd = wc = 0.0
    for it, got in zip(items, gc.run_serial(exe, tmp, items)):
        info = gc.reference(it)["info"]
        assert not info["cg_capped"] and not info["lm_capped"], it["name"]
        d, c = gc.hold_converged(it["name"], got, it)
        wd, wc = max(wd, d), max(wc, c)
        if len(it["truth"]) in (16, 48):
            ratio = gc.drift_ratio(got, it)
            print(f"{it['name']}: centre error after / before {ratio:.4f}, CG {got['cg']} against {sum(info['cg'])}")
            assert ratio <= rg.DRIFT_BOUND, it["name"]
    print(f"serial walk against optimize(), converged: nodes {wd:.3e} (recorded {rg.CONVERGED_NODES:.3e}), cost {wc:.3e} "
          f"(recorded {rg.CONVERGED_COST:.3e})")


@pytest.mark.parametrize("regime", ["flow", "converged"])
def test_weights_scaled_by_a_power_of_two(serial, regime):
    """Every weight times 4 and times 2^-4: H, g, the damping and every CG scalar scale exactly or not at all, so every node keeps
    its bits, the costs scale exactly and the counts are equal.  A walk that drops W somewhere, or applies it twice, does not.
    (graph_cases.WEIGHT_SCALES says why the powers are even.)"""
    exe, tmp = serial
    names = gc.CONVERGED_CASES if regime == "converged" else [c[0] for c in gc.LOOP_CASES if c[0] != "capacity"]
    items = [gc.loop_item(n, regime) for n in names]
    base = gc.run_serial(exe, tmp, items)
    for f in gc.WEIGHT_SCALES:
        for it, one, got in zip(items, base, gc.run_serial(exe, tmp, [gc.scaled(it, f) for it in items])):
            gc.same_under_scaled_weights(it["name"], one, got, f)
            assert got["cg"] == one["cg"], it["name"]
