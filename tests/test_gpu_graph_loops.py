"""vslam_graph_optimize and vslam_world_close_loops (include/vslam_graph.h) on the device where loops disagree with the chain and
the weights differ per edge and per group (graph_cases.LOOP_CASES): minima with cost > 0, a hub whose degree spans three chunks of
the adjacency fill, multi-edges, VSLAM_GRAPH_MAX_NODES x VSLAM_GRAPH_MAX_EDGES, and both iteration caps.

Two regimes.  Under a FIXED FLOW (ref_graph.FLOW: cg_tolerance = 1e-30 and small caps) every solve runs exactly cg_iterations and
the outer loop exactly max_iterations, so the device, the serial walk and the reference differ by rounding alone and are held
within 16 x ref_graph.DELTA_FLOW -- a number measured on the CPU between the reference and the serial walk, never on the device.
Run to CONVERGENCE the flows may part and the bound is the coarse one (CONVERGED_NODES, CONVERGED_COST), measured the same way."""
import numpy as np
import pytest

import graph_cases as gc
import ref_graph as rg
import sim3_cases as sc3
from test_gpu_graph import WRITTEN, _close, _reference_tracks, _run, exe   # noqa: F401  (exe: the serial walk, built once per module)
from test_gpu_sim3 import W_FRAMES, _plant, two_tracks                     # noqa: F401

pytestmark = pytest.mark.gpu
FLOW_BOUND = 16 * rg.DELTA_FLOW


# ------------------------------------------------------------------------------------------------ vslam_graph_optimize
@pytest.mark.parametrize("name", [c[0] for c in gc.LOOP_CASES])
def test_fixed_flow_against_the_serial_walk_and_the_reference(ctx, exe, tmp_path, name):
    it = gc.loop_item(name)
    ser = gc.run_serial(exe, tmp_path, [it])[0]
    got = _run(ctx, [it])[0][0]
    print(name, "stats", got["stats"].tolist(), "serial", ser["stats"].tolist(), "reference", gc.reference(it)["stats"].tolist())
    assert ser["cg"] == it["prm"]["max_iterations"] * it["prm"]["cg_iterations"]
    gc.hold_flow(f"{name} device", got, it, against=ser)
    if name == "capacity":   # once more behind a small item: the second workspace starts 7.2 MB in
        small = dict(gc.loop_item("drift16"), prm=it["prm"])
        both = _run(ctx, [small, it])[0]
        gc.hold_flow(f"{name} device, slot 1 of 2", both[1], it, against=ser)
        gc.hold_flow("drift16 under capacity's flow, slot 0 of 2", both[0], small)
        for k in ("scale", "R", "T", "stats"):
            assert gc.same_bits(both[1][k], got[k]), (k, "alone and at slot 1 of 2")


@pytest.mark.parametrize("name", gc.CONVERGED_CASES)
def test_converged_against_the_serial_walk_and_the_reference(ctx, exe, tmp_path, name):
    it = gc.loop_item(name, "converged")
    ser = gc.run_serial(exe, tmp_path, [it])[0]
    got = _run(ctx, [it])[0][0]
    info = gc.reference(it)["info"]
    print(name, "stats", got["stats"].tolist(), "serial", ser["stats"].tolist(), "CG", ser["cg"], "reference", gc.reference(it)["stats"].tolist(),
          "CG", sum(info["cg"]))
    gc.hold_converged(f"{name} device", got, it, against=ser)
    assert got["stats"][2] < got["stats"][1]
    if name in gc.DRIFT_LOOPS:
        ratio = gc.drift_ratio(got, it)
        print(f"{name}: centre error after / before {ratio:.4f}")
        assert ratio <= rg.DRIFT_BOUND


@pytest.mark.parametrize("regime", ["flow", "converged"])
def test_weights_scaled_by_a_power_of_two(ctx, regime):
    """Every weight times 4 and times 2^-4 (graph_cases.WEIGHT_SCALES): every node keeps every bit, the costs scale exactly, the
    counts are equal.  A kernel that leaves W out of H, g or the operator, or applies it twice, cannot do that."""
    names = gc.CONVERGED_CASES if regime == "converged" else [c[0] for c in gc.LOOP_CASES if c[0] != "capacity"]
    for name in names:
        it = gc.loop_item(name, regime)
        one = _run(ctx, [it])[0][0]
        assert one["stats"][3] >= 1
        for f in gc.WEIGHT_SCALES:
            gc.same_under_scaled_weights(f"{name} {regime}", one, _run(ctx, [gc.scaled(it, f)])[0][0], f)


@pytest.mark.parametrize("regime", ["flow", "converged"])
def test_bits_depend_on_the_item_alone(ctx, regime):
    """a drift item and the hub (three fill chunks at one node: the carry in `fill` and the ranks inside a chunk) alone, twice, and
    at two slots each of a batch that also holds an item that is left alone"""
    prm = dict(rg.FLOW, max_iterations=3, cg_iterations=2) if regime == "flow" else dict(rg.CONVERGED)
    drift, hub, alone_item = gc.loop_item("drift48"), gc.loop_item("hub"), gc.hand_cases()["nan_scale"][0]
    batch = [drift, alone_item, hub, hub, drift]
    mixed = _run(ctx, batch, prm)[0]
    assert np.isnan(mixed[1]["stats"][1:]).all() and not gc.written(mixed[1], alone_item).any()
    for it, slots in ((drift, (0, 4)), (hub, (2, 3))):
        alone, again = _run(ctx, [it], prm)[0][0], _run(ctx, [it], prm)[0][0]
        assert alone["stats"][3] >= 1 and gc.written(alone, it).sum() == (47 if it is drift else 7)
        for k in ("scale", "R", "T", "stats"):
            assert gc.same_bits(alone[k], again[k]), (k, "the same item twice")
            for s in slots:
                assert gc.same_bits(alone[k], mixed[s][k]), (k, f"alone and at slot {s} of 5")


# ------------------------------------------------------------------------------------------------ vslam_world_close_loops
SEQ_WEIGHT, LOOP_WEIGHT = (4.0, 1.0, 0.5), (0.25, 2.0, 8.0)
WORLD_FLOW = dict(rg.FLOW, max_iterations=3, cg_iterations=2)   # the conditions of a fixed flow are asserted on the reference below


def _model(rt, t, fa, fb, rng):
    """the track's own relation of two frames, 4 % / 0.02 rad / 0.03 off"""
    Twc = rt["tracks"][t]["Twc"].reshape(-1, 4, 4)
    node = lambda f: (1.0, Twc[f, :3, :3], Twc[f, :3, 3])
    zs, zR, zt = rg.relative(node(fa), node(fb))
    d = rng.normal(size=3)
    return zs * (1.0 + 0.04 * rng.choice([-1.0, 1.0])), rg.random_rotation(rng, 0.02) @ zR, zt + 0.03 * d / np.linalg.norm(d)


def _row(t, fa, fb, use, Z):
    return (t, fa, fb, use, float(Z[0]), np.asarray(Z[1], np.float64).reshape(9), np.asarray(Z[2], np.float64))


def _hold_world(before, after, want, ref_stats, ref_written, stats, prm):
    """the device's world against ref_graph.close_loops' (`want`, changed in place by it): the integers exact, the costs and every
    written array within 16 x DELTA_FLOW relative to the scene's size, the written / unwritten pattern, every other bit kept"""
    for t in range(2):
        if not ref_written[t].any():
            assert stats[t, 0] == 0 and np.isnan(stats[t, 1:]).all(), t
            for kd, _ in WRITTEN:
                assert gc.same_bits(after[kd][t], before[kd][t]), (kd, f"track {t} has no loop")
            continue
        assert ref_written[t].tolist() == [False] + [True] * (W_FRAMES - 1)
        assert stats[t, 0] == ref_stats[t][0] and stats[t, 3] == ref_stats[t][3] == prm["max_iterations"], (t, stats[t].tolist())
        assert stats[t, 2] < stats[t, 1]
        assert np.abs(stats[t, 1:3] - ref_stats[t][1:3]).max() <= FLOW_BOUND * max(1.0, ref_stats[t][1]), (t, stats[t].tolist(), ref_stats[t].tolist())
        size = max(1.0, float(np.abs(before["world_Twc"][t]).max()), float(np.nanmax(np.abs(before["world_points"][t, :want[t]["size"], :3]))))
        for kd, kr in WRITTEN:
            got, ref, was = after[kd][t], want[t][kr], before[kd][t]
            got = got[:W_FRAMES] if kd in ("world_Twc", "world_pose", "world_scale") else got
            was = was[:W_FRAMES] if kd in ("world_Twc", "world_pose", "world_scale") else was
            changed_ref = np.asarray(ref).view(np.uint8).reshape(len(ref), -1) != np.asarray(was).view(np.uint8).reshape(len(was), -1)
            changed_got = np.asarray(got).view(np.uint8).reshape(len(got), -1) != np.asarray(was).view(np.uint8).reshape(len(was), -1)
            assert np.array_equal(changed_ref.any(1), changed_got.any(1)), (t, kd, "the rows written")
            assert changed_got.any(), (t, kd)
            worst = float(np.nanmax(np.abs(got.astype(np.float64) - ref.astype(np.float64))))
            print(f"track {t} {kd}: {worst:.3e} from the reference (bound {FLOW_BOUND * size:.3e})")
            assert worst <= FLOW_BOUND * size, (t, kd, worst)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (t, kd)
        assert gc.same_bits(after["world_pose"][t], after["world_Twc"][t].astype(np.float32))
        assert gc.same_bits(after["world_Twc"][t][:, 12:], before["world_Twc"][t][:, 12:])
        assert gc.same_bits(after["world_points"][t][:, 3], before["world_points"][t][:, 3])
    for k in before:
        if isinstance(before[k], np.ndarray) and k not in [w[0] for w in WRITTEN]:
            assert gc.same_bits(after[k], before[k]), (k, "not the call's to write")


def _fixed_flow_held(infos, prm):
    for info in infos:
        assert info["moved"] and info["steps"] == info["accepted"] == prm["max_iterations"]
        assert info["cg"] == [prm["cg_iterations"]] * prm["max_iterations"] and min(info["cg_ratio"]) >= rg.FLOW_RATIO, info["cg_ratio"]


def test_close_loops_weighted_on_both_tracks_across_gather_chunks(ctx, two_tracks):
    """Two loops on track 0 and one on track 1, 4 % / 0.02 rad / 0.03 off, under seq_weight and loop_weight that differ in every
    group, in a list of 600 rows: the taken ones in the gather's chunks 0, 1 and 2, every other row not taken by one of the rules."""
    tt = two_tracks
    a = tt["map"]
    rt = sc3.ref_tracks(2)
    _plant(ctx, tt, rt)
    before = a.view()
    rng = np.random.default_rng(11)
    taken = {7: (0, 5, 1), 300: (1, 4, 0), 599: (0, 2, 4)}
    some = _model(rt, 0, 5, 1, rng)
    not_taken = [(0, 5, 1, 0, some), (7, 5, 1, 1, some), (-1, 5, 1, 1, some), (2, 5, 1, 1, some), (0, 3, 3, 1, some), (1, 6, 1, 1, some),
                 (0, 2, -1, 1, some), (1, 4, 2, 1, (np.nan, some[1], some[2])), (0, 4, 2, 1, (0.0, some[1], some[2])),
                 (0, 4, 2, 1, (-1.0, some[1], some[2])), (1, 4, 0, 1, (1.0, some[1] * np.inf, some[2])), (0, 1, 3, 1, (1.0, some[1], some[2] * np.nan))]
    loops = [_row(*not_taken[k % len(not_taken)]) if k not in taken else _row(*taken[k], 1, _model(rt, *taken[k], rng)) for k in range(600)]
    assert sorted(k // 256 for k in taken) == [0, 1, 2]
    want = _reference_tracks(before, a.observations())
    infos = []
    ref_stats, ref_written = rg.close_loops(want, loops, SEQ_WEIGHT, LOOP_WEIGHT, infos=infos, **WORLD_FLOW)
    _fixed_flow_held(infos, WORLD_FLOW)
    assert len(infos) == 2 and ref_stats[0][0] == W_FRAMES - 1 + 2 and ref_stats[1][0] == W_FRAMES - 1 + 1
    assert min(s[2] for s in ref_stats) > 1e-6   # the loops disagree with the chain: the minimum costs > 0
    stats = _close(tt, loops, seq_weight=SEQ_WEIGHT, loop_weight=LOOP_WEIGHT, **WORLD_FLOW)
    print("stats", stats.tolist(), "reference", [s.tolist() for s in ref_stats])
    _hold_world(before, a.view(), want, ref_stats, ref_written, stats, WORLD_FLOW)
    # the weights are told apart: under the two swapped the reference ends far outside the bound
    other = _reference_tracks(before, a.observations())
    rg.close_loops(other, loops, LOOP_WEIGHT, SEQ_WEIGHT, **WORLD_FLOW)
    assert np.abs(other[0]["Twc"] - want[0]["Twc"]).max() > 1e6 * FLOW_BOUND


def test_close_loops_takes_the_first_loops_that_fit(ctx, two_tracks):
    """8200 taken rows on the 6-frame track 0: VSLAM_GRAPH_MAX_EDGES - 5 of them fit, in list order.  Row 8187 is the first that
    does not: with a wildly different model there, every output keeps its bits."""
    tt = two_tracks
    a = tt["map"]
    rt = sc3.ref_tracks(2)
    rng = np.random.default_rng(12)
    room = rg.MAX_EDGES - (W_FRAMES - 1)
    loops = []
    for k in range(8200):
        fa, fb = (int(v) for v in rng.choice(W_FRAMES, 2, replace=False))
        loops.append(_row(0, fa, fb, 1, _model(rt, 0, fa, fb, rng)))
    wild = list(loops)
    wild[room] = _row(0, 5, 0, 1, (3.0, rg.random_rotation(rng, 2.0), np.array([40.0, -30.0, 20.0])))
    views = []
    for rows in (loops, wild):
        _plant(ctx, tt, rt)
        before = a.view()
        stats = _close(tt, rows, seq_weight=SEQ_WEIGHT, loop_weight=LOOP_WEIGHT, **WORLD_FLOW)
        views.append((before, a.view(), stats))
    before, after, stats = views[0]
    assert stats[0, 0] == rg.MAX_EDGES and stats[1, 0] == 0
    want = _reference_tracks(before, a.observations())
    infos = []
    ref_stats, ref_written = rg.close_loops(want, loops, SEQ_WEIGHT, LOOP_WEIGHT, infos=infos, **WORLD_FLOW)
    _fixed_flow_held(infos, WORLD_FLOW)
    assert ref_stats[0][0] == rg.MAX_EDGES
    print("stats", stats.tolist(), "reference", [s.tolist() for s in ref_stats])
    _hold_world(before, after, want, ref_stats, ref_written, stats, WORLD_FLOW)
    # the row is one that would tell: taken in place of row 8186, the reference moves
    moved = _reference_tracks(before, a.observations())
    swapped = list(loops)
    swapped[room - 1] = wild[room]
    rg.close_loops(moved, swapped, SEQ_WEIGHT, LOOP_WEIGHT, **WORLD_FLOW)
    assert np.abs(moved[0]["Twc"] - want[0]["Twc"]).max() > 1e3 * FLOW_BOUND
    for k in after:
        if isinstance(after[k], np.ndarray):
            assert gc.same_bits(views[1][0][k], before[k]), (k, "planted alike")
            assert gc.same_bits(views[1][1][k], after[k]), (k, "a row behind the room changed the result")
    assert gc.same_bits(views[1][2], stats)
