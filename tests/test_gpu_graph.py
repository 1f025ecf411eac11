"""vslam_graph_optimize and vslam_world_close_loops (include/vslam_graph.h) on the device against the sanitized serial walk of
graph_math.h (tests/native/graph_serial.cpp) and tests/ref_graph.py.  The number of usable edges, the set of written nodes and
every bit outside it (the padding's sentinels included) are exact; the written nodes are held within 16 x ref_graph.DELTA_REF of the
serial walk and of the reference.  The shapes (graph_cases.SHAPES) put the 256 lanes on both sides of N and E and take several
strided passes; every one converges before either iteration cap (test_ref_graph.py asserts that).  Every graph here is consistent
(cost 0 at the minimum) and unit-weighted, and the one world scene carries a loop 2e-4 off: loops that disagree with the chain,
weights that differ, multi-edges, the capacity and both iteration caps are tests/test_gpu_graph_loops.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_cases as gc
import ref_graph as rg
import sim3_cases as sc3
from test_gpu_sim3 import W_FRAMES, W_KP, _plant, two_tracks   # the real map and world the Sim(3) tests plant reference tracks into
from vslam_amd import capi

pytestmark = pytest.mark.gpu
BOUND = 16 * rg.DELTA_REF
ARGS = ("scale", "R", "T", "fixed", "n_nodes", "edge_ab", "edge_scale", "edge_R", "edge_T", "edge_weight", "n_edges", "stats")
ALIGN = dict(scale=8, R=8, T=8, fixed=4, n_nodes=4, edge_ab=8, edge_scale=8, edge_R=8, edge_T=8, edge_weight=8, n_edges=4, stats=8)
KEYS = dict(scale="scale", R="R", T="T", fixed="fixed", edge_ab="ab", edge_scale="zs", edge_R="zR", edge_T="zt", edge_weight="zw")
SENTINEL = -7.625


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return gc.build_serial(tmp_path_factory.mktemp("graph_serial"))


def _batch(items):
    """items of any strides as one batch over the largest, the room behind each item's own stride filled with sentinels"""
    B, S, Es = len(items), max(len(it["scale"]) for it in items), max(len(it["zs"]) for it in items)
    b = dict(scale=np.full((B, S), SENTINEL), R=np.full((B, S, 9), SENTINEL), T=np.full((B, S, 3), SENTINEL), fixed=np.full((B, S), 5, np.int32),
             n_nodes=np.zeros(B, np.int32), edge_ab=np.full((B, Es, 2), -9, np.int32), edge_scale=np.full((B, Es), SENTINEL),
             edge_R=np.full((B, Es, 9), SENTINEL), edge_T=np.full((B, Es, 3), SENTINEL), edge_weight=np.full((B, Es, 3), SENTINEL),
             n_edges=np.zeros(B, np.int32), stats=np.full((B, 4), SENTINEL))
    for i, it in enumerate(items):
        s, e = len(it["scale"]), len(it["zs"])
        for kd, ki in KEYS.items():
            n = s if kd in ("scale", "R", "T", "fixed") else e
            b[kd][i, :n] = np.asarray(it[ki]).reshape(b[kd][i, :n].shape)
        b["n_nodes"][i], b["n_edges"][i] = it["n_nodes"], it["n_edges"]
    return b


def _cuda(b):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}


def _run(ctx, items, prm=None):
    b = _batch(items)
    d = _cuda(b)
    prm = dict(items[0].get("prm", {})) if prm is None else prm
    _, _, _, stats = ctx.graph_optimize(*(d[k] for k in ARGS[:11]), **prm)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got["stats"] = stats.cpu().numpy()
    out = []
    for i, it in enumerate(items):
        s = len(it["scale"])
        out.append(dict(scale=got["scale"][i, :s], R=got["R"][i, :s], T=got["T"][i, :s], stats=got["stats"][i]))
        for k in ("scale", "R", "T"):   # behind the item's own stride nothing is written
            assert gc.same_bits(got[k][i, s:], b[k][i, s:]), (i, k)
    for k in ARGS[3:11]:                # the inputs are inputs
        assert gc.same_bits(got[k], b[k]), k
    return out, got


@pytest.mark.parametrize("k", range(len(gc.SHAPES)), ids=[f"{s[0]}x{s[1]}" for s in gc.SHAPES])
def test_shapes_against_the_serial_walk_and_the_reference(ctx, exe, tmp_path, k):
    it = gc.shape_item(k)
    ser = gc.run_serial(exe, tmp_path, [it])[0]
    got = _run(ctx, [it])[0][0]
    ref = gc.reference(it)
    print(gc.SHAPES[k], "stats", got["stats"].tolist(), "serial", ser["stats"].tolist(), "reference", ref["stats"].tolist())
    assert got["stats"][0] == ref["stats"][0] == ser["stats"][0]
    gc.hold(f"{gc.SHAPES[k]} device", got, it, BOUND, against=ser)
    assert got["stats"][2] < got["stats"][1] and got["stats"][3] >= 1


def test_bits_depend_on_the_item_alone(ctx):
    it = gc.shape_item(6)   # 257 x 260
    prm = it["prm"]
    alone = _run(ctx, [it], prm)[0][0]
    again = _run(ctx, [it], prm)[0][0]
    others = [gc.shape_item(3), gc.shape_item(5), gc.hand_cases()["nan_scale"][0], it, gc.shape_item(2)]
    slot3 = _run(ctx, others, prm)[0][3]
    assert gc.written(alone, it).sum() == 257 - 9   # nodes 0, 32, ... 256 are held
    for k in ("scale", "R", "T", "stats"):
        assert gc.same_bits(alone[k], again[k]), (k, "the same item twice")
        assert gc.same_bits(alone[k], slot3[k]), (k, "alone and at slot 3 of 5")


def test_a_larger_stride_with_nan_padding(ctx, exe, tmp_path):
    N, E, seed, every = gc.SHAPES[5]
    it = gc.shape_item(5, node_stride=300, edge_stride=333)   # ref_graph.pack pads with NaN and -1
    assert np.isnan(it["scale"][N:]).all() and np.isnan(it["zs"][E:]).all()
    tight = gc.shape_item(5)
    ser = gc.run_serial(exe, tmp_path, [it])[0]
    got = _run(ctx, [it])[0][0]
    gc.hold("stride 300 x 333", got, it, BOUND, against=ser)
    same = _run(ctx, [tight])[0][0]
    for k in ("scale", "R", "T"):
        assert gc.same_bits(got[k][:N], same[k]), (k, "the stride changes no bit")
    assert gc.same_bits(got["stats"], same["stats"])


def test_hand_cases_keep_the_callers_bits(ctx, exe, tmp_path):
    cases = gc.hand_cases()
    items = [c[0] for c in cases.values()]
    sers = gc.run_serial(exe, tmp_path, items)
    gots = _run(ctx, items, gc.SHAPE_PRM)[0]   # one batch: left-alone items between moving ones
    for (name, (it, moved, use)), got, ser in zip(cases.items(), gots, sers):
        assert got["stats"][0] == use, name
        gc.hold(name, got, it, BOUND, against=ser if moved else None)
        assert gc.written(got, it).any() == moved, name
        if not moved:
            assert np.isnan(got["stats"][1:]).all(), name


def _raw(ctx, d, over=None, prm=None, **sizes):
    ptr = {k: d[k].data_ptr() for k in ARGS}
    ptr.update(over or {})
    sz = dict(batch=d["scale"].shape[0], node_stride=d["scale"].shape[1], edge_stride=d["edge_scale"].shape[1])
    sz.update(sizes)
    v = lambda k: C.c_void_p(ptr[k])
    return ctx.lib.vslam_graph_optimize(ctx.handle, v("scale"), v("R"), v("T"), v("fixed"), v("n_nodes"), sz["batch"], sz["node_stride"], v("edge_ab"),
                                        v("edge_scale"), v("edge_R"), v("edge_T"), v("edge_weight"), v("n_edges"), sz["edge_stride"],
                                        C.byref(prm) if prm is not None else C.c_void_p(0), v("stats"))


def test_invalid_arguments_are_refused_before_anything_is_queued(ctx):
    it = gc.shape_item(2)
    b = _batch([it])
    d = _cuda(b)
    for bad in (dict(max_iterations=0), dict(max_iterations=65), dict(cg_iterations=0), dict(cg_iterations=8193), dict(cg_tolerance=0.0),
                dict(cg_tolerance=1.0), dict(cg_tolerance=-1e-3), dict(cg_tolerance=float("nan"))):
        assert _raw(ctx, d, prm=capi.GraphParams.make(ctx.lib, **bad)) == -1, bad
    for k in ARGS:
        if k != "stats":
            assert _raw(ctx, d, over={k: 0}) == -1, k
    for kw in (dict(batch=0), dict(batch=-2), dict(node_stride=0), dict(node_stride=-1), dict(edge_stride=0), dict(edge_stride=-3)):
        assert _raw(ctx, d, **kw) == -1, kw
    assert _raw(ctx, d, node_stride=4097) == -4 and _raw(ctx, d, edge_stride=8193) == -4
    for k, need in ALIGN.items():   # one pointer at a time, one byte off and half its requirement off
        for off in (1, need // 2):
            assert _raw(ctx, d, over={k: d[k].data_ptr() + off}) == -1, (k, off)
            assert "d_" in ctx.lib.vslam_last_error(ctx.handle).decode()
    assert ctx.lib.vslam_graph_optimize(C.c_void_p(0), *[C.c_void_p(0)] * 5, 1, 5, *[C.c_void_p(0)] * 6, 6, C.c_void_p(0), C.c_void_p(0)) == -1
    ctx.synchronize()
    for k, v in d.items():
        assert gc.same_bits(v.cpu().numpy(), b[k]), (k, "nothing ran")
    prm = capi.GraphParams.make(ctx.lib, **it["prm"])
    assert _raw(ctx, d, prm=prm) == 0   # and the next call is the plain call's
    ctx.synchronize()
    want = _run(ctx, [it])[0][0]
    assert gc.same_bits(d["scale"].cpu().numpy()[0], want["scale"]) and gc.same_bits(d["stats"].cpu().numpy()[0], want["stats"])
    d2 = _cuda(b)                       # d_stats may be NULL
    assert _raw(ctx, d2, over=dict(stats=0), prm=prm) == 0
    ctx.synchronize()
    assert gc.same_bits(d2["T"].cpu().numpy()[0], want["T"]) and gc.same_bits(d2["stats"].cpu().numpy(), b["stats"])


def _calls(ctx, k, seed=None):
    import graph_calls as gcl
    it = gc.shape_item(k)
    if seed is not None:   # the same shape from another seed: other nodes, other loops, other measurements
        N, E, _, every = gc.SHAPES[k]
        it = dict(rg.consistent(N, E - (N - 1), seed, fixed_every=every)[0], prm=it["prm"])
    prm = capi.GraphParams.make(ctx.lib, **it["prm"])
    d = _cuda(_batch([it]))
    return {"vslam_graph_optimize": gcl.optimize({k2: d[k2] for k2 in ARGS[:11]}, prm)}, prm


def test_outputs_depend_on_the_arguments_not_on_the_workspace(ctx):
    import entry_calls as ec
    import graph_calls as gcl
    calls, keep = _calls(ctx, 4)
    assert sorted(calls) == sorted(gcl.ENTRIES)
    call = calls["vslam_graph_optimize"]
    rc, msg, first, _ = ec.run(ctx, call)
    assert rc == 0, msg
    assert np.frombuffer(first["d_stats"].tobytes(), np.float64)[0] == gc.SHAPES[4][1]
    assert "graph_workspace" in ctx.workspace_slots()
    for fill in (0x00, 0x5A, 0xFF):
        ctx.workspace_fill(fill)
        rc, msg, got, _ = ec.run(ctx, call)
        assert rc == 0 and not ec._same(first, got), (fill, ec._same(first, got))
    size = ctx.workspace_slots()["graph_workspace"]
    big = gc.shape_item(7)                            # behind a call of itself at a shape no test has run: the arena grows
    _run(ctx, [big, gc.shape_item(3), big, big])
    assert ctx.workspace_slots()["graph_workspace"] > size
    rc, msg, got, _ = ec.run(ctx, call)
    assert rc == 0 and not ec._same(first, got), ec._same(first, got)


def test_stream_order_behind_a_stalled_stream(ctx):
    """On the session's context and the stream it is bound to (torch's default stream), as tests/test_gpu_sim3.py does and for its
    reason: the test makes no stream and no context of its own."""
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    stream = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == stream
    (calls, keep), (others, keep2) = _calls(ctx, 4), _calls(ctx, 4, seed=9)
    call, other = calls["vslam_graph_optimize"], others["vslam_graph_optimize"]
    decoys = Decoys(call, other, None)
    sizing = choose_sizing(ctx, [call], stream)
    print("stream order:", sizing)
    res = run_behind_stall(ctx, call, stream, decoys, sizing)
    assert res.rc == 0, res.msg
    assert res.pending_at_return, "vslam_graph_optimize waited for the device before it returned"
    assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
    assert set(res.got) == set(res.expected)
    for k in res.expected:
        assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"


# ------------------------------------------------------------------------------------------------ on a world attached to a map
WRITTEN = (("world_Twc", "Twc"), ("world_pose", "pose"), ("world_scale", "scale"), ("world_carry", "carry"), ("world_points", "points"))


def _loops(rt):
    """a loop inside track 0 (frame 5 seen again from frame 1: the tracks' own relation, 2e-4 / 1e-4 rad / 1.5e-4 off), and rows that
    are not taken: use == 0, no such track, equal frames, a frame past the recorded ones, a NaN, a scale of 0; track 1 has no loop.
    WHY SO SMALL AN OFFSET: a loop that disagrees with the chain leaves a minimum with a cost > 0, and the schedule stops at a
    relative decrease of the cost below 2^-40, where the nodes are determined to about 1e-8 sqrt(cost) only: measured on this scene
    with a loop 4 % / 0.02 rad / 0.03 off (total cost 5e-4), the device (4 accepted steps) and ref_graph (5) ended 2.3e-10 apart
    with costs 6e-16 apart, relative.  16 x DELTA_REF relative to this scene is 5.3e-12, so the total cost has to stay below about
    1e-8; the frames still move by some 1e-5, tens of f32 steps."""
    Twc = rt["tracks"][0]["Twc"].reshape(-1, 4, 4)
    node = lambda f: (1.0, Twc[f, :3, :3], Twc[f, :3, 3])
    rng = np.random.default_rng(3)
    zs, zR, zt = rg.relative(node(5), node(1))
    good = (zs * (1.0 + 2e-4), rg.random_rotation(rng, 1e-4) @ zR, zt + 1.5e-4 * rng.normal(size=3))
    rows = [(0, 5, 1, 0, good), (0, 5, 1, 1, good), (7, 5, 1, 1, good), (-1, 5, 1, 1, good), (0, 3, 3, 1, good), (0, 6, 1, 1, good),
            (0, 2, -1, 1, good), (0, 4, 2, 1, (np.nan, good[1], good[2])), (0, 4, 2, 1, (0.0, good[1], good[2])),
            (0, 4, 0, 1, (1.0, good[1] * np.inf, good[2]))]
    return [(t, fa, fb, use, float(Z[0]), np.asarray(Z[1], np.float64).reshape(9), np.asarray(Z[2], np.float64)) for t, fa, fb, use, Z in rows]


def _close(tt, loops, **kw):
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dt)).cuda()
    stats = tt["world"].close_loops(tt["map"], dev([l[:3] for l in loops], np.int32), dev([l[4] for l in loops], np.float64),
                                    dev([l[5] for l in loops], np.float64), dev([l[6] for l in loops], np.float64),
                                    use=dev([l[3] for l in loops], np.int32), **kw)
    tt["world"].ctx.synchronize()
    return stats.cpu().numpy()


def _reference_tracks(view, obs):
    off, fr = obs[0].cpu().numpy(), obs[1].cpu().numpy()
    out = []
    for t in range(2):
        size = int(view["sizes"][t])
        anchor = np.full(view["world_points"].shape[1], -1, np.int64)
        for i in range(size):
            if off[t, i + 1] > off[t, i]:
                anchor[i] = fr[t, off[t, i]]
        out.append(dict(Twc=view["world_Twc"][t, :W_FRAMES].copy(), pose=view["world_pose"][t, :W_FRAMES].copy(),
                        scale=view["world_scale"][t, :W_FRAMES].copy(), carry=view["world_carry"][t].copy(),
                        carry_index=view["world_carry_index"][t], points=view["world_points"][t].copy(), size=size, anchor=anchor))
    return out


def test_close_loops_on_a_planted_world(ctx, two_tracks):
    tt = two_tracks
    a, wa = tt["map"], tt["world"]
    rt = sc3.ref_tracks(2)
    _plant(ctx, tt, rt)
    before = a.view()
    assert before["frames"] == W_FRAMES
    loops = _loops(rt)
    want = _reference_tracks(before, a.observations())
    anchored = [int(((w["anchor"] >= 1) & (w["anchor"] < W_FRAMES)).sum()) for w in want]
    ref_stats, ref_written = rg.close_loops(want, loops)
    stats = _close(tt, loops)
    after = a.view()
    print("stats", stats.tolist(), "reference", [s.tolist() for s in ref_stats], "points with a written anchor", anchored)
    assert anchored[0] > 0 and ref_written[0].tolist() == [False] + [True] * (W_FRAMES - 1) and not ref_written[1].any()
    assert stats[0, 0] == W_FRAMES - 1 + 1 and stats[0, 3] >= 1 and stats[0, 2] < stats[0, 1]      # five sequential edges and ONE taken loop
    assert stats[1, 0] == 0 and np.isnan(stats[1, 1:]).all()
    assert np.abs(stats[0, 1:3] - ref_stats[0][1:3]).max() <= BOUND * max(1.0, ref_stats[0][1])
    size = max(1.0, float(np.abs(before["world_Twc"][0]).max()), float(np.nanmax(np.abs(before["world_points"][0, :want[0]["size"], :3]))))
    for kd, kr in WRITTEN:
        got, ref, was = after[kd][0], want[0][kr], before[kd][0]
        got = got[:W_FRAMES] if kd in ("world_Twc", "world_pose", "world_scale") else got
        was = was[:W_FRAMES] if kd in ("world_Twc", "world_pose", "world_scale") else was
        changed_ref = np.asarray(ref).view(np.uint8).reshape(len(ref), -1) != np.asarray(was).view(np.uint8).reshape(len(was), -1)
        changed_got = np.asarray(got).view(np.uint8).reshape(len(got), -1) != np.asarray(was).view(np.uint8).reshape(len(was), -1)
        assert np.array_equal(changed_ref.any(1), changed_got.any(1)), (kd, "the rows written")   # the written / unwritten pattern
        assert changed_got.any(), kd
        worst = float(np.nanmax(np.abs(got.astype(np.float64) - ref.astype(np.float64))))
        print(f"{kd}: {worst:.3e} from the reference (bound {BOUND * size:.3e})")
        assert worst <= BOUND * size, (kd, worst)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), kd
    assert gc.same_bits(after["world_pose"][0], after["world_Twc"][0].astype(np.float32))           # the same rounded once
    assert gc.same_bits(after["world_Twc"][0][:, 12:], before["world_Twc"][0][:, 12:])             # row 3 kept
    assert gc.same_bits(after["world_points"][0][:, 3], before["world_points"][0][:, 3])           # w kept
    for k in before:   # everything else, the loop-less track and every array of the map keep their bits
        if not isinstance(before[k], np.ndarray):
            continue
        if k in [w[0] for w in WRITTEN]:
            assert gc.same_bits(after[k][1], before[k][1]), (k, "track 1 has no loop")
        else:
            assert gc.same_bits(after[k], before[k]), (k, "not the call's to write")
    # the loop now closes: its residual under the result is far below the one under the start
    assert stats[0, 2] < 0.5 * stats[0, 1]
    # refusals, as vslam_world_adjust's
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dt)).cuda()
    one = [dev([0], np.int32), dev([5], np.int32), dev([1], np.int32), dev([1], np.int32), dev([1.0], np.float64), dev(np.eye(3).reshape(1, 9), np.float64),
           dev(np.zeros((1, 3)), np.float64)]
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda world=wa.handle, n=1, args=None: ctx.lib.vslam_world_close_loops(ctx.handle, world, a.handle, *(args or [p(t) for t in one]), n,
                                                                                   C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
    other = capi.World(ctx, 2, W_FRAMES, W_KP)
    assert call(world=other.handle) == -1 and call(n=0) == -1 and call(n=-1) == -1
    other.close()
    for i in range(7):
        args = [p(t) for t in one]
        args[i] = C.c_void_p(one[i].data_ptr() + (4 if i >= 4 else 2))
        assert call(args=args) == -1, i
        args[i] = C.c_void_p(0)
        assert call(args=args) == -1, i
    ctx.synchronize()
    again = a.view()
    for k in after:
        if isinstance(after[k], np.ndarray):
            assert gc.same_bits(again[k], after[k]), (k, "a refused call writes nothing")
    wa.reset()   # reset undoes it
    ctx.synchronize()
    z = wa.view()
    assert np.array_equal(z["Twc"][0, 0], np.eye(4).reshape(16)) and (z["scale"] == 1.0).all()


def test_close_loops_leaves_absorbed_rows_nan(ctx, two_tracks):
    tt = two_tracks
    a, wa = tt["map"], tt["world"]
    rt = sc3.ref_tracks(2)
    _plant(ctx, tt, rt)
    fstats = wa.fuse(a).cpu().numpy()
    ctx.synchronize()
    before = a.view()
    nan_rows = np.isnan(before["world_points"][0, :, 0])
    print("fusion:", fstats.tolist(), "absorbed rows of track 0:", int(nan_rows.sum()))
    stats = _close(tt, _loops(rt))
    after = a.view()
    assert stats[0, 3] >= 1
    assert np.array_equal(np.isnan(after["world_points"][0, :, 0]), nan_rows)
    assert gc.same_bits(after["world_points"][0][nan_rows], before["world_points"][0][nan_rows])
    want = _reference_tracks(before, a.observations())
    rg.close_loops(want, _loops(rt))
    size = max(1.0, float(np.nanmax(np.abs(before["world_points"][0, :want[0]["size"], :3]))))
    assert np.nanmax(np.abs(after["world_points"][0].astype(np.float64) - want[0]["points"].astype(np.float64))) <= BOUND * size
