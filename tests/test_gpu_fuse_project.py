"""vslam_fuse_project and vslam_world_fuse_project (include/vslam_fuse_project.h) on the device, bit for bit against
tests/ref_fuse_project.py: every hand case and random item of tests/fuse_project_cases.py alone and in batches of three, items moved
between slots, slots from n_found on keeping the caller's fill; the refusals; the alignment, workspace and stream-order contracts
through the Call of tests/fuse_project_calls.py, as tests/test_gpu_graph.py applies them; and the call on a world attached to a real
map, against the reference run on the state read back before the call."""
import ctypes as C

import numpy as np
import pytest
import torch

import fuse_project_calls as fcl
import fuse_project_cases as fpc
import pnp_cases as pc
import ref_fuse as rf
import ref_fuse_project as rfp
from vslam_amd import capi

pytestmark = pytest.mark.gpu
FILL = -77
OUT_KEYS = rfp.OUTS + ("n_found", "stats")
IN_KEYS = ("points", "n", "offsets", "cam", "kp", "obs_desc", "R", "T", "n_cams", "xy", "desc", "n_kp")


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _prefill(B, Fs):
    p = {k: np.full((B, Fs), FILL, np.int32) for k in rfp.OUTS}
    p.update(n_found=np.full(B, FILL, np.int32), stats=np.full((B, 6), FILL, np.int32))
    return p


def _run(ctx, items, found_stride, params=None):
    """the items as one batch on the device over the fill, held to the reference on the same stacked arrays -> the outputs (numpy)"""
    params = params or {}
    b = rfp.batch_of(items)
    if all(it.get("cam_mask") is None for it in items):
        b["cam_mask"] = None                       # d_cam_mask == NULL
    d = {k: _t(v) for k, v in b.items() if v is not None}
    B = len(items)
    out = {k: _t(v) for k, v in _prefill(B, found_stride).items()}
    it0 = items[0]
    o = ctx.fuse_project(*(d[k] for k in IN_KEYS), it0["K"], it0["width"], it0["height"], cam_mask=d.get("cam_mask"), found_stride=found_stride,
                         out=out, **params)
    ctx.synchronize()
    got = {k: o[k].cpu().numpy() for k in OUT_KEYS}
    ref = rfp.project_batch(b, it0["K"], it0["width"], it0["height"], found_stride, prefill=_prefill(B, found_stride), **params)
    for k in OUT_KEYS:
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k, v in d.items():
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(b[k])), (k, "an input is an input")
    return got


def _item_bits(got, b):
    m = int(got["n_found"][b])
    return [got[k][b, :m].tolist() for k in rfp.OUTS] + [got["stats"][b].tolist()]


def test_hand_cases_alone_and_in_batches_of_three(ctx):
    cases = fpc.hand_cases()
    plain = []
    for name, c in cases.items():
        fs = c["found_stride"] or 8
        got = _run(ctx, [c], fs, c["params"])
        found = list(zip(*(got[k][0, :got["n_found"][0]].tolist() for k in rfp.OUTS)))
        assert found == c["expect"], (name, found)
        if c["expect_stats"] is not None:
            assert np.array_equal(got["stats"][0], c["expect_stats"]), (name, got["stats"][0])
        if not c["params"] and c["found_stride"] is None:
            plain.append(name)
    assert len(plain) >= 24
    for j in range(0, len(plain) - 2, 3):      # three neighbours share a batch: padded to the largest strides, every item with a mask
        _run(ctx, [cases[n] for n in plain[j:j + 3]], 8)


def test_random_items_alone_in_threes_and_moved_between_slots(ctx):
    cases = fpc.random_cases()
    for name, c in cases.items():
        got = _run(ctx, [c], 4 * c["n"], c.get("params"))
        s = got["stats"][0]
        print(f"{name}: tried {s[0]}, visible {s[1]}, proposing {s[2]}, found {s[3]}, with a holder {s[4]}")
        assert c["n"] < 255 or (s[3] > 0 and s[4] > 0)
        if c["n"] >= 255:                          # found_stride one below the number found
            short = _run(ctx, [c], int(s[3]) - 1, c.get("params"))
            assert short["n_found"][0] == s[3] - 1 and short["stats"][0].tolist() == s[:5].tolist() + [s[3] - 1]
    a, b, c = cases["n600c9"], cases["n257c2"], cases["n256c9"]
    first = _run(ctx, [a, b, c], 1200)
    again = _run(ctx, [a, b, c], 1200)
    moved = _run(ctx, [c, a, b], 1200)
    two = _run(ctx, [b, a], 1200)                  # other strides around b: its bits stay the item's own
    for s0, s1 in ((0, 1), (1, 2), (2, 0)):
        assert _item_bits(first, s0) == _item_bits(moved, s1) == _item_bits(again, s0), (s0, s1)
    assert _item_bits(two, 1) == _item_bits(first, 0)
    alone = _run(ctx, [cases["n257c2"]], 1200)
    assert _item_bits(alone, 0)[:4] == _item_bits(first, 1)[:4]    # the mask differs (NULL / zeros), the rule does not


# ------------------------------------------------------------------------------------------------ refusals and contracts
def _raw(ctx, d, outs, over=None, prm=None, K=None, **sizes):
    ptr = {name: d[key].data_ptr() for name, key in fcl.INS.items()}
    ptr.update({"d_" + k: v.data_ptr() for k, v in outs.items()})
    ptr.update(over or {})
    sz = dict(batch=d["points"].shape[0], pt_stride=d["points"].shape[1], obs_stride=d["cam"].shape[1], cam_stride=d["R"].shape[1],
              kp_stride=d["xy"].shape[2], found_stride=outs["found_point"].shape[1], width=640, height=480)
    sz.update(sizes)
    K = np.ascontiguousarray(fpc.K.reshape(9)) if K is None else K
    v = lambda k: C.c_void_p(ptr[k])
    return ctx.lib.vslam_fuse_project(
        ctx.handle, v("d_points"), v("d_n_points"), sz["pt_stride"], v("d_obs_offsets"), v("d_obs_cam"), v("d_obs_kp"), v("d_obs_desc"), sz["obs_stride"],
        v("d_R"), v("d_T"), v("d_n_cams"), sz["cam_stride"], v("d_xy"), v("d_desc"), v("d_n_kp"), sz["kp_stride"], v("d_cam_mask"),
        K.ctypes.data_as(C.c_void_p) if K is not False else C.c_void_p(0), sz["width"], sz["height"], sz["batch"],
        C.byref(prm) if prm is not None else C.c_void_p(0), v("d_found_point"), v("d_found_cam"), v("d_found_kp"), v("d_found_dist"),
        v("d_found_holder"), sz["found_stride"], v("d_n_found"), v("d_stats"))


def test_invalid_arguments_are_refused_before_anything_is_queued(ctx):
    c = fpc.random_cases()["n255c2"]
    b = rfp.batch_of([c])
    d = {k: _t(v) for k, v in b.items()}
    fill = _prefill(1, 600)
    outs = {k: _t(v) for k, v in fill.items()}
    for bad in (dict(radius_px=0.0), dict(radius_px=-1.0), dict(radius_px=64.5), dict(radius_px=float("nan")), dict(radius_px=float("inf")),
                dict(dist_threshold=0), dict(dist_threshold=258), dict(ratio10=-1), dict(ratio10=11)):
        assert _raw(ctx, d, outs, prm=capi.SearchParams.make(ctx.lib, **bad)) == -1, bad
    for k in fcl.ALIGN:
        if k not in fcl.OPTIONAL:
            assert _raw(ctx, d, outs, over={k: 0}) == -1, k
    assert _raw(ctx, d, outs, K=False) == -1
    Kbad = np.ascontiguousarray(fpc.K.reshape(9)).copy()
    Kbad[4] = np.inf
    assert _raw(ctx, d, outs, K=Kbad) == -1
    for name in ("batch", "pt_stride", "obs_stride", "cam_stride", "kp_stride", "found_stride", "width", "height"):
        for v in (0, -2):
            assert _raw(ctx, d, outs, **{name: v}) == -1, (name, v)
    assert _raw(ctx, d, outs, kp_stride=16385) == -4 and _raw(ctx, d, outs, cam_stride=1025) == -4 and _raw(ctx, d, outs, batch=65536) == -4
    assert _raw(ctx, d, outs, width=16385) == -4 and _raw(ctx, d, outs, height=16385) == -4
    for k, need in fcl.ALIGN.items():             # one pointer at a time, one byte off and half its requirement off
        base = (d[fcl.INS[k]] if k in fcl.INS else outs[k[2:]]).data_ptr()
        for off in (1, need // 2):
            assert _raw(ctx, d, outs, over={k: base + off}) == -1, (k, off)
            assert "d_" in ctx.lib.vslam_last_error(ctx.handle).decode()
    ctx.synchronize()
    for k, v in outs.items():
        assert np.array_equal(v.cpu().numpy(), fill[k]), (k, "nothing ran")
    assert _raw(ctx, d, outs) == 0                 # and the next call is the plain call's
    ctx.synchronize()
    want = _run(ctx, [c], 600)
    for k in OUT_KEYS:
        assert np.array_equal(outs[k].cpu().numpy(), want[k]), k
    outs2 = {k: _t(v) for k, v in fill.items()}   # d_stats and d_cam_mask may be NULL
    assert _raw(ctx, d, outs2, over=dict(d_stats=0, d_cam_mask=0)) == 0
    ctx.synchronize()
    assert np.array_equal(outs2["found_kp"].cpu().numpy(), want["found_kp"]) and np.array_equal(outs2["stats"].cpu().numpy(), fill["stats"])


def _calls(ctx, name, other=False):
    """the Call of one random item, or (other) of the same shape from another seed, both padded to common strides"""
    c = fpc.random_cases()[name]
    c2 = rfp.random_item(77, c["n"], c["n_cams"], kp_stride=c["xy"].shape[1], cam_stride=len(c["R"]), S=len(c["points"]))
    j = 1 if other else 0
    d = {k: _t(v[j:j + 1]) for k, v in rfp.batch_of([c, c2]).items()}
    return fcl.fuse_project(d, c["K"], c["width"], c["height"], 4 * c["n"])


def test_outputs_depend_on_the_arguments_not_on_the_workspace(ctx):
    import entry_calls as ec
    call = _calls(ctx, "n256c9")
    assert [call.entry] == fcl.ENTRIES
    rc, msg, first, _ = ec.run(ctx, call)
    assert rc == 0, msg
    assert np.frombuffer(first["d_stats"].tobytes(), np.int32)[3] > 0
    slots = ctx.workspace_slots()
    S, O, Cs, Kp = 259, None, 10, 96
    assert slots["fuse_project_cells"] >= Cs * Kp * 12 and slots["fuse_project_work"] >= (Cs * S + Cs * 8 + 1) * 4
    for fill in (0x00, 0x5A, 0xFF):
        ctx.workspace_fill(fill)
        rc, msg, got, _ = ec.run(ctx, call)
        assert rc == 0 and not ec._same(first, got), (fill, ec._same(first, got))
    size = ctx.workspace_slots()["fuse_project_work"]
    big = fpc.random_cases()["n600c9"]             # behind a call of itself at a batch no test has run: the arena grows
    _run(ctx, [big] * 5, 1200)
    assert ctx.workspace_slots()["fuse_project_work"] > size
    rc, msg, got, _ = ec.run(ctx, call)
    assert rc == 0 and not ec._same(first, got), ec._same(first, got)
    size = ctx.workspace_slots()
    ec.run(ctx, call)
    assert ctx.workspace_slots() == size, "nothing is allocated after the first call of a size"


def test_stream_order_behind_a_stalled_stream(ctx):
    """On the session's context and the stream it is bound to (torch's default stream), as tests/test_gpu_graph.py does: the test
    makes no stream and no context of its own."""
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    stream = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == stream
    call, other = _calls(ctx, "n256c9"), _calls(ctx, "n256c9", other=True)
    decoys = Decoys(call, other, None)
    sizing = choose_sizing(ctx, [call], stream)
    print("stream order:", sizing)
    res = run_behind_stall(ctx, call, stream, decoys, sizing)
    assert res.rc == 0, res.msg
    assert res.pending_at_return, "vslam_fuse_project waited for the device before it returned"
    assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
    assert set(res.got) == set(res.expected)
    for k in res.expected:
        assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"


# ------------------------------------------------------------------------------------------------ on the world
from test_gpu_pnp import SCENE_KP, SCENE_MCAP, SCENE_OCAP, _put, _scene_map  # noqa: E402


def _np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _keypoints(scenes, frames=6, kp=SCENE_KP):
    T = len(scenes)
    xy, desc = np.zeros((T, frames, kp, 2), np.float32), np.zeros((T, frames, kp, 32), np.uint8)
    n_kp = np.zeros((T, frames), np.int32)
    for t, ws in enumerate(scenes):
        for f in range(frames):
            xy[t, f, :ws["n"]], desc[t, f, :ws["n"]], n_kp[t, f] = ws["xy"][f], ws["desc"][f], ws["n"]
    return xy, desc, n_kp


def _state(a, wa):
    """everything the reference of the world call reads, read back from the device"""
    v = a.view()
    off, fr, kp = _np(a.observations())
    _, mdesc = _np(a.observation_descriptors())
    ex = v.get("world_extra")
    T = len(v["sizes"])
    extras = [np.zeros((0, 3), np.int64)] * T if ex is None else [np.stack([ex[k][t, :ex["n"][t]] for k in ("point", "frame", "kp")], 1) for t in range(T)]
    edesc = [np.zeros((0, 32), np.uint8)] * T if ex is None else [ex["desc"][t, :ex["n"][t]] for t in range(T)]
    return dict(view=v, off=off, fr=fr, kp=kp, mdesc=mdesc, extras=extras, edesc=edesc)


def _reference(st, t, xy, desc, n_kp, K, W, H, lo, hi, frames, max_frames, kp_stride, obs_capacity, **kw):
    v = st["view"]
    fuse_to = v["world_fuse_to"][t] if "world_fuse_to" in v else None
    return rfp.world_fuse_project(fuse_to, v["world_points"][t], v["sizes"][t], st["off"][t], st["fr"][t], st["kp"][t], st["mdesc"][t], st["extras"][t],
                                  st["edesc"][t], v["world_Twc"][t], frames, xy[t], desc[t], n_kp[t], K, W, H, lo, hi, max_frames, kp_stride,
                                  obs_capacity, **kw)


def _hold_world(a, wa, st, refs, stats, what):
    """the state after a call against the references of every track: d_fuse_to, the log, the NaN rows, the statistics and the world's
    CSR with its descriptors afterwards"""
    after = a.view()
    off, fr, kp, desc = _np(wa.observations(a))
    for t, r in enumerate(refs):
        assert np.array_equal(stats[t], r["stats"]), (what, t, stats[t], r["stats"])
        assert np.array_equal(after["world_fuse_to"][t], r["fuse_to"]), (what, t)
        assert np.array_equal(_bits(after["world_points"][t]), _bits(r["world_points"])), (what, t, "NaN rows for the newly absorbed only")
        ex, m = after["world_extra"], len(r["extras"])
        assert ex["n"][t] == m, (what, t, ex["n"][t], m)
        for j, k in enumerate(("point", "frame", "kp")):
            assert np.array_equal(ex[k][t, :m], r["extras"][:, j]), (what, t, k)
        assert np.array_equal(ex["desc"][t, :m], r["extra_desc"]), (what, t)
        csr, cdesc = rfp.world_csr(r["fuse_to"], after["sizes"][t], st["off"][t], st["fr"][t], st["kp"][t], st["mdesc"][t], r["extras"], r["extra_desc"],
                                   after["world_Twc"].shape[1], wa.kp_stride, a.obs_capacity)
        total = len(csr["out_cam"])
        assert np.array_equal(off[t], csr["out_offsets"]), (what, t)
        assert np.array_equal(fr[t, :total], csr["out_cam"]) and np.array_equal(kp[t, :total], csr["out_kp"]), (what, t)
        assert (fr[t, total:] == -1).all() and np.array_equal(desc[t, :total], cdesc) and not desc[t, total:].any(), (what, t)
    keep = [k for k in st["view"] if k not in ("world_points", "world_fuse_to", "world_extra")]
    for k in keep:                                 # every array of the map and the rest of the world
        assert np.array_equal(_bits(after[k]), _bits(st["view"][k])), (what, k)
    return after


def test_world_fuse_project_on_a_stepped_map_of_two_tracks(ctx):
    seed, ws0 = pc.first_world_scene(60)
    _, ws1 = pc.first_world_scene(60, seeds=range(seed + 1, 4000))
    scenes = [ws0, ws1]
    a, wa, cur = _scene_map(ctx, scenes)
    try:
        xy, desc, n_kp = _keypoints(scenes)
        K, W, H = pc.SCENE_K, pc.SCENE_W, pc.SCENE_H
        dims = dict(frames=6, max_frames=6, kp_stride=SCENE_KP, obs_capacity=SCENE_OCAP)
        wa.fuse(a)
        ctx.synchronize()
        st = _state(a, wa)
        assert "world_extra" not in st["view"] and "world_fuse_to" in st["view"]
        live0 = [(st["view"]["world_fuse_to"][t] == np.arange(SCENE_MCAP))[:st["view"]["sizes"][t]].sum() for t in range(2)]
        stats = wa.fuse_project(a, _t(xy), _t(desc), _t(n_kp), K, W, H).cpu().numpy()
        ctx.synchronize()
        refs = [_reference(st, t, xy, desc, n_kp, K, W, H, 0, 6, **dims) for t in range(2)]
        after = _hold_world(a, wa, st, refs, stats, "first call")
        live1 = [(after["world_fuse_to"][t] == np.arange(SCENE_MCAP))[:after["sizes"][t]].sum() for t in range(2)]
        print("stats", stats.tolist(), "live points", [int(x) for x in live0], "->", [int(x) for x in live1])
        assert all(l1 < l0 for l0, l1 in zip(live0, live1)) and (stats[:, 4] > 0).all() and (stats[:, 3] > stats[:, 4]).all()
        assert np.array_equal(stats[:, 6], stats[:, 5]) and np.array_equal(stats[:, 7], stats[:, 6])
        fv, state = C.c_void_p(), C.c_int32()
        ctx._check(ctx.lib.vslam_world_fusion_view(wa.handle, C.byref(fv), C.byref(state)))
        assert state.value == 5, "bit 0: fused, bit 2: extras exist"
        # a second call appends nothing: every pair is now skipped or already united
        st2 = _state(a, wa)
        stats2 = wa.fuse_project(a, _t(xy), _t(desc), _t(n_kp), K, W, H).cpu().numpy()
        ctx.synchronize()
        refs2 = [_reference(st2, t, xy, desc, n_kp, K, W, H, 0, 6, **dims) for t in range(2)]
        _hold_world(a, wa, st2, refs2, stats2, "second call")
        print("second call", stats2.tolist())
        assert (stats2[:, 6] == 0).all() and np.array_equal(stats2[:, 7], stats[:, 7])
        # refusals: nothing is queued, nothing changes
        snap = a.view()
        xy_t, desc_t, n_t = _t(xy), _t(desc), _t(n_kp)
        other = capi.World(ctx, 2, 6, SCENE_KP)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            other.fuse_project(a, xy_t, desc_t, n_t, K, W, H)
        other.close()
        for frames in ((-1, 3), (4, 3), (0, 7)):
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                wa.fuse_project(a, xy_t, desc_t, n_t, K, W, H, frames=frames)
        for kw in (dict(search=dict(radius_px=65.0)), dict(search=dict(ratio10=11))):
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                wa.fuse_project(a, xy_t, desc_t, n_t, K, W, H, **kw)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.fuse_project(a, _t(xy[:, :5]), _t(desc[:, :5]), _t(n_kp[:, :5]), K, W, H)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.fuse_project(a, xy_t, desc_t, n_t, K, 0, H)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            wa.fuse_project(a, xy_t, desc_t, n_t, K, 16385, H)
        p = lambda t_, off=0: C.c_void_p(t_.data_ptr() + off)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        raw = lambda x=p(xy_t), d_=p(desc_t), n_=p(n_t), k_=Kh.ctypes.data_as(C.c_void_p): ctx.lib.vslam_world_fuse_project(
            ctx.handle, wa.handle, a.handle, x, d_, n_, 6, k_, W, H, 0, 6, C.c_void_p(0), C.c_void_p(0))
        assert raw(x=p(xy_t, 4)) == -1 and raw(d_=p(desc_t, 8)) == -1 and raw(n_=p(n_t, 2)) == -1
        assert raw(x=C.c_void_p(0)) == -1 and raw(d_=C.c_void_p(0)) == -1 and raw(n_=C.c_void_p(0)) == -1 and raw(k_=C.c_void_p(0)) == -1
        ctx.synchronize()
        again = a.view()
        for k in snap:
            if isinstance(snap[k], np.ndarray):
                assert np.array_equal(_bits(again[k]), _bits(snap[k])), (k, "a refused call writes nothing")
        for k in ("point", "frame", "kp", "desc", "n"):
            assert np.array_equal(again["world_extra"][k], snap["world_extra"][k]), k
        assert raw() == 0                          # search and d_stats may be NULL
        # a reset empties the log
        a.reset()
        ctx.synchronize()
        z = a.view()
        assert "world_fuse_to" not in z and "world_extra" not in z
    finally:
        a.close(); wa.close()
    # frames = (2, 4) on a fresh map: no camera outside that range is touched
    a, wa, cur = _scene_map(ctx, scenes)
    try:
        st = _state(a, wa)                         # no fusion yet: the call makes one
        assert "world_fuse_to" not in st["view"]
        stats = wa.fuse_project(a, _t(xy), _t(desc), _t(n_kp), K, W, H, frames=(2, 4), search=dict(radius_px=6.0)).cpu().numpy()
        ctx.synchronize()
        refs = [_reference(st, t, xy, desc, n_kp, K, W, H, 2, 4, radius_px=6.0, **dims) for t in range(2)]
        after = _hold_world(a, wa, st, refs, stats, "frames (2, 4)")
        ex = after["world_extra"]
        for t in range(2):
            fr_ = ex["frame"][t, :ex["n"][t]]
            assert ex["n"][t] > 0 and ((fr_ >= 2) & (fr_ < 4)).all()
        full = [_reference(st, t, xy, desc, n_kp, K, W, H, 0, 6, radius_px=6.0, **dims)["stats"][3] for t in range(2)]
        print("frames (2, 4):", stats.tolist(), "found over every frame", [int(x) for x in full])
        assert all(stats[t, 3] < full[t] for t in range(2))
    finally:
        a.close(); wa.close()


# ---- the two-pass case on a real map: frames 6 .. 11 repeat frames 0 .. 5 with freshly permuted keypoint indices
R_KP, R_FRAMES = 64, 12
R_MCAP, R_OCAP = R_FRAMES * R_KP, 4 * R_FRAMES * R_KP


def _revisit_map(ctx):
    """ONE track stepped by vslam_map_step over the 60-point scene's six frames, a step without a RANSAC winner (nothing is pushed, the
    frame is recorded), and the same six frames again with permuted keypoints; then, as tests/test_gpu_sim3.py writes reference
    tracks, the world's poses and points overwritten with the scene's true geometry (what vslam_world_close_loops is there to reach),
    so that the two visits lie on top of each other.  -> map, world, (xy, desc, n_kp) [1][12][R_KP], ws"""
    seed, ws = pc.first_world_scene(60)
    n, sc = ws["n"], ws["scene"]
    rng = np.random.default_rng(4242)
    again = [rng.permutation(n) for _ in range(6)]
    xy, desc, n_kp = np.zeros((1, R_FRAMES, R_KP, 2), np.float32), np.zeros((1, R_FRAMES, R_KP, 32), np.uint8), np.full((1, R_FRAMES), n, np.int32)
    for f in range(6):
        xy[0, f, :n], desc[0, f, :n] = ws["xy"][f], ws["desc"][f]
        xy[0, 6 + f, again[f]], desc[0, 6 + f, again[f]] = ws["xy"][f], ws["desc"][f]
    a = capi.PointMap(ctx, 1, R_FRAMES, R_KP, R_MCAP, R_OCAP)
    wa = a.attach_world()
    bgr = torch.full((1, pc.SCENE_H, pc.SCENE_W, 3), 90, dtype=torch.uint8).cuda()

    def frame(f):
        d = dict(xy=_t(xy[:, f]), desc=_t(desc[:, f]), n=_t(n_kp[:, f]))
        d["nodes"] = ctx.kdtree_build(d["xy"], d["n"])
        return d
    last = frame(0)
    for f in range(1, R_FRAMES):
        cur = frame(f)
        matches, best, F = np.zeros((1, R_KP, 2), np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 9), np.float32)
        if f == 6:
            best[0] = (-1, 0, 0, 0)                # no winner between the two visits
        else:
            p = ws["pairs"][f % 6 - 1]
            m = p["matches"] if f < 6 else np.stack([again[f - 7][p["matches"][:, 0]], again[f - 6][p["matches"][:, 1]]], 1)
            matches[0, :len(m)], best[0], F[0] = m, (0, len(m), 0, len(m)), p["F"]
        a.step(last, cur, dict(matches=_t(matches), best=_t(best), F=_t(F)), bgr, pc.SCENE_K)
        last = cur
    ctx.synchronize()
    v = a.view()
    assert v["frames"] == R_FRAMES
    off, fr, kp = _np(a.observations())
    inv = [np.argsort(q) for q in ws["perm"]]
    ident_kp = inv + [None] * 6
    for f in range(6):
        q = np.zeros(n, np.int64)
        q[again[f]] = inv[f]
        ident_kp[6 + f] = q
    size = int(v["sizes"][0])
    pts = v["world_points"].copy()
    ident_pt = np.full(size, -1, np.int64)
    for i in range(size):
        if off[0, i + 1] > off[0, i]:
            ident_pt[i] = ident_kp[fr[0, off[0, i]]][kp[0, off[0, i]]]
            pts[0, i] = (*sc["points"][ident_pt[i]], 1.0)
    Twc = np.zeros((1, R_FRAMES, 16))
    for f in range(R_FRAMES):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = ws["Rwc"][f % 6], sc["centres"][f % 6]
        Twc[0, f] = M.reshape(16)
    wo = wa.arrays()
    _put(ctx, wo.d_world_points, pts); _put(ctx, wo.d_Twc, Twc); _put(ctx, wo.d_pose, Twc.astype(np.float32))
    ctx.synchronize()
    return a, wa, (xy, desc, n_kp), ws, ident_pt


def test_two_passes_on_a_real_map_and_the_consumers(ctx):
    import ref_tracks as rt
    a, wa, (xy, desc, n_kp), ws, ident_pt = _revisit_map(ctx)
    try:
        K, W, H = pc.SCENE_K, pc.SCENE_W, pc.SCENE_H
        dims = dict(frames=R_FRAMES, max_frames=R_FRAMES, kp_stride=R_KP, obs_capacity=R_OCAP)
        # with the call never made: the fusion and the world's CSR are the parent's -- its outputs' bits, and no kernel of this file
        st0 = _state(a, wa)
        ctx.prof_enable(True)
        ctx.prof_reset()
        wa.fuse(a)
        got = _np(wa.observations(a))
        ctx.synchronize()
        names = set(ctx.prof_report())
        ctx.prof_enable(False)
        assert names and not any(nm.startswith("fuse_project") for nm in names), names
        size = int(st0["view"]["sizes"][0])
        r, to, wp = rf.world_fuse(np.arange(R_MCAP, dtype=np.int32), st0["view"]["world_points"][0], size, st0["off"][0], st0["fr"][0], st0["kp"][0],
                                  R_FRAMES, R_KP)
        total = len(r["out_cam"])
        assert np.array_equal(got[0][0], r["out_offsets"]) and np.array_equal(got[1][0, :total], r["out_cam"]) and np.array_equal(got[2][0, :total], r["out_kp"])
        assert np.array_equal(got[3][0, :total], st0["mdesc"][0][r["out_src"]]) and (got[1][0, total:] == -1).all()
        st = _state(a, wa)
        assert np.array_equal(st["view"]["world_fuse_to"][0], to) and "world_extra" not in st["view"]
        live0 = int((to[:size] == np.arange(size)).sum())
        visits = [set(st0["fr"][0][st0["off"][0][i]:st0["off"][0][i + 1]] // 6) for i in range(size)]
        print("map points seen in the first visit only, the second only, both (the map's own association, behind a carried pose):",
              visits.count({0}), visits.count({1}), visits.count({0, 1}))
        assert visits.count({0}) > 20 and visits.count({1}) > 20, "both visits have map points of their own"

        def mixed_groups(labels):
            groups = {}
            for i in range(size):
                if labels[i] >= 0 and ident_pt[i] >= 0:
                    groups.setdefault(int(labels[i]), set()).add(int(ident_pt[i]))
            return sum(len(g) > 1 for g in groups.values())
        mixed0 = mixed_groups(to)
        # the call
        stats = wa.fuse_project(a, _t(xy), _t(desc), _t(n_kp), K, W, H).cpu().numpy()
        ctx.synchronize()
        ref = _reference(st, 0, xy, desc, n_kp, K, W, H, 0, R_FRAMES, **dims)
        after = _hold_world(a, wa, st, [ref], stats, "two passes")
        fuse_to = after["world_fuse_to"][0]
        live1 = int((fuse_to[:size] == np.arange(size)).sum())
        physical = len(set(ident_pt[ident_pt >= 0]))
        mixed = mixed_groups(fuse_to)
        print(f"two passes on the device: {size} map points, {physical} physical; live {live0} -> {live1} (reference "
              f"{int((ref['fuse_to'][:size] == np.arange(size)).sum())}); stats {stats.tolist()}; mixed groups {mixed0} -> {mixed}")
        assert live1 == int((ref["fuse_to"][:size] == np.arange(size)).sum()) and live1 < live0
        assert mixed <= mixed0, "the round mixes no two physical points that the fusion by shared observations had kept apart"
        both = sum(1 for i in range(size) if fuse_to[i] == i and
                   len({int(f) // 6 for j in np.flatnonzero(fuse_to[:size] == i) for f in st0["fr"][0][st0["off"][0][j]:st0["off"][0][j + 1]]}) == 2)
        assert both > 0, "tracks now span both visits"
        # World.retriangulate on the merged lists = the batch entry fed by hand with the world's CSR
        off, fr, kp, _ = wa.observations(a, desc=False)
        cams = rf.cameras(after["world_Twc"][0], R_FRAMES)
        b = dict(points=after["world_points"], n=after["sizes"].astype(np.int32), offsets=off.cpu().numpy(), cam=fr.cpu().numpy(), kp=kp.cpu().numpy(),
                 R=cams[0][None], T=cams[1][None], n_cams=np.full(1, R_FRAMES, np.int32), xy=xy)
        hand = ctx.triangulate_tracks(*(_t(b[k]) for k in ("points", "n", "offsets", "cam", "kp", "R", "T", "n_cams", "xy")), K)
        want = rt.batch_reference(b, K)
        status, tstats = wa.retriangulate(a, _t(xy), K)
        ctx.synchronize()
        tri = a.view()
        assert np.array_equal(status.cpu().numpy(), hand["status"].cpu().numpy()) and np.array_equal(tstats.cpu().numpy(), hand["stats"].cpu().numpy())
        assert np.array_equal(tstats.cpu().numpy(), want["stats"]) and np.array_equal(status.cpu().numpy(), want["status"])
        assert np.array_equal(_bits(tri["world_points"]), _bits(hand["out_points"].cpu().numpy()))
        print("retriangulate on the merged lists:", tstats.cpu().numpy().tolist())
        assert tstats.cpu().numpy()[0, 1] > 0
        # World.adjust on the merged lists = vslam_adjust_windows fed by hand with the window's part of the world's CSR
        off_n, fr_n, kp_n = off.cpu().numpy()[0], fr.cpu().numpy()[0], kp.cpu().numpy()[0]
        f0 = R_FRAMES - 8
        Rw, Tw = np.zeros((1, 8, 9)), np.zeros((1, 8, 3))
        cams = rf.cameras(tri["world_Twc"][0], R_FRAMES)
        Rw[0], Tw[0] = cams[0][f0:], cams[1][f0:]
        offs, ocam, oxy = np.zeros((1, R_MCAP + 1), np.int32), np.zeros((1, R_OCAP), np.int32), np.zeros((1, R_OCAP, 2), np.float32)
        e = 0
        for i in range(size):
            offs[0, i] = e
            for o in range(off_n[i], off_n[i + 1]):
                if f0 <= fr_n[o] < R_FRAMES and 0 <= kp_n[o] < R_KP:
                    ocam[0, e], oxy[0, e] = fr_n[o] - f0, xy[0, fr_n[o], kp_n[o]]
                    e += 1
        offs[0, size:] = e
        X = tri["world_points"][:, :, :3].astype(np.float64)
        _, _, _, st_hand = ctx.adjust_windows(_t(Rw), _t(Tw), _t(np.full(1, 8, np.int32)), _t(X), _t(tri["sizes"]), _t(offs), _t(ocam), _t(oxy), K)
        st_world = wa.adjust(a, _t(xy), K)
        ctx.synchronize()
        print("adjust on the merged lists:", st_world.cpu().numpy().tolist())
        assert np.array_equal(_bits(st_world.cpu().numpy()), _bits(st_hand.cpu().numpy())) and st_world.cpu().numpy()[0, 0] > 0
        # vslam_world_reset gives back "no fusion" with an empty log
        wa.reset()
        ctx.synchronize()
        fv, state = C.c_void_p(), C.c_int32()
        ctx._check(ctx.lib.vslam_world_fusion_view(wa.handle, C.byref(fv), C.byref(state)))
        z = wa.view()
        assert state.value == 0 and not fv.value and "extra" not in z and "fuse_to" not in z
    finally:
        a.close(); wa.close()
