"""include/vslam_tracks.h on the device (vslam_triangulate_tracks and vslam_world_retriangulate) against tests/ref_tracks.py, bit for bit
throughout: positions, statuses, counts, the three f64 of d_info and the statistics of an f64 rule written in one order.  Outputs are
written over a sentinel fill and compared whole.  Every test asserts that its own inputs are not vacuous: the statuses its inputs can
produce occur (DEGENERATE needs every ray of a row to be the same one and the parallax test switched off: the hand cases alone), and
rows with status 0 differ from their input rows."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import pnp_cases as pc
import ref_fuse as rf
import ref_tracks as rt
import tracks_calls as tcl
import tracks_cases as tc
from offset_views import SENTINEL_BYTE, offset_view, sentinel_fill
from test_gpu_fuse import _bits, _hold
from vslam_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DT = dict(out_points=torch.float32, status=torch.int32, counts=torch.int32, info=torch.float64, stats=torch.int32)
IN_KEYS = ("points", "n", "offsets", "cam", "kp", "R", "T", "n_cams", "xy")
OTHER = dict(cos_parallax_max=0.99999, huber_px=1.0, inlier_px=2.0, iterations=3, min_good=3, good10=8)


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _shapes(B, S):
    return dict(out_points=(B, S, 4), status=(B, S), counts=(B, S, 2), info=(B, S, 3), stats=(B, 4))


def _outs(B, S):
    return {k: sentinel_fill(torch.empty(s, dtype=OUT_DT[k], device="cuda")) for k, s in _shapes(B, S).items()}


def _run(ctx, b, K, **params):
    B, S = b["points"].shape[:2]
    out = _outs(B, S)
    ctx.triangulate_tracks(*[_t(b[k]) for k in IN_KEYS], K, out=out, **params)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _seen(ref, name, want):
    """every status of `want` occurs, and some OK row differs from its input row"""
    st = ref["status"]
    have = set(np.unique(st).tolist())
    print(f"{name}: statuses -1 .. 6: {np.bincount(st.reshape(-1) + 1, minlength=8).tolist()}, stats {ref['stats'].tolist()}")
    assert set(want) <= have, (name, sorted(set(want) - have))


def _moved(got, b):
    ok = got["status"] == rt.OK
    return ((got["out_points"].view(np.uint32) != b["points"].view(np.uint32)).any(-1) & ok).sum()


_CACHE = {}


def _item(key):
    """the random items of this file and their references, made once"""
    if key not in _CACHE:
        n, cams, kw, prm = key
        c = rt.random_track_item(1000 + 10 * n + cams, n, cams, S=n + 3, **dict(kw))
        b = rt.batch_tracks([c])
        _CACHE[key] = (c, b, rt.batch_reference(b, c["K"], **dict(prm)))
    return _CACHE[key]


def test_header_symbols_and_defaults(ctx):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_tracks.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.TRACK_SYMBOLS) and sorted(tcl.ENTRIES) == sorted(n for n in names if not n.endswith("_default"))
    others = set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS) | set(capi.SEARCH_SYMBOLS) | set(capi.PNP_SYMBOLS) | set(capi.FUSE_SYMBOLS)
    assert not set(names) & others
    for nm in names:
        assert hasattr(ctx.lib, nm), nm
    p = capi.TrackParams.make(ctx.lib)
    keys = ("cos_parallax_max", "huber_px", "inlier_px", "iterations", "min_good", "good10")
    assert tuple(getattr(p, k) for k in keys) == (0.9998, 2.0, 6.0, 10, 2, 5) == tuple(rt.DEFAULTS[k] for k in keys)
    ap = capi.AdjustParams.make(ctx.lib)
    assert p.huber_px == ap.huber_px and p.inlier_px == ap.gate_px
    assert ctx.lib.vslam_track_params_default(C.c_void_p(0)) == -1


@pytest.mark.parametrize("variant", list(tc.HAND_VARIANTS))
def test_hand_cases(ctx, variant):
    c = tc.hand_cases()[variant]
    b = rt.batch_tracks([c])
    got = _run(ctx, b, c["K"], **c["params"])
    _hold(got, rt.batch_reference(b, c["K"], **c["params"]), rt.OUTS, variant)
    tc.check_hand(variant, {k: v[0] for k, v in got.items()})


RANDOM = [(255, 6, ()), (256, 6, ()), (257, 6, ()), (513, 6, ()), (5000, 6, ()), (257, 64, ()), (5000, 64, ()),
          (20, 1024, (("rows", (1024, 1024)), ("cam_stride", 1024), ("junk", 0.02)))]


@pytest.mark.parametrize("n,cams,kw", RANDOM, ids=[f"n{n}c{c}" for n, c, _ in RANDOM])
def test_random_items(ctx, n, cams, kw):
    for prm in ((), tuple(OTHER.items()), (("iterations", 0),)):
        if n == 5000 and prm and prm[0][0] != "iterations":
            continue
        c, b, ref = _item((n, cams, kw, prm))
        got = _run(ctx, b, c["K"], **dict(prm))
        _hold(got, ref, rt.OUTS, (n, cams, prm))
        full = dict(kw).get("rows") is not None
        _seen(ref, f"n = {n}, {cams} cameras, {dict(prm) or 'defaults'}", [rt.OK] if full else [rt.NO_PART, rt.OK, rt.TOO_FEW, rt.LOW_PARALLAX, rt.UNSUPPORTED])
        assert _moved(got, b) > 0
        if full:
            assert b["R"].shape[1] == 1024 and (np.diff(b["offsets"][0, :n + 1]) == 1024).sum() >= n - 2, "rows as long as the camera count"
    statuses = np.concatenate([_item((n, cams, kw, prm))[2]["status"].reshape(-1) for prm in ((), (("iterations", 0),))])
    if (n, cams) == (5000, 64):
        assert {rt.BEHIND, rt.WORSE} <= set(statuses.tolist()), "the large item reaches every status a random item can"


@pytest.fixture(scope="module")
def three():
    items = [rt.random_track_item(31, 700, 6), rt.random_track_item(32, 40, 4), rt.random_track_item(33, 1300, 9, rows=(1, 5))]
    b = rt.batch_tracks(items)
    K = items[0]["K"]
    return items, b, K, rt.batch_reference(b, K)


def test_batch_of_three_items_of_different_sizes(ctx, three):
    items, b, K, ref = three
    got = _run(ctx, b, K)
    _hold(got, ref, rt.OUTS)
    assert (got["stats"][:, 1] > 0).all() and (got["stats"][:, 3] > 0).all() and got["stats"][:, 2].sum() > 0
    assert all(_moved({k: v[i] for k, v in got.items()}, {"points": b["points"][i]}) > 0 for i in range(3))


def test_one_item_same_bits_alone_in_any_slot_and_in_two_runs(ctx, three):
    items, b, K, ref = three
    one = {k: v[2:3] for k, v in b.items()}
    alone, again = _run(ctx, one, K), _run(ctx, one, K)
    _hold(alone, again, rt.OUTS)
    for slot, src in ((0, [2, 0, 1]), (1, [0, 2, 1])):
        got = _run(ctx, {k: v[src] for k, v in b.items()}, K)
        for k in rt.OUTS:
            assert np.array_equal(_bits(got[k][slot]), _bits(alone[k][0])), (slot, k)
    for k in rt.OUTS:
        assert np.array_equal(_bits(alone[k][0]), _bits(ref[k][2])), k


def test_in_place_gives_the_bits_of_out_of_place(ctx, three):
    items, b, K, ref = three
    B, S = b["points"].shape[:2]
    out = _outs(B, S)
    out["out_points"] = _t(b["points"])
    ins = [_t(b[k]) for k in IN_KEYS]
    ins[0] = out["out_points"]
    ctx.triangulate_tracks(*ins, K, out=out)
    ctx.synchronize()
    _hold({k: v.cpu().numpy() for k, v in out.items()}, ref, rt.OUTS)
    assert (ref["status"] == rt.OK).any() and (ref["status"] > 0).any()


# ------------------------------------------------------------------------------------------------ refusals, alignment, stream order
ARGS = ("points", "n_points", "offsets", "cam", "kp", "R", "T", "n_cams", "xy", "out_points", "status", "counts", "info", "stats")
ALIGN = dict(points=16, out_points=16, xy=8, R=8, T=8, info=8, n_points=4, offsets=4, cam=4, kp=4, n_cams=4, status=4, counts=4, stats=4)
OPTIONAL = ("counts", "info")


def _tensors(b):
    B, S = b["points"].shape[:2]
    d = dict(points=_t(b["points"]), n_points=_t(b["n"]), offsets=_t(b["offsets"]), cam=_t(b["cam"]), kp=_t(b["kp"]), R=_t(b["R"]), T=_t(b["T"]),
             n_cams=_t(b["n_cams"]), xy=_t(b["xy"]))
    d.update(_outs(B, S))
    return d


def _raw(ctx, d, K, over=None, params=None, K_over=None, **sizes):
    B, S, O, Cs, Kp = d["points"].shape[0], d["points"].shape[1], d["cam"].shape[1], d["R"].shape[1], d["xy"].shape[2]
    ptr = {k: d[k].data_ptr() for k in ARGS}
    ptr.update(over or {})
    sz = dict(pt_stride=S, obs_stride=O, cam_stride=Cs, kp_stride=Kp, batch=B)
    sz.update(sizes)
    Kh = np.ascontiguousarray(np.asarray(K if K_over is None or K_over is False else K_over, np.float32).reshape(9))
    v = lambda k: C.c_void_p(ptr[k])
    return ctx.lib.vslam_triangulate_tracks(ctx.handle, v("points"), v("n_points"), sz["pt_stride"], v("offsets"), v("cam"), v("kp"), sz["obs_stride"],
                                            v("R"), v("T"), v("n_cams"), sz["cam_stride"], v("xy"), sz["kp_stride"],
                                            Kh.ctypes.data_as(C.c_void_p) if K_over is not False else C.c_void_p(0), sz["batch"],
                                            C.byref(params) if params is not None else C.c_void_p(0), v("out_points"), v("status"), v("counts"),
                                            v("info"), v("stats"))


BAD_PARAMS = (dict(cos_parallax_max=float("nan")), dict(cos_parallax_max=float("inf")), dict(cos_parallax_max=-1.0), dict(cos_parallax_max=1.0000001),
              dict(huber_px=0.0), dict(huber_px=float("nan")), dict(huber_px=float("inf")), dict(inlier_px=0.0), dict(inlier_px=-1.0),
              dict(inlier_px=float("nan")), dict(inlier_px=float("inf")), dict(iterations=-1), dict(iterations=65), dict(min_good=1), dict(good10=-1),
              dict(good10=11))


def _bad_Ks(K):
    out = []
    for bad in (float("nan"), float("inf")):
        Kb = np.array(K, np.float32).copy()
        Kb[1, 2] = bad
        out.append(Kb)
    Ks = np.array(K, np.float32).copy()
    Ks[2] = Ks[0]                                                    # two equal rows: the determinant is 0
    out.append(Ks)
    out.append(np.zeros((3, 3), np.float32))
    return out                                                      # (no finite f32 K has a determinant or an inverse that overflows f64)


@pytest.fixture(scope="module")
def one():
    c = rt.random_track_item(51, 300, 6)
    b = rt.batch_tracks([c])
    return c, b, rt.batch_reference(b, c["K"])


def _sentinel(d, keys):
    for k in keys:
        assert (d[k].view(torch.uint8) == SENTINEL_BYTE).all(), (k, "nothing ran")


def test_refusals_before_anything_is_queued(ctx, one):
    c, b, ref = one
    K = c["K"]
    d = _tensors(b)
    for bad in BAD_PARAMS:
        assert _raw(ctx, d, K, params=capi.TrackParams.make(ctx.lib, **bad)) == -1, bad
    for k in ARGS:
        if k not in OPTIONAL:
            assert _raw(ctx, d, K, over={k: 0}) == -1, k
    assert _raw(ctx, d, K, K_over=False) == -1
    for kw in (dict(batch=0), dict(pt_stride=0), dict(obs_stride=-1), dict(cam_stride=0), dict(kp_stride=0)):
        assert _raw(ctx, d, K, **kw) == -1, kw
    for Kb in _bad_Ks(K):
        assert _raw(ctx, d, K, K_over=Kb) == -1, Kb
    for kw in (dict(kp_stride=rt.MAX_KP + 1), dict(cam_stride=rt.MAX_CAMS + 1)):
        assert _raw(ctx, d, K, **kw) == -4, kw
    for k, need in ALIGN.items():
        assert _raw(ctx, d, K, over={k: d[k].data_ptr() + need // 2}) == -1, k
        assert "d_" in ctx.lib.vslam_last_error(ctx.handle).decode()
    ctx.synchronize()
    _sentinel(d, rt.OUTS)
    assert _raw(ctx, d, K) == 0                                      # and the next call is exact
    ctx.synchronize()
    _hold({k: d[k].cpu().numpy() for k in rt.OUTS}, ref, rt.OUTS)
    d2 = _tensors(b)
    assert _raw(ctx, d2, K, over=dict(counts=0, info=0)) == 0        # params, d_counts and d_info may be NULL
    ctx.synchronize()
    _hold({k: d2[k].cpu().numpy() for k in ("out_points", "status", "stats")}, ref, ("out_points", "status", "stats"))
    _sentinel(d2, OPTIONAL)
    assert (ref["status"] == rt.OK).any() and (ref["status"] > 0).any()


def test_every_pointer_exactly_at_its_alignment_gives_the_aligned_bits(ctx, one):
    c, b, ref = one
    for nm, need in ALIGN.items():
        d = _tensors(b)
        v, whole, check = offset_view(tuple(d[nm].shape), d[nm].dtype, need // d[nm].element_size())
        assert v.data_ptr() % need == 0 and v.data_ptr() % (2 * need) != 0, nm
        if nm in IN_KEYS or nm == "n_points":
            v.copy_(d[nm])
        d[nm] = v
        assert _raw(ctx, d, c["K"]) == 0, nm
        ctx.synchronize()
        check(nm)
        _hold({k: d[k].cpu().numpy() for k in rt.OUTS}, ref, rt.OUTS, nm)


def _dev(b, i=None):
    return {k: _t(v if i is None else v[i:i + 1]) for k, v in b.items()}


def test_triangulate_stream_order_behind_a_stalled_stream():
    from test_gpu_fuse import _behind_stall
    items = [rt.random_track_item(71, 600, 6), rt.random_track_item(72, 600, 6)]
    both = rt.batch_tracks(items)                                     # one shape for the call and its decoys

    def make(i):
        return tcl.triangulate_tracks(_dev(both, i), items[i]["K"])

    def check(got):
        st = np.frombuffer(got["d_stats"].tobytes(), np.int32)
        assert st[1] > 0 and st[2] > 0 and st[3] > 0
    _behind_stall(make, "vslam_triangulate_tracks", check)


def test_the_call_takes_no_workspace_and_does_not_depend_on_it(ctx, one):
    """The workspace discipline: the same bits with the arena as found and behind Context.workspace_fill; for the batch call
    that is true because it takes no slot at all."""
    import entry_calls as ec
    c, b, ref = one
    for in_place in (False, True):
        call = tcl.triangulate_tracks(_dev(b), c["K"], in_place=in_place)
        slots = ctx.workspace_slots()
        rc, msg, first, _ = ec.run(ctx, call)
        assert rc == 0, msg
        assert ctx.workspace_slots() == slots, "vslam_triangulate_tracks took a workspace slot"
        for fill in (0, 0x5A):
            ctx.workspace_fill(fill)
            rc, msg, got, _ = ec.run(ctx, call)
            assert rc == 0 and not ec._same(first, got), (fill, ec._same(first, got))
        name = "d_points" if in_place else "d_out_points"
        assert np.array_equal(first[name].reshape(-1), _bits(ref["out_points"])) and np.array_equal(first["d_info"].reshape(-1), _bits(ref["info"]))


# ------------------------------------------------------------------------------------------------ on the world
from test_gpu_fuse import _frame, _np, _step, _xy_all  # noqa: E402
from test_gpu_pnp import SCENE_KP, SCENE_MCAP, SCENE_OCAP, _put, _scene_map  # noqa: E402
from test_gpu_world import _same  # noqa: E402


@pytest.fixture(scope="module")
def scenes():
    return [pc.first_world_scene(60)[1], pc.first_world_scene(400)[1]]


def _by_hand(ctx, a, wa, xy_all, view, **params):
    """Context.triangulate_tracks fed by hand with the world's CSR, the cameras of ref_fuse.cameras and world_points -> its outputs and
    the reference's for the same arrays"""
    T = len(view["sizes"])
    off, fr, kp, _ = wa.observations(a, desc=False)
    cams = [rf.cameras(view["world_Twc"][t], 6) for t in range(T)]
    b = dict(points=view["world_points"], n=view["sizes"].astype(np.int32), offsets=off.cpu().numpy(), cam=fr.cpu().numpy(), kp=kp.cpu().numpy(),
             R=np.stack([c[0] for c in cams]), T=np.stack([c[1] for c in cams]), n_cams=np.full(T, 6, np.int32), xy=xy_all)
    return _run(ctx, b, pc.SCENE_K, **params), rt.batch_reference(b, pc.SCENE_K, **params)


def _retriangulate_and_hold(ctx, a, wa, xy_all, what, **params):
    before = a.view()
    hand, ref = _by_hand(ctx, a, wa, xy_all, before, **params)
    _hold(hand, ref, rt.OUTS, what)
    status, stats = wa.retriangulate(a, _t(xy_all), pc.SCENE_K, **params)
    ctx.synchronize()
    after = a.view()
    assert np.array_equal(status.cpu().numpy(), hand["status"]) and np.array_equal(stats.cpu().numpy(), hand["stats"]), what
    assert np.array_equal(_bits(after["world_points"]), _bits(hand["out_points"])), what
    _same(before, after, keys=[k for k in before if k != "world_points"])
    nan_before = np.isnan(before["world_points"][:, :, :3]).any(-1)
    assert np.array_equal(_bits(after["world_points"][nan_before]), _bits(before["world_points"][nan_before])), "NaN rows keep their bits"
    moved = (after["world_points"].view(np.uint32) != before["world_points"].view(np.uint32)).any(-1)
    assert ((hand["status"] == rt.OK) | ~moved).all() and moved.any(1).all(), "only rows with status 0 are written, and some are"
    ok3 = ((hand["status"] == rt.OK) & (hand["counts"][:, :, 0] >= 3)).sum(1)
    print(f"{what}: stats {hand['stats'].tolist()}, OK with m >= 3: {ok3.tolist()}, rows moved {moved.sum(1).tolist()}")
    return hand, ok3, nan_before


def test_world_retriangulate_without_and_with_a_fusion(ctx, scenes):
    a, wa, cur = _scene_map(ctx, scenes)
    try:
        xy_all, _ = _xy_all(scenes)
        assert "world_fuse_to" not in a.view()
        _, ok3_unfused, _ = _retriangulate_and_hold(ctx, a, wa, xy_all, "no fusion")
        assert "world_fuse_to" not in a.view(), "the call makes no fusion state"
    finally:
        a.close(); wa.close()
    a, wa, cur = _scene_map(ctx, scenes)
    try:
        wa.fuse(a)
        ctx.synchronize()
        hand, ok3_fused, nan_rows = _retriangulate_and_hold(ctx, a, wa, xy_all, "after the fusion")
        assert nan_rows.any(1).all() and (hand["status"][nan_rows] == rt.NO_PART).all(), "an absorbed point takes no part"
        assert (ok3_fused > ok3_unfused).all(), (ok3_fused, ok3_unfused)
        _retriangulate_and_hold(ctx, a, wa, xy_all, "other parameters", cos_parallax_max=0.99999, iterations=0, good10=8)
        # the world's consumers still run on the result
        got = wa.search(a, cur, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H)
        st_cull = wa.cull(a, _t(xy_all), pc.SCENE_K).cpu().numpy()
        st_adj = wa.adjust(a, _t(xy_all), pc.SCENE_K).cpu().numpy()
        ctx.synchronize()
        assert (got["n_corr"].cpu().numpy() >= 8).all() and (st_cull[:, 1] > 0).all() and (st_adj[:, 0] > 0).all()
        # a reset and the same steps: the bits of a map never touched
        b, wb, _ = _scene_map(ctx, scenes)
        try:
            want_view = b.view()
        finally:
            b.close(); wb.close()
        a.reset()
        bgr = torch.full((len(scenes), pc.SCENE_H, pc.SCENE_W, 3), 90, dtype=torch.uint8).cuda()
        last = _frame(ctx, scenes, 0)
        for f in range(1, 6):
            last = _step(ctx, a, scenes, f, last, bgr)
        ctx.synchronize()
        got_view = a.view()
        assert "world_fuse_to" not in got_view
        _same(want_view, got_view)
    finally:
        a.close(); wa.close()


def test_world_refusals(ctx, scenes):
    a, wa, cur = _scene_map(ctx, scenes)
    other = capi.World(ctx, len(scenes), 6, SCENE_KP)
    try:
        T = len(scenes)
        xy_all, _ = _xy_all(scenes)
        xy = _t(xy_all)
        before = a.view()
        slots = ctx.workspace_slots()
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            other.retriangulate(a, xy, pc.SCENE_K)                       # not the world attached to that map
        for bad in BAD_PARAMS:
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                wa.retriangulate(a, xy, pc.SCENE_K, **bad)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.retriangulate(a, _t(xy_all[:, :5]), pc.SCENE_K)           # fewer frames of keypoints than recorded
        for Kb in _bad_Ks(pc.SCENE_K):
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                wa.retriangulate(a, xy, Kb)
        st = sentinel_fill(torch.empty((T, 4), dtype=torch.int32, device="cuda"))
        status = sentinel_fill(torch.empty((T, SCENE_MCAP), dtype=torch.int32, device="cuda"))
        Kh = np.ascontiguousarray(pc.SCENE_K.reshape(9))
        lib, h, null, kp = ctx.lib, ctx.handle, C.c_void_p(0), Kh.ctypes.data_as(C.c_void_p)
        p = lambda t, by=0: C.c_void_p(t.data_ptr() + by)
        call = lib.vslam_world_retriangulate
        assert call(h, null, a.handle, p(xy), 6, kp, null, p(status), p(st)) == -1 and call(h, wa.handle, null, p(xy), 6, kp, null, p(status), p(st)) == -1
        assert call(h, wa.handle, a.handle, null, 6, kp, null, p(status), p(st)) == -1 and call(h, wa.handle, a.handle, p(xy), 6, null, null, p(status), p(st)) == -1
        assert call(h, wa.handle, a.handle, p(xy, 4), 6, kp, null, p(status), p(st)) == -1
        assert call(h, wa.handle, a.handle, p(xy), 6, kp, null, p(status, 2), p(st)) == -1
        assert call(h, wa.handle, a.handle, p(xy), 6, kp, null, p(status), p(st, 2)) == -1
        assert call(null, wa.handle, a.handle, p(xy), 6, kp, null, p(status), p(st)) == -1
        ctx.synchronize()
        _sentinel(dict(st=st, status=status), ("st", "status"))
        assert ctx.workspace_slots() == slots, "a refused call takes no workspace"
        _same(before, a.view())
        assert call(h, wa.handle, a.handle, p(xy), 6, kp, null, null, null) == 0      # params, d_status and d_stats may be NULL
        ctx.synchronize()
        after = a.view()
        assert not np.array_equal(_bits(after["world_points"]), _bits(before["world_points"]))
        _same(before, after, keys=[k for k in before if k != "world_points"])
    finally:
        a.close(); wa.close(); other.close()


def test_world_retriangulate_stream_order_and_workspace(ctx, scenes):
    """vslam_world_retriangulate on the session's context behind a stalled stream, as test_gpu_fuse holds vslam_world_cull: the keypoints
    are the inputs, a noisy copy the decoys; the world is put back before every run and what the call leaves in it is compared beside
    its outputs.  Then the same call with its workspace as found and behind Context.workspace_fill."""
    import entry_calls as ec
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    stream = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == stream
    a, wa, _ = _scene_map(ctx, scenes)
    try:
        T = len(scenes)
        xy_all, _ = _xy_all(scenes)
        wa.fuse(a)
        ctx.synchronize()
        start = a.view()

        def before():
            _put(ctx, wa.arrays().d_world_points, start["world_points"])

        def state():
            v = a.view()
            return {k: v[k] for k in ("world_points", "world_fuse_to", "world_Twc", "points", "sizes")}

        def make(noise):
            xy = xy_all.copy()
            if noise:
                rng = np.random.default_rng(noise)
                xy[:, 2:] += rng.uniform(-30, 30, xy[:, 2:].shape).astype(np.float32)
            return tcl.world_retriangulate(wa, a, _t(xy), 6, pc.SCENE_K, before, state)
        call, other = make(0), make(9)
        decoys = Decoys(call, other, None)
        sizing = choose_sizing(ctx, [call], stream)
        res = run_behind_stall(ctx, call, stream, decoys, sizing)
        assert res.rc == 0, res.msg
        assert res.pending_at_return, "vslam_world_retriangulate waited for the device before it returned"
        assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
        assert set(res.got) == set(res.expected)
        for k in res.expected:
            assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"
        st = np.frombuffer(res.got["d_stats"].tobytes(), np.int32).reshape(T, 4)
        assert (st[:, 1] > 0).all() and (st[:, 2] > 0).all()              # exact scenes: points come out OK or without parallax
        assert res.got["state:world_points"].size == _bits(start["world_points"]).size
        assert not np.array_equal(res.got["state:world_points"].reshape(-1), _bits(start["world_points"]))
        rc, msg, first, _ = ec.run(ctx, call)
        assert rc == 0, msg
        assert np.array_equal(first["d_stats"], res.got["d_stats"]) and np.array_equal(first["state:world_points"], res.got["state:world_points"])
        for fill in (0, 0x5A):
            ctx.workspace_fill(fill)
            rc, msg, got, _ = ec.run(ctx, call)
            assert rc == 0 and set(got) == set(first) and not ec._same(first, got), (fill, ec._same(first, got))
    finally:
        a.close(); wa.close()


# ------------------------------------------------------------------------------------------------ C++ surfaces
def test_cpp_surfaces_match_the_c_entry_points(ctx, one, tmp_path):
    """tests/native/tracks_demo.cpp: vslam::triangulate_tracks (include/vslam/helpers.h) on one item gives the bits of the C entry
    point; vslam::World::retriangulate (include/vslam/World.h) is taken on a world attached to a map and throws on one that is not."""
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path / "tracks_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "tracks_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    c, b, ref = one
    S, O, Cs, Kp = b["points"].shape[1], b["cam"].shape[1], b["R"].shape[1], b["xy"].shape[2]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("6i", S, O, int(b["n"][0]), Cs, int(b["n_cams"][0]), Kp))
        f.write(np.asarray(c["K"], np.float32).tobytes())
        for k, dt in (("points", np.float32), ("offsets", np.int32), ("cam", np.int32), ("kp", np.int32), ("R", np.float64), ("T", np.float64),
                      ("xy", np.float32)):
            f.write(np.ascontiguousarray(b[k][0], dt).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    want = b"".join(np.ascontiguousarray(ref[k]).tobytes() for k in rt.OUTS)
    assert (ref["status"] == rt.OK).any() and (ref["status"] > 0).any()
    assert buf[:len(want)] == want
    tail = np.frombuffer(buf[len(want):], np.int32)
    assert len(tail) == 5 and not tail[:4].any() and tail[4] == 1, "an empty attached map: nothing takes part; a world that is not attached is refused"
