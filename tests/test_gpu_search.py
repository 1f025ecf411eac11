"""The search by projection on the device (include/vslam_search.h: vslam_search_projection, vslam_map_observation_descriptors,
vslam_world_search) against tests/ref_search.py, bit for bit throughout: every output of the rule is an integer, a copy of an
input, or an input widened.  The reference is brute force over all keypoints; the device bins them into a grid, so the grid's
edges (tests/search_cases.grid_cases) are where the two could part.  Outputs are written over a sentinel fill and compared
whole: what the rule does not write keeps the caller's bits."""
import os
import re

import numpy as np
import pytest
import torch

import ref_search as rs
import search_cases as sc
from vslam_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = capi.C
OUTS = ("kp_of_point", "dist", "corr_points", "corr_xy", "corr_point", "corr_kp", "n_corr", "stats")
SENTINEL = dict(kp_of_point=77, dist=78, corr_points=7.5, corr_xy=8.5, corr_point=79, corr_kp=80, n_corr=81, stats=82)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _cuda(b, taken=None):
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}
    d["taken"] = None if taken is None else torch.from_numpy(np.ascontiguousarray(taken, np.int32)).cuda()
    return d


def _prefill(B, S, Kp):
    shapes = dict(kp_of_point=((B, S), np.int32), dist=((B, S), np.int32), corr_points=((B, Kp, 3), np.float64), corr_xy=((B, Kp, 2), np.float32),
                  corr_point=((B, Kp), np.int32), corr_kp=((B, Kp), np.int32), n_corr=((B,), np.int32), stats=((B, 4), np.int32))
    return {k: np.full(s, SENTINEL[k], t) for k, (s, t) in shapes.items()}


def _search(ctx, b, K, width, height, taken=None, **params):
    """b: ref_search.batch_of's arrays -> the device's outputs over the sentinel fill, as numpy"""
    d = _cuda(b, taken)
    B, S, Kp = b["points"].shape[0], b["points"].shape[1], b["xy"].shape[1]
    out = {k: torch.from_numpy(v).cuda() for k, v in _prefill(B, S, Kp).items()}
    ctx.search_projection(d["points"], d["n_points"], d["offsets"], d["obs_desc"], d["R"], d["T"], K, width, height, d["xy"], d["desc"],
                          d["n_kp"], d["taken"], out=out, **params)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _reference(b, K, width, height, taken=None, **params):
    B, S, Kp = b["points"].shape[0], b["points"].shape[1], b["xy"].shape[1]
    return rs.search_batch(b["points"], b["n_points"], b["offsets"], b["obs_desc"], b["R"], b["T"], K, width, height, b["xy"], b["desc"],
                           b["n_kp"], taken, prefill=_prefill(B, S, Kp), **params)


def _hold(got, ref, name=""):
    for k in OUTS:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (name, k)


def _case_batch(c):
    return rs.batch_of([c]), (None if c.get("taken") is None else c["taken"][None])


def _run_case(ctx, name, c):
    b, taken = _case_batch(c)
    got = _search(ctx, b, c["K"], c["width"], c["height"], taken, **c.get("params", {}))
    ref = _reference(b, c["K"], c["width"], c["height"], taken, **c.get("params", {}))
    _hold(got, ref, name)
    return got


def test_header_symbols_and_defaults(ctx):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_search.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.SEARCH_SYMBOLS)
    assert not set(names) & (set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS))
    for nm in names:
        assert hasattr(ctx.lib, nm), nm
    p = capi.SearchParams.make(ctx.lib)
    assert (p.radius_px, p.dist_threshold, p.ratio10) == (8.0, 64, 8) == tuple(rs.DEFAULTS[k] for k in ("radius_px", "dist_threshold", "ratio10"))
    assert ctx.lib.vslam_search_params_default(C.c_void_p(0)) == -1


def test_hand_cases(ctx):
    for name, c in sc.hand_cases().items():
        got = _run_case(ctx, name, c)
        assert np.array_equal(got["kp_of_point"][0], c["expect"]), (name, got["kp_of_point"][0])


GRID = sc.grid_cases()


@pytest.mark.parametrize("size", ["37x23", "640x480", "1280x720", "16384x16384", "patch"])
def test_grid_edges(ctx, size):
    for name in [n for n in GRID if n.startswith(size)]:
        got = _run_case(ctx, name, GRID[name])
        print(name, got["stats"][0])
        assert got["stats"][0, 3] > 0, name


def test_one_item_at_max_kp(ctx):
    c = sc.random_case(7, 600, rs.MAX_KP, 1280, 720, 8.0)
    assert c["n_kp"] == len(c["xy"]) == 16384
    got = _run_case(ctx, "max_kp", c)
    assert got["stats"][0, 3] > 100 and got["kp_of_point"].max() > 16000


@pytest.mark.parametrize("n_points", [255, 256, 257, 511, 512, 513, 5000])
def test_point_chunks(ctx, n_points):
    c = sc.random_case(100 + n_points, n_points, 700, 640, 480, 8.0)
    got = _run_case(ctx, f"n{n_points}", c)
    assert got["stats"][0, 3] > 50


def test_a_batch_of_three_items_of_different_sizes(ctx):
    items = [sc.random_case(21, 700, 300, 640, 480, 8.0), sc.random_case(22, 60, 900, 640, 480, 8.0), sc.random_case(23, 1300, 40, 640, 480, 8.0)]
    b = rs.batch_of(items)
    taken = np.full(b["xy"].shape[:2], -1, np.int32)
    for i, it in enumerate(items):
        taken[i, :len(it["taken"])] = it["taken"]
    K = items[0]["K"]
    got = _search(ctx, b, K, 640, 480, taken, radius_px=8.0)
    _hold(got, _reference(b, K, 640, 480, taken, radius_px=8.0))
    assert (got["stats"][:, 3] > 0).all()


@pytest.fixture(scope="module")
def planted():
    scenes = [rs.planted_scene(s) for s in (1, 2, 3, 4, 5, 6)]
    b = rs.batch_of(scenes)
    return scenes, b, _reference(b, scenes[0]["K"], 640, 480)


def test_planted_scenes_as_one_batch(ctx, planted):
    scenes, b, ref = planted
    got = _search(ctx, b, scenes[0]["K"], 640, 480)
    _hold(got, ref)
    for i, s in enumerate(scenes):
        found, wrong = rs.scene_shares(s, dict(kp_of_point=got["kp_of_point"][i]))
        assert found >= 0.90 and wrong <= 0.05


def test_one_item_same_bits_alone_in_any_slot_and_in_two_runs(ctx, planted):
    scenes, b, ref = planted
    K = scenes[0]["K"]
    one = {k: v[2:3] for k, v in b.items()}
    alone = _search(ctx, one, K, 640, 480)
    again = _search(ctx, one, K, 640, 480)
    _hold(alone, again)
    order = [0, 1, 3, 4, 5, 2]
    for slot, src in ((0, [2, 0, 1, 3, 4, 5]), (5, order)):
        got = _search(ctx, {k: v[src] for k, v in b.items()}, K, 640, 480)
        for k in OUTS:
            assert np.array_equal(_bits(got[k][slot]), _bits(alone[k][0])), (slot, k)
    for k in OUTS:
        assert np.array_equal(_bits(alone[k][0]), _bits(ref[k][2])), k


def test_chained_into_the_resection(ctx, planted):
    """vslam_resect_poses fed the device's d_corr_points / d_corr_xy / d_n_corr directly = the same call fed the reference's"""
    scenes, b, ref = planted
    K = scenes[0]["K"]
    d = _cuda(b)
    out = ctx.search_projection(d["points"], d["n_points"], d["offsets"], d["obs_desc"], d["R"], d["T"], K, 640, 480, d["xy"], d["desc"], d["n_kp"])
    R1, T1, st1 = ctx.resect_poses(out["corr_points"], out["corr_xy"], out["n_corr"], K, d["R"].clone(), d["T"].clone())
    r = {k: torch.from_numpy(ref[k]).cuda() for k in ("corr_points", "corr_xy")}   # sentinels from n_corr on: not read
    R2, T2, st2 = ctx.resect_poses(r["corr_points"], r["corr_xy"], torch.from_numpy(ref["n_corr"]).cuda(), K, d["R"].clone(), d["T"].clone())
    ctx.synchronize()
    for a, c in ((R1, R2), (T1, T2), (st1, st2)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(c.cpu().numpy()))
    st = st1.cpu().numpy()
    assert (st[:, 3] >= 1).all() and (st[:, 2] < st[:, 1]).all()


# ------------------------------------------------------------------------------------------------ refusals, alignment
ARGS = ("points", "n_points", "offsets", "obs_desc", "R", "T", "xy", "desc", "n_kp", "taken", "kp_of_point", "dist", "corr_points", "corr_xy",
        "corr_point", "corr_kp", "n_corr", "stats")
OPTIONAL = ("taken", "corr_point", "corr_kp", "stats")
ALIGN = dict(points=16, desc=16, obs_desc=16, xy=8, corr_xy=8, R=8, T=8, corr_points=8, n_points=4, offsets=4, n_kp=4, taken=4, kp_of_point=4,
             dist=4, corr_point=4, corr_kp=4, n_corr=4, stats=4)


def _raw(ctx, d, K, w_, h_, over=None, out=None, params=None, K_over=None, **sizes):
    """the C entry point with any pointer or size replaced -> (rc, the output tensors)"""
    B, S, Kp, O = d["points"].shape[0], d["points"].shape[1], d["xy"].shape[1], d["obs_desc"].shape[1]
    if out is None:
        out = {k: torch.from_numpy(v).cuda() for k, v in _prefill(B, S, Kp).items()}
    ptr = {k: (d[k].data_ptr() if d.get(k) is not None else 0) for k in ARGS[:10]}
    ptr.update({k: out[k].data_ptr() for k in ARGS[10:]})
    ptr.update(over or {})
    sz = dict(pt_stride=S, obs_stride=O, kp_stride=Kp, batch=B, width=w_, height=h_)
    sz.update(sizes)
    Kh = np.ascontiguousarray(np.asarray(K if K_over is None or K_over is False else K_over, np.float32).reshape(9))
    v = lambda k: C.c_void_p(ptr[k])
    rc = ctx.lib.vslam_search_projection(
        ctx.handle, v("points"), v("n_points"), sz["pt_stride"], v("offsets"), v("obs_desc"), sz["obs_stride"], v("R"), v("T"),
        Kh.ctypes.data_as(C.c_void_p) if K_over is not False else C.c_void_p(0), sz["width"], sz["height"], v("xy"), v("desc"), v("n_kp"),
        sz["kp_stride"], v("taken"), sz["batch"], C.byref(params) if params is not None else C.c_void_p(0), v("kp_of_point"), v("dist"),
        v("corr_points"), v("corr_xy"), v("corr_point"), v("corr_kp"), v("n_corr"), v("stats"))
    return rc, out


def test_invalid_arguments_are_refused_before_anything_is_queued(ctx, planted):
    scenes, b, ref = planted
    K = scenes[0]["K"]
    one = {k: v[:1] for k, v in b.items()}
    d = _cuda(one, np.full(one["xy"].shape[:2], -1, np.int32))
    B, S, Kp = 1, one["points"].shape[1], one["xy"].shape[1]
    out = {k: torch.from_numpy(v).cuda() for k, v in _prefill(B, S, Kp).items()}
    for bad in (dict(radius_px=0.0), dict(radius_px=-1.0), dict(radius_px=64.5), dict(radius_px=float("nan")), dict(radius_px=float("inf")),
                dict(dist_threshold=0), dict(dist_threshold=258), dict(ratio10=-1), dict(ratio10=11)):
        assert _raw(ctx, d, K, 640, 480, out=out, params=capi.SearchParams.make(ctx.lib, **bad))[0] == -1, bad
    for k in ARGS:
        if k not in OPTIONAL:
            assert _raw(ctx, d, K, 640, 480, out=out, over={k: 0})[0] == -1, k
    assert _raw(ctx, d, K, 640, 480, out=out, K_over=False)[0] == -1                     # h_K NULL
    for kw in (dict(batch=0), dict(batch=-1), dict(pt_stride=0), dict(obs_stride=0), dict(kp_stride=0), dict(width=0), dict(height=-4)):
        assert _raw(ctx, d, K, 640, 480, out=out, **kw)[0] == -1, kw
    for bad in (float("nan"), float("inf")):
        Kb = np.array(K, np.float32).copy()
        Kb[1, 2] = bad
        assert _raw(ctx, d, K, 640, 480, out=out, K_over=Kb)[0] == -1
    for kw in (dict(kp_stride=rs.MAX_KP + 1), dict(width=16385), dict(height=16385)):
        assert _raw(ctx, d, K, 640, 480, out=out, **kw)[0] == -4, kw
    for k, need in ALIGN.items():                                                        # one pointer at a time, below its requirement
        base = out[k].data_ptr() if k in out else d[k].data_ptr()
        assert _raw(ctx, d, K, 640, 480, out=out, over={k: base + need // 2})[0] == -1, k
        assert "d_" in ctx.lib.vslam_last_error(ctx.handle).decode()
    assert ctx.lib.vslam_search_projection(C.c_void_p(0), *[C.c_void_p(0)] * 2, S, *[C.c_void_p(0)] * 2, 8, *[C.c_void_p(0)] * 3, 640, 480,
                                           *[C.c_void_p(0)] * 3, Kp, C.c_void_p(0), 1, *[C.c_void_p(0)] * 9) == -1
    ctx.synchronize()
    fill = _prefill(B, S, Kp)
    for k in OUTS:
        assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(fill[k])), (k, "nothing ran")
    rc, out = _raw(ctx, d, K, 640, 480, out=out)                                         # and the next call is exact
    ctx.synchronize()
    assert rc == 0
    _hold({k: v.cpu().numpy() for k, v in out.items()}, {k: v[:1] for k, v in ref.items()})
    rc, o2 = _raw(ctx, d, K, 640, 480, over=dict(taken=0, corr_point=0, corr_kp=0, stats=0))   # the optional ones may be NULL
    ctx.synchronize()
    assert rc == 0
    for k in OUTS:
        want = fill[k] if k in ("corr_point", "corr_kp", "stats") else ref[k][:1]
        assert np.array_equal(_bits(o2[k].cpu().numpy()), _bits(want)), k


def test_every_pointer_exactly_at_its_alignment_gives_the_aligned_bits(ctx, planted):
    from offset_views import offset_view
    scenes, b, ref = planted
    K = scenes[0]["K"]
    one = {k: v[:1] for k, v in b.items()}
    B, S, Kp = 1, one["points"].shape[1], one["xy"].shape[1]
    taken = np.full(one["xy"].shape[:2], -1, np.int32)
    names = dict(points="points", n_points="n_points", offsets="offsets", obs_desc="obs_desc", R="R", T="T", xy="xy", desc="desc", n_kp="n_kp",
                 taken="taken")
    for nm, need in ALIGN.items():
        d = _cuda(one, taken)
        out = {k: torch.from_numpy(v).cuda() for k, v in _prefill(B, S, Kp).items()}
        src = d if nm in names else out
        elem = src[nm].element_size()
        v, whole, check = offset_view(tuple(src[nm].shape), src[nm].dtype, need // elem)
        assert v.data_ptr() % need == 0 and v.data_ptr() % (2 * need) != 0, nm
        v.copy_(src[nm])
        src[nm] = v
        rc, out = _raw(ctx, d, K, 640, 480, out=out)
        ctx.synchronize()
        assert rc == 0, nm
        check(nm)
        _hold({k: x.cpu().numpy() for k, x in out.items()}, {k: x[:1] for k, x in ref.items()}, nm)


def test_stream_order_behind_a_stalled_stream(planted):
    import header_calls as hc
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    scenes, b, ref = planted
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = capi.Context(0)
        try:
            def make(i):
                return hc.search_projection(_cuda({k: v[i:i + 1] for k, v in b.items()}), scenes[0]["K"], 640, 480)
            call, other = make(0), make(1)
            decoys = Decoys(call, other, None)
            sizing = choose_sizing(ctx, [call], stream)
            print("stream order:", sizing)
            res = run_behind_stall(ctx, call, stream, decoys, sizing)
            assert res.rc == 0, res.msg
            assert res.pending_at_return, "vslam_search_projection waited for the device before it returned"
            assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
            assert set(res.got) == set(res.expected)
            for k in res.expected:
                assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"
            assert np.frombuffer(res.got["d_n_corr"].tobytes(), np.int32)[0] == ref["n_corr"][0] > 100
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------------ on the world
from test_gpu_world import FRAMES as MF, KP as MKP, MCAP, OCAP, TRACKS, W as MW, H as MH, _Kmat, _frame_batches, _same, _track, sequences  # noqa: E402,F401


def _pose_of(Twc):
    """include/vslam_adjust.h, "camera c": (R, T) of a camera -> world matrix M (16,)"""
    R, T = np.zeros(9), np.zeros(3)
    for r in range(3):
        for c in range(3):
            R[3 * r + c] = Twc[4 * c + r]
        T[r] = -((Twc[r] * Twc[3] + Twc[4 + r] * Twc[7]) + Twc[8 + r] * Twc[11])
    return R, T


def _by_hand(ctx, pmap, view, cur, Km, **params):
    """vslam_search_projection built from the views: -> the device's outputs (cuda), R, T (numpy) searched from"""
    f1 = int(view["frames"]) - 1
    RT = [_pose_of(view["world_Twc"][t, f1]) for t in range(TRACKS)]
    R, T = np.stack([x[0] for x in RT]), np.stack([x[1] for x in RT])
    off, desc = pmap.observation_descriptors()
    out = ctx.search_projection(torch.from_numpy(view["world_points"]).cuda(), torch.from_numpy(view["sizes"]).cuda(), off, desc,
                                torch.from_numpy(R).cuda(), torch.from_numpy(T).cuda(), Km, MW, MH, cur["xy"], cur["desc"], cur["n"], **params)
    ctx.synchronize()
    return out, R, T, off.cpu().numpy(), desc.cpu().numpy()


def _hold_world_outputs(got, hand):
    n = hand["n_corr"].cpu().numpy()
    assert np.array_equal(got["n_corr"].cpu().numpy(), n)
    for k in ("corr_point", "corr_kp"):
        a, b_ = got[k].cpu().numpy(), hand[k].cpu().numpy()
        for t in range(TRACKS):
            assert np.array_equal(a[t, :n[t]], b_[t, :n[t]]), (k, t)
            assert not a[t, n[t]:].any(), "slots from n_corr on keep their bits"
    return n


@pytest.mark.parametrize("resection", [None, {}], ids=["plain", "resecting"])
def test_world_search(ctx, sequences, resection):
    a = capi.PointMap(ctx, TRACKS, MF, MKP, MCAP, OCAP)
    wa = a.attach_world(resection=resection)
    try:
        out = _track(ctx, a, sequences)
        ctx.synchronize()
        Km = _Kmat()
        cur, _ = _frame_batches(out, MF - 1)
        before = a.view()
        assert before["frames"] == MF and int(before["sizes"].min()) > 8
        # the map's observation descriptors: row o is the descriptor of the (frame, keypoint) vslam_map_observations puts at row o
        off2, fr, kp = [t.cpu().numpy() for t in a.observations()]
        hand, R, T, off, desc = _by_hand(ctx, a, before, cur, Km)
        all_desc = out["desc"].cpu().numpy().reshape(TRACKS, MF, MKP, 32)
        assert np.array_equal(off, off2)
        for t in range(TRACKS):
            total = off[t, before["sizes"][t]]
            assert total > 0 and np.array_equal(desc[t, :total], all_desc[t, fr[t, :total], kp[t, :total]]), t
            assert not desc[t, total:].any(), "rows past the track's total keep their bits"
        # against the reference, from the same views
        ref = rs.search_batch(before["world_points"], before["sizes"], off, desc, R, T, Km, MW, MH, cur["xy"].cpu().numpy(),
                              cur["desc"].cpu().numpy(), cur["n"].cpu().numpy())
        for k in OUTS:
            assert np.array_equal(_bits(hand[k].cpu().numpy()), _bits(ref[k])), k
        # search only: equal to the call built by hand, and nothing of the world or the map changes
        got = wa.search(a, cur, Km, MW, MH)
        ctx.synchronize()
        n = _hold_world_outputs(got, hand)
        print("found per track", n.tolist(), "of", before["sizes"].tolist(), "points; links of the last step", before["world_links"][:, MF - 1].tolist())
        assert (n >= 8).all() and "stats" not in got
        _same(before, a.view())

        # resecting: the hand-built chain and the header's write-back in numpy f64
        def chain(view, params):
            h, R0, T0, _, _ = _by_hand(ctx, a, view, cur, Km)
            Rn, Tn, st = ctx.resect_poses(h["corr_points"], h["corr_xy"], h["n_corr"], Km, torch.from_numpy(R0).cuda(), torch.from_numpy(T0).cuda(),
                                          **params)
            ctx.synchronize()
            Rn, Tn, st = Rn.cpu().numpy(), Tn.cpu().numpy(), st.cpu().numpy()
            want = {k: view[k].copy() for k in ("world_Twc", "world_pose", "world_carry")}
            f1 = MF - 1
            for t in np.flatnonzero(~np.isnan(st[:, 3])):
                old = view["world_Twc"][t, f1].copy()
                m = np.zeros(16)
                for r in range(3):
                    for c in range(3):
                        m[4 * r + c] = Rn[t, 3 * c + r]
                    m[4 * r + 3] = -((Rn[t, r] * Tn[t, 0] + Rn[t, 3 + r] * Tn[t, 1]) + Rn[t, 6 + r] * Tn[t, 2])
                m[15] = 1.0
                want["world_Twc"][t, f1] = m
                want["world_pose"][t, f1] = m.astype(np.float32)
                for k in np.flatnonzero(view["world_carry_index"][t] >= 0):
                    p = view["world_carry"][t, k]
                    w = [((old[4 * r] * p[0] + old[4 * r + 1] * p[1]) + old[4 * r + 2] * p[2]) + old[4 * r + 3] for r in range(3)]
                    want["world_carry"][t, k] = [((Rn[t, 3 * r] * w[0] + Rn[t, 3 * r + 1] * w[1]) + Rn[t, 3 * r + 2] * w[2]) + Tn[t, r] for r in range(3)]
            return h, st, want

        def hold(view, params):
            h, st, want = chain(view, params)
            got = wa.search(a, cur, Km, MW, MH, resect=params)
            ctx.synchronize()
            after = a.view()
            _hold_world_outputs(got, h)
            assert np.array_equal(_bits(got["stats"].cpu().numpy()), _bits(st))
            valid = view["world_carry_index"] >= 0
            for k in ("world_Twc", "world_pose"):
                assert np.array_equal(_bits(after[k]), _bits(want[k])), k
            assert np.array_equal(_bits(after["world_carry"][valid]), _bits(want["world_carry"][valid]))
            keep = [k for k in view if k not in want]
            assert all(k in keep for k in ("points", "world_points", "world_scale", "world_links", "world_carry_index", "sizes", "obs_counts"))
            _same(view, after, keys=keep)
            return st, after
        # one track left alone: min_links above what the track with the fewest correspondences found, below the others'
        order = np.argsort(n)
        if n[order[0]] < n[order[1]]:
            st, after = hold(before, dict(min_links=int(n[order[0]]) + 1))
            alone = order[0]
            assert np.isnan(st[alone, 1:]).all() and not np.isnan(st[order[1:], 3]).any()
            assert np.array_equal(_bits(after["world_Twc"][alone]), _bits(before["world_Twc"][alone]))
            assert np.array_equal(_bits(after["world_carry"][alone]), _bits(before["world_carry"][alone]))
            assert not np.array_equal(after["world_Twc"][order[1]], before["world_Twc"][order[1]])
            view = after
        else:
            view = before
        st, after = hold(view, {})
        moved = ~np.isnan(st[:, 3])
        print("resection: participants", st[:, 0].tolist(), "mean rho", st[:, 1].tolist(), "->", st[:, 2].tolist(), "accepted", st[:, 3].tolist())
        assert moved.any() and (st[moved, 2] < st[moved, 1]).all()
        assert np.array_equal(_bits(after["world_Twc"][:, :MF - 1]), _bits(view["world_Twc"][:, :MF - 1])), "earlier frames keep their bits"
    finally:
        a.close(); wa.close()


def test_world_search_after_a_pair_without_a_winner(ctx, sequences):
    """The last pair of track 1 has no winner: its carry is empty, so the step's resection has no links -- and the search from
    the pose the chain kept still finds the map's points in the frame."""
    a = capi.PointMap(ctx, TRACKS, MF, MKP, MCAP, OCAP)
    b = capi.PointMap(ctx, TRACKS, MF, MKP, MCAP, OCAP)
    wb = b.attach_world(resection={})
    try:
        out = _track(ctx, a, sequences)
        ctx.synchronize()
        Km = _Kmat()
        last, _ = _frame_batches(out, 0)
        for f in range(1, MF):
            cur, pair = _frame_batches(out, f)
            if f == MF - 1:
                pair["best"][1, 0] = -1
            b.step(last, cur, pair, sequences[:, f].contiguous(), Km)
            last = cur
        ctx.synchronize()
        v = b.view()
        assert (v["world_carry_index"][1] < 0).all() and (v["world_carry_index"][0] >= 0).any()
        got = wb.search(b, last, Km, MW, MH, resect={})
        ctx.synchronize()
        n, st = got["n_corr"].cpu().numpy(), got["stats"].cpu().numpy()
        print("found", n.tolist(), "statistics", st.tolist())
        assert n[1] >= 8
        hand, _, _, _, _ = _by_hand(ctx, b, v, last, Km)
        assert np.array_equal(hand["n_corr"].cpu().numpy(), n)
    finally:
        a.close(); b.close(); wb.close()


def test_world_search_errors(ctx, sequences):
    a = capi.PointMap(ctx, TRACKS, MF, MKP, MCAP, OCAP)
    wa = a.attach_world()
    other = capi.World(ctx, TRACKS, MF, MKP)
    try:
        out = _track(ctx, a, sequences)
        ctx.synchronize()
        Km = _Kmat()
        cur, _ = _frame_batches(out, MF - 1)
        before = a.view()
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            other.search(a, cur, Km, MW, MH)                                # not the world attached to that map
        for bad in (dict(radius_px=0.0), dict(radius_px=65.0), dict(dist_threshold=0), dict(ratio10=11)):
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                wa.search(a, cur, Km, MW, MH, **bad)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.search(a, cur, Km, MW, MH, resect=dict(min_links=5))
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.search(a, cur, Km, 0, MH)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            wa.search(a, cur, Km, 16385, MH)
        Kb = Km.copy()
        Kb[0, 0] = np.nan
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.search(a, cur, Kb, MW, MH)
        o = {k: torch.full((TRACKS, MKP), 5, dtype=torch.int32).cuda() for k in ("corr_point", "corr_kp")}
        o["n_corr"] = torch.full((TRACKS,), 5, dtype=torch.int32).cuda()
        st = torch.full((TRACKS, 4), 5.0, dtype=torch.float64).cuda()

        def raw(**over):
            p = dict(xy=cur["xy"].data_ptr(), desc=cur["desc"].data_ptr(), n=cur["n"].data_ptr(), K=Km.ctypes.data, corr_point=o["corr_point"].data_ptr(),
                     corr_kp=o["corr_kp"].data_ptr(), n_corr=o["n_corr"].data_ptr(), stats=st.data_ptr())
            p.update(over)
            v = lambda k: C.c_void_p(p[k])
            return ctx.lib.vslam_world_search(ctx.handle, wa.handle, a.handle, v("xy"), v("desc"), v("n"), v("K"), MW, MH, C.c_void_p(0), C.c_void_p(0),
                                              v("corr_point"), v("corr_kp"), v("n_corr"), v("stats"))
        for k in ("xy", "desc", "n", "K", "corr_point", "corr_kp", "n_corr"):
            assert raw(**{k: 0}) == -1, k
        for k, off in (("xy", 4), ("desc", 8), ("n", 2), ("corr_point", 2), ("corr_kp", 2), ("n_corr", 2), ("stats", 4)):
            base = st.data_ptr() if k == "stats" else (o[k].data_ptr() if k in o else cur[k].data_ptr())
            assert raw(**{k: base + off}) == -1, k
        ctx.synchronize()
        _same(before, a.view())
        assert all((x.cpu().numpy() == 5).all() for x in o.values()) and (st.cpu().numpy() == 5.0).all(), "nothing ran"
        assert raw(stats=0) == 0                                             # search, resect and d_stats may be NULL
        ctx.synchronize()
        want = wa.search(a, cur, Km, MW, MH)
        ctx.synchronize()
        assert np.array_equal(o["n_corr"].cpu().numpy(), want["n_corr"].cpu().numpy()) and (o["n_corr"].cpu().numpy() >= 8).all()
    finally:
        a.close(); wa.close(); other.close()


def test_world_search_stream_order_behind_a_stalled_stream(sequences):
    """the search-only call (it changes nothing of the world, so the plain run and the stalled run start from the same state):
    the current frame's arrays are the inputs, another frame's the decoys"""
    import header_calls as hc
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = capi.Context(0)
        a = capi.PointMap(ctx, TRACKS, MF, MKP, MCAP, OCAP)
        wa = a.attach_world()
        try:
            out = _track(ctx, a, sequences)
            ctx.synchronize()

            def make(f):
                return hc.world_search(wa, a, _frame_batches(out, f)[0], _Kmat(), MW, MH)
            call, other = make(MF - 1), make(1)
            decoys = Decoys(call, other, None)
            sizing = choose_sizing(ctx, [call], stream)
            print("stream order:", sizing)
            res = run_behind_stall(ctx, call, stream, decoys, sizing)
            assert res.rc == 0, res.msg
            assert res.pending_at_return, "vslam_world_search waited for the device before it returned"
            assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
            assert set(res.got) == set(res.expected)
            for k in res.expected:
                assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"
            assert (np.frombuffer(res.got["d_n_corr"].tobytes(), np.int32) >= 8).all()
        finally:
            a.close(); wa.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ C++ surfaces
def test_cpp_surfaces_match_the_c_entry_point(ctx, planted, tmp_path):
    """tests/native/search_demo.cpp: vslam::search_projection (include/vslam/helpers.h) on one item gives the bits of the C entry
    point; vslam::World::search (include/vslam/World.h) is taken on a world attached to a map and throws on one that is not."""
    import struct
    import subprocess
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path / "search_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "search_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    scenes, b, ref = planted
    one = {k: v[3:4] for k, v in b.items()}
    S, O, Kp = one["points"].shape[1], one["obs_desc"].shape[1], one["xy"].shape[1]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(scenes[0]["K"], np.float32).tobytes())
        f.write(struct.pack("7i", S, O, Kp, int(one["n_points"][0]), int(one["n_kp"][0]), 640, 480))
        for k, dt in (("R", np.float64), ("T", np.float64), ("points", np.float32), ("offsets", np.int32), ("obs_desc", np.uint8),
                      ("xy", np.float32), ("desc", np.uint8)):
            f.write(np.ascontiguousarray(one[k][0], dt).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    d = _cuda(one)
    out = ctx.search_projection(d["points"], d["n_points"], d["offsets"], d["obs_desc"], d["R"], d["T"], scenes[0]["K"], 640, 480, d["xy"],
                                d["desc"], d["n_kp"])
    ctx.synchronize()
    want = b"".join(out[k].cpu().numpy().tobytes() for k in ("kp_of_point", "dist", "corr_point", "corr_kp", "n_corr", "stats", "corr_points",
                                                             "corr_xy"))
    assert int(out["n_corr"][0]) == ref["n_corr"][3] > 100
    assert buf[:len(want)] == want
    tail = struct.unpack("3i", buf[len(want):])
    assert tail == (0, 0, 1), "an empty attached map: taken, nothing found; a world that is not attached is refused"
