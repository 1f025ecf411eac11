"""include/vslam_fuse.h on the device (vslam_fuse_points, vslam_cull_points and their calls on a world) against tests/ref_fuse.py, bit for
bit throughout: the fusion is integers, the cull's outputs are integer verdicts and counts of an f64 rule written in one order.
Outputs are written over a sentinel fill and compared whole: what a rule does not write keeps the caller's bits.  Every test asserts
that its own inputs are not vacuous (groups, absorbed points, dropped duplicates, kept and culled points) wherever the rule under test
can produce them."""
import os
import re

import numpy as np
import pytest
import torch

import fuse_cases as fc
import pnp_cases as pc
import ref_fuse as rf
from vslam_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = capi.C
FSENT = dict(fuse_to=77, out_offsets=78, out_cam=79, out_kp=80, out_src=81, stats=82)
CSENT = dict(keep=77, counts=78, stats=79)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


# ------------------------------------------------------------------------------------------------ the fusion
def _fprefill(B, S, O):
    shapes = dict(fuse_to=(B, S), out_offsets=(B, S + 1), out_cam=(B, O), out_kp=(B, O), out_src=(B, O), stats=(B, 4))
    return {k: np.full(s, FSENT[k], np.int32) for k, s in shapes.items()}


def _fuse(ctx, b, cam_stride, kp_stride, masked=True):
    """b: ref_fuse.batch_fuse's arrays -> the device's outputs over the sentinel fill, as numpy"""
    B, S, O = b["offsets"].shape[0], b["offsets"].shape[1] - 1, b["cam"].shape[1]
    out = {k: _t(v) for k, v in _fprefill(B, S, O).items()}
    ctx.fuse_points(_t(b["n"]), _t(b["offsets"]), _t(b["cam"]), _t(b["kp"]), cam_stride, kp_stride, _t(b["mask"]) if masked else None, out=out)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _fuse_ref(b, cam_stride, kp_stride, masked=True):
    B, S, O = b["offsets"].shape[0], b["offsets"].shape[1] - 1, b["cam"].shape[1]
    return rf.fuse_batch(b["n"], b["offsets"], b["cam"], b["kp"], cam_stride, kp_stride, b["mask"] if masked else None, prefill=_fprefill(B, S, O))


def _hold(got, ref, keys, name=""):
    for k in keys:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (name, k)


def _run_fuse(ctx, name, c):
    b = rf.batch_fuse([c])
    masked = c.get("mask") is not None
    got = _fuse(ctx, b, c["cam_stride"], c["kp_stride"], masked)
    _hold(got, _fuse_ref(b, c["cam_stride"], c["kp_stride"], masked), rf.FUSE_OUTS, name)
    return got


def test_header_symbols_and_defaults(ctx):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_fuse.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.FUSE_SYMBOLS)
    assert not set(names) & (set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS) | set(capi.SEARCH_SYMBOLS) | set(capi.PNP_SYMBOLS))
    for nm in names:
        assert hasattr(ctx.lib, nm), nm
    p = capi.CullParams.make(ctx.lib)
    assert (p.inlier_px, p.min_good, p.mature_good, p.mature_age, p.good10) == tuple(rf.CULL_DEFAULTS[k] for k in ("inlier_px", "min_good", "mature_good", "mature_age", "good10"))
    assert p.inlier_px == capi.AdjustParams.make(ctx.lib).gate_px
    assert ctx.lib.vslam_cull_params_default(C.c_void_p(0)) == -1


def test_fuse_hand_cases(ctx):
    seen = np.zeros(4, np.int64)
    dropped = 0
    for name, c in fc.fuse_hand_cases().items():
        got = _run_fuse(ctx, name, c)
        assert np.array_equal(got["fuse_to"][0], c["expect"]), (name, got["fuse_to"][0])
        seen += got["stats"][0]
        if not name.startswith("broken") and c["n"] > 0:
            n = min(c["n"], len(c["expect"]))
            part = c["expect"][:n] >= 0
            valid = sum(1 for i in np.flatnonzero(part) for o in range(c["offsets"][i], c["offsets"][i + 1])
                        if 0 <= c["cam"][o] < c["cam_stride"] and 0 <= c["kp"][o] < c["kp_stride"])
            dropped += valid - got["stats"][0, 3]
    print("hand cases: taking part, groups, absorbed, kept", seen.tolist(), "duplicates dropped", dropped)
    assert seen[1] > 0 and seen[2] > 0 and dropped > 0


def _chain(order, S=None):
    """a chain of points: the j-th and the (j + 1)-th of `order` share cell (0, j + 1)"""
    n = len(order)
    S = S or n
    rows = [None] * n
    for j, i in enumerate(order):
        rows[i] = [(0, j), (0, j + 1)]
    offsets = np.concatenate([[0], np.cumsum([2] * n), [2 * n] * (S - n)]).astype(np.int32)
    flat = [e for r in rows for e in r]
    return dict(n=n, offsets=offsets, cam=np.array([e[0] for e in flat], np.int32), kp=np.array([e[1] for e in flat], np.int32), cam_stride=2,
                kp_stride=n + 1, mask=None)


def test_fuse_convergence_on_chains_and_one_crowded_cell(ctx):
    far = _chain(list(range(299, -1, -1)))                         # index 0 at the far end of the chain
    ends = [x for pair in zip(range(150), range(299, 149, -1)) for x in pair]
    alt = _chain(ends)                                             # 0, 299, 1, 298, ...: neighbours in the chain are far apart in index
    for name, c in (("far", far), ("alternating", alt)):
        got = _run_fuse(ctx, name, c)
        assert (got["fuse_to"][0] == 0).all() and got["stats"][0].tolist() == [300, 1, 299, 301], name
        assert got["out_offsets"][0, 1] == 301
    crowd = dict(n=1000, offsets=np.arange(0, 2002, 2, dtype=np.int32), cam=np.tile([1, 0], 1000).astype(np.int32),
                 kp=np.stack([np.full(1000, 7), np.arange(1000)], 1).reshape(-1).astype(np.int32), cam_stride=2, kp_stride=1000, mask=None)
    got = _run_fuse(ctx, "crowd", crowd)
    assert (got["fuse_to"][0] == 0).all() and got["stats"][0].tolist() == [1000, 1, 999, 1001]


@pytest.mark.parametrize("n", [255, 256, 257, 513, 5000])
def test_fuse_point_chunks(ctx, n):
    c = rf.random_fuse_item(900 + n, n, kp_stride=max(16, n // 2), S=n + 3)
    got = _run_fuse(ctx, f"n{n}", c)
    st = got["stats"][0]
    valid = int(((c["cam"] >= 0) & (c["cam"] < c["cam_stride"]) & (c["kp"] >= 0) & (c["kp"] < c["kp_stride"]))[:c["offsets"][n]].sum())
    print(f"n = {n}: taking part {st[0]}, groups with more than one member {st[1]}, absorbed {st[2]}, kept {st[3]} of {valid} valid entries")
    assert st[1] > 0 and st[2] > 0 and 0 < st[3] < valid and (got["fuse_to"][0, :n] < 0).any()
    if n == 5000:                                                   # and the same item without its mask: other groups
        other = _run_fuse(ctx, "unmasked", dict(c, mask=None))
        assert not np.array_equal(other["fuse_to"], got["fuse_to"])


@pytest.fixture(scope="module")
def three():
    items = [rf.random_fuse_item(31, 700, kp_stride=300), rf.random_fuse_item(32, 40, kp_stride=300), rf.random_fuse_item(33, 1300, kp_stride=300, obs=(1, 4))]
    b = rf.batch_fuse(items)
    return items, b, _fuse_ref(b, 6, 300)


def test_fuse_batch_of_three_items_of_different_sizes(ctx, three):
    items, b, ref = three
    got = _fuse(ctx, b, 6, 300)
    _hold(got, ref, rf.FUSE_OUTS)
    assert (got["stats"][:, 1] > 0).all() and (got["stats"][:, 2] > 0).all()


def test_fuse_one_item_same_bits_alone_in_any_slot_and_in_two_runs(ctx, three):
    items, b, ref = three
    one = {k: v[2:3] for k, v in b.items()}
    alone, again = _fuse(ctx, one, 6, 300), _fuse(ctx, one, 6, 300)
    _hold(alone, again, rf.FUSE_OUTS)
    for slot, src in ((0, [2, 0, 1]), (1, [0, 2, 1])):
        got = _fuse(ctx, {k: v[src] for k, v in b.items()}, 6, 300)
        for k in rf.FUSE_OUTS:
            assert np.array_equal(_bits(got[k][slot]), _bits(alone[k][0])), (slot, k)
    for k in rf.FUSE_OUTS:
        assert np.array_equal(_bits(alone[k][0]), _bits(ref[k][2])), k


def test_fuse_mask_may_be_the_output(ctx, three):
    """d_mask = d_fuse_to: a point's mask is read before its fuse_to is written"""
    items, b, ref = three
    B, S, O = b["offsets"].shape[0], b["offsets"].shape[1] - 1, b["cam"].shape[1]
    out = {k: _t(v) for k, v in _fprefill(B, S, O).items()}
    out["fuse_to"] = _t(b["mask"])
    ctx.fuse_points(_t(b["n"]), _t(b["offsets"]), _t(b["cam"]), _t(b["kp"]), 6, 300, out["fuse_to"], out=out)
    ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = dict(ref, fuse_to=ref["fuse_to"].copy())
    _hold(got, want, rf.FUSE_OUTS)


# ------------------------------------------------------------------------------------------------ the cull
def _cull_batch(items):
    S, O = max(len(it["points"]) for it in items), max(len(it["cam"]) for it in items)
    Cs, Kp = max(len(it["R"]) for it in items), max(it["xy"].shape[1] for it in items)
    B = len(items)
    b = dict(points=np.full((B, S, 4), np.nan, np.float32), n=np.array([it["n"] for it in items], np.int32), offsets=np.zeros((B, S + 1), np.int32),
             cam=np.zeros((B, O), np.int32), kp=np.zeros((B, O), np.int32), R=np.zeros((B, Cs, 9)), T=np.zeros((B, Cs, 3)),
             n_cams=np.array([it["n_cams"] for it in items], np.int32), xy=np.zeros((B, Cs, Kp, 2), np.float32))
    for i, it in enumerate(items):
        s, o, c, k = len(it["points"]), len(it["cam"]), len(it["R"]), it["xy"].shape[1]
        b["points"][i, :s], b["offsets"][i, :s + 1], b["offsets"][i, s + 1:] = it["points"], it["offsets"], it["offsets"][-1]
        b["cam"][i, :o], b["kp"][i, :o], b["R"][i, :c], b["T"][i, :c], b["xy"][i, :c, :k] = it["cam"], it["kp"], it["R"], it["T"], it["xy"]
    return b


def _cull(ctx, b, K, **params):
    B, S = b["points"].shape[:2]
    out = dict(keep=_t(np.full((B, S), CSENT["keep"], np.int32)), counts=_t(np.full((B, S, 2), CSENT["counts"], np.int32)),
               stats=_t(np.full((B, 4), CSENT["stats"], np.int32)))
    ctx.cull_points(_t(b["points"]), _t(b["n"]), _t(b["offsets"]), _t(b["cam"]), _t(b["kp"]), _t(b["R"]), _t(b["T"]), _t(b["n_cams"]), _t(b["xy"]), K,
                    out=out, **params)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _cull_ref(b, K, **params):
    return rf.cull_batch(b["points"], b["n"], b["offsets"], b["cam"], b["kp"], b["R"], b["T"], b["n_cams"], b["xy"], K, **params)


def test_cull_hand_case(ctx):
    c = fc.cull_hand_case()
    b = _cull_batch([c])
    got = _cull(ctx, b, c["K"])
    _hold(got, _cull_ref(b, c["K"]), rf.CULL_OUTS)
    assert np.array_equal(got["keep"][0], c["expect"]) and np.array_equal(got["counts"][0], c["expect_counts"])
    assert got["stats"][0, 1] > 0 and got["stats"][0, 2] > 0


@pytest.mark.parametrize("n,cams", [(257, 6), (257, 64), (5000, 6), (5000, 64)])
def test_cull_random_items(ctx, n, cams):
    c = rf.random_cull_item(10 * n + cams, n, cams, S=n + 3, cam_stride=cams + 1)
    b = _cull_batch([c])
    for params in ({}, dict(inlier_px=3.0, min_good=1, mature_good=4, mature_age=cams // 2, good10=8)):
        got = _cull(ctx, b, c["K"], **params)
        _hold(got, _cull_ref(b, c["K"], **params), rf.CULL_OUTS, (n, cams, params))
        st = got["stats"][0]
        print(f"n = {n}, {cams} cameras, {params or 'defaults'}: taking part {st[0]}, kept {st[1]}, culled {st[2]}, good observations {st[3]}")
        assert st[1] > 0 and st[2] > 0 and (got["keep"][0, :n] == -1).any() and 0 < st[3] < got["counts"][0, :, 0].sum()


def test_cull_batch_of_three_and_the_same_bits_in_any_slot_and_run(ctx):
    items = [rf.random_cull_item(41, 300, 6), rf.random_cull_item(42, 30, 4), rf.random_cull_item(43, 700, 9, obs=(1, 5))]
    b = _cull_batch(items)
    K = items[0]["K"]
    got = _cull(ctx, b, K)
    _hold(got, _cull_ref(b, K), rf.CULL_OUTS)
    assert (got["stats"][:, 1] > 0).all() and (got["stats"][:, 2] > 0).all()
    one = {k: v[2:3] for k, v in b.items()}
    alone, again = _cull(ctx, one, K), _cull(ctx, one, K)
    _hold(alone, again, rf.CULL_OUTS)
    moved = _cull(ctx, {k: v[[2, 1, 0]] for k, v in b.items()}, K)
    for k in rf.CULL_OUTS:
        assert np.array_equal(moved[k][0], alone[k][0]) and np.array_equal(got[k][2], alone[k][0]), k


# ------------------------------------------------------------------------------------------------ refusals, alignment, stream order
FARGS = ("n_points", "offsets", "cam", "kp", "mask", "fuse_to", "out_offsets", "out_cam", "out_kp", "out_src", "stats")
FOPTIONAL = ("mask", "out_src", "stats")


def _fuse_tensors(b):
    B, S, O = b["offsets"].shape[0], b["offsets"].shape[1] - 1, b["cam"].shape[1]
    d = dict(n_points=_t(b["n"]), offsets=_t(b["offsets"]), cam=_t(b["cam"]), kp=_t(b["kp"]), mask=_t(b["mask"]))
    d.update({k: _t(v) for k, v in _fprefill(B, S, O).items()})
    return d


def _fuse_raw(ctx, d, over=None, **sizes):
    B, S, O = d["offsets"].shape[0], d["offsets"].shape[1] - 1, d["cam"].shape[1]
    ptr = {k: d[k].data_ptr() for k in FARGS}
    ptr.update(over or {})
    sz = dict(pt_stride=S, obs_stride=O, cam_stride=6, kp_stride=300, batch=B)
    sz.update(sizes)
    v = lambda k: C.c_void_p(ptr[k])
    return ctx.lib.vslam_fuse_points(ctx.handle, v("n_points"), sz["pt_stride"], v("offsets"), v("cam"), v("kp"), sz["obs_stride"], sz["cam_stride"],
                                     sz["kp_stride"], v("mask"), sz["batch"], v("fuse_to"), v("out_offsets"), v("out_cam"), v("out_kp"), v("out_src"),
                                     v("stats"))


def test_fuse_refusals_before_anything_is_queued(ctx, three):
    items, b, ref = three
    one = {k: v[:1] for k, v in b.items()}
    d = _fuse_tensors(one)
    for k in FARGS:
        if k not in FOPTIONAL:
            assert _fuse_raw(ctx, d, over={k: 0}) == -1, k
    for kw in (dict(batch=0), dict(batch=-1), dict(pt_stride=0), dict(obs_stride=0), dict(cam_stride=0), dict(kp_stride=-2)):
        assert _fuse_raw(ctx, d, **kw) == -1, kw
    for kw in (dict(kp_stride=rf.MAX_KP + 1), dict(cam_stride=rf.MAX_CAMS + 1)):
        assert _fuse_raw(ctx, d, **kw) == -4, kw
    for k in FARGS:
        assert _fuse_raw(ctx, d, over={k: d[k].data_ptr() + 2}) == -1, k
        assert "d_" in ctx.lib.vslam_last_error(ctx.handle).decode()
    assert ctx.lib.vslam_fuse_points(C.c_void_p(0), C.c_void_p(0), 1, *[C.c_void_p(0)] * 3, 1, 1, 1, C.c_void_p(0), 1, *[C.c_void_p(0)] * 6) == -1
    ctx.synchronize()
    S, O = one["offsets"].shape[1] - 1, one["cam"].shape[1]
    fill = _fprefill(1, S, O)
    for k in rf.FUSE_OUTS:
        assert np.array_equal(d[k].cpu().numpy(), fill[k]), (k, "nothing ran")
    assert _fuse_raw(ctx, d) == 0                                    # and the next call is exact
    ctx.synchronize()
    _hold({k: d[k].cpu().numpy() for k in rf.FUSE_OUTS}, {k: v[:1] for k, v in ref.items()}, rf.FUSE_OUTS)
    d2 = _fuse_tensors(one)
    assert _fuse_raw(ctx, d2, over=dict(mask=0, out_src=0, stats=0)) == 0   # the optional ones may be NULL
    ctx.synchronize()
    want = _fuse_ref(one, 6, 300, masked=False)
    for k in rf.FUSE_OUTS:
        assert np.array_equal(d2[k].cpu().numpy(), fill[k] if k in ("out_src", "stats") else want[k]), k


def test_fuse_every_pointer_exactly_at_four_bytes_gives_the_aligned_bits(ctx, three):
    from offset_views import offset_view
    items, b, ref = three
    one = {k: v[:1] for k, v in b.items()}
    for nm in FARGS:
        d = _fuse_tensors(one)
        v, whole, check = offset_view(tuple(d[nm].shape), d[nm].dtype, 1)
        assert v.data_ptr() % 4 == 0 and v.data_ptr() % 8 != 0, nm
        v.copy_(d[nm])
        d[nm] = v
        assert _fuse_raw(ctx, d) == 0, nm
        ctx.synchronize()
        check(nm)
        _hold({k: d[k].cpu().numpy() for k in rf.FUSE_OUTS}, {k: x[:1] for k, x in ref.items()}, rf.FUSE_OUTS, nm)


CARGS = ("points", "n_points", "offsets", "cam", "kp", "R", "T", "n_cams", "xy", "keep", "counts", "stats")
CALIGN = dict(points=16, xy=8, R=8, T=8, n_points=4, offsets=4, cam=4, kp=4, n_cams=4, keep=4, counts=4, stats=4)


def _cull_tensors(b):
    B, S = b["points"].shape[:2]
    return dict(points=_t(b["points"]), n_points=_t(b["n"]), offsets=_t(b["offsets"]), cam=_t(b["cam"]), kp=_t(b["kp"]), R=_t(b["R"]), T=_t(b["T"]),
                n_cams=_t(b["n_cams"]), xy=_t(b["xy"]), keep=_t(np.full((B, S), CSENT["keep"], np.int32)),
                counts=_t(np.full((B, S, 2), CSENT["counts"], np.int32)), stats=_t(np.full((B, 4), CSENT["stats"], np.int32)))


def _cull_raw(ctx, d, K, over=None, params=None, K_over=None, **sizes):
    B, S, O, Cs, Kp = d["points"].shape[0], d["points"].shape[1], d["cam"].shape[1], d["R"].shape[1], d["xy"].shape[2]
    ptr = {k: d[k].data_ptr() for k in CARGS}
    ptr.update(over or {})
    sz = dict(pt_stride=S, obs_stride=O, cam_stride=Cs, kp_stride=Kp, batch=B)
    sz.update(sizes)
    Kh = np.ascontiguousarray(np.asarray(K if K_over is None or K_over is False else K_over, np.float32).reshape(9))
    v = lambda k: C.c_void_p(ptr[k])
    return ctx.lib.vslam_cull_points(ctx.handle, v("points"), v("n_points"), sz["pt_stride"], v("offsets"), v("cam"), v("kp"), sz["obs_stride"], v("R"),
                                     v("T"), v("n_cams"), sz["cam_stride"], v("xy"), sz["kp_stride"],
                                     Kh.ctypes.data_as(C.c_void_p) if K_over is not False else C.c_void_p(0), sz["batch"],
                                     C.byref(params) if params is not None else C.c_void_p(0), v("keep"), v("counts"), v("stats"))


@pytest.fixture(scope="module")
def cull_one():
    c = rf.random_cull_item(51, 300, 6)
    b = _cull_batch([c])
    return c, b, _cull_ref(b, c["K"])


def test_cull_refusals_before_anything_is_queued(ctx, cull_one):
    c, b, ref = cull_one
    K = c["K"]
    d = _cull_tensors(b)
    for bad in (dict(inlier_px=0.0), dict(inlier_px=-1.0), dict(inlier_px=float("nan")), dict(inlier_px=float("inf")), dict(min_good=0),
                dict(mature_good=0), dict(mature_age=-1), dict(mature_age=(1 << 20) + 1), dict(good10=-1), dict(good10=11)):
        assert _cull_raw(ctx, d, K, params=capi.CullParams.make(ctx.lib, **bad)) == -1, bad
    for k in CARGS:
        if k != "counts":
            assert _cull_raw(ctx, d, K, over={k: 0}) == -1, k
    assert _cull_raw(ctx, d, K, K_over=False) == -1
    for kw in (dict(batch=0), dict(pt_stride=0), dict(obs_stride=-1), dict(cam_stride=0), dict(kp_stride=0)):
        assert _cull_raw(ctx, d, K, **kw) == -1, kw
    for bad in (float("nan"), float("inf")):
        Kb = np.array(K, np.float32).copy()
        Kb[1, 2] = bad
        assert _cull_raw(ctx, d, K, K_over=Kb) == -1
    for kw in (dict(kp_stride=rf.MAX_KP + 1), dict(cam_stride=rf.MAX_CAMS + 1)):
        assert _cull_raw(ctx, d, K, **kw) == -4, kw
    for k, need in CALIGN.items():
        assert _cull_raw(ctx, d, K, over={k: d[k].data_ptr() + need // 2}) == -1, k
        assert "d_" in ctx.lib.vslam_last_error(ctx.handle).decode()
    ctx.synchronize()
    for k in rf.CULL_OUTS:
        assert (d[k].cpu().numpy() == CSENT[k]).all(), (k, "nothing ran")
    assert _cull_raw(ctx, d, K) == 0
    ctx.synchronize()
    _hold({k: d[k].cpu().numpy() for k in rf.CULL_OUTS}, ref, rf.CULL_OUTS)
    d2 = _cull_tensors(b)
    assert _cull_raw(ctx, d2, K, over=dict(counts=0)) == 0              # params and d_counts may be NULL
    ctx.synchronize()
    assert np.array_equal(d2["keep"].cpu().numpy(), ref["keep"]) and (d2["counts"].cpu().numpy() == CSENT["counts"]).all()


def test_cull_every_pointer_exactly_at_its_alignment_gives_the_aligned_bits(ctx, cull_one):
    from offset_views import offset_view
    c, b, ref = cull_one
    for nm, need in CALIGN.items():
        d = _cull_tensors(b)
        v, whole, check = offset_view(tuple(d[nm].shape), d[nm].dtype, need // d[nm].element_size())
        assert v.data_ptr() % need == 0 and v.data_ptr() % (2 * need) != 0, nm
        v.copy_(d[nm])
        d[nm] = v
        assert _cull_raw(ctx, d, c["K"]) == 0, nm
        ctx.synchronize()
        check(nm)
        _hold({k: d[k].cpu().numpy() for k in rf.CULL_OUTS}, ref, rf.CULL_OUTS, nm)


def _behind_stall(make, entry, check):
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = capi.Context(0)
        try:
            call, other = make(0), make(1)
            decoys = Decoys(call, other, None)
            sizing = choose_sizing(ctx, [call], stream)
            print("stream order:", sizing)
            res = run_behind_stall(ctx, call, stream, decoys, sizing)
            assert res.rc == 0, res.msg
            assert res.pending_at_return, f"{entry} waited for the device before it returned"
            assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
            assert set(res.got) == set(res.expected)
            for k in res.expected:
                assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"
            check(res.got)
        finally:
            ctx.close()


def test_fuse_stream_order_behind_a_stalled_stream():
    import header_calls as hc
    items = [rf.random_fuse_item(61, 600, kp_stride=300), rf.random_fuse_item(62, 600, kp_stride=300)]
    O = max(len(it["cam"]) for it in items)

    def make(i):
        it = items[i]
        b = rf.batch_fuse([dict(it, cam=np.concatenate([it["cam"], np.zeros(O - len(it["cam"]), np.int32)]),
                                kp=np.concatenate([it["kp"], np.zeros(O - len(it["kp"]), np.int32)]))])
        return hc.fuse_points({k: _t(b[k]) for k in ("n", "offsets", "cam", "kp", "mask")}, 6, 300)

    def check(got):
        st = np.frombuffer(got["d_stats"].tobytes(), np.int32)
        assert st[1] > 0 and st[2] > 0
    _behind_stall(make, "vslam_fuse_points", check)


def test_cull_stream_order_behind_a_stalled_stream():
    import header_calls as hc
    items = [rf.random_cull_item(71, 600, 6), rf.random_cull_item(72, 600, 6)]
    both = _cull_batch(items)                                          # one shape for the call and its decoys

    def make(i):
        return hc.cull_points({k: _t(v[i:i + 1]) for k, v in both.items()}, items[i]["K"])

    def check(got):
        st = np.frombuffer(got["d_stats"].tobytes(), np.int32)
        assert st[1] > 0 and st[2] > 0
    _behind_stall(make, "vslam_cull_points", check)


# ------------------------------------------------------------------------------------------------ on the world
from test_gpu_pnp import SCENE_KP, SCENE_MCAP, SCENE_OCAP, _restore, _scene_map  # noqa: E402
from test_gpu_world import _same  # noqa: E402

MAP_KEYS = ("points", "colors", "sizes", "map_point_ids", "R_t", "pose", "obs_counts", "n_obs")


@pytest.fixture(scope="module")
def scenes():
    return [pc.first_world_scene(60)[1], pc.first_world_scene(400)[1]]


def _xy_all(scenes, frames=6):
    xy = np.zeros((len(scenes), frames, SCENE_KP, 2), np.float32)
    desc = np.zeros((len(scenes), frames, SCENE_KP, 32), np.uint8)
    for t, ws in enumerate(scenes):
        for f in range(frames):
            xy[t, f, :ws["n"]], desc[t, f, :ws["n"]] = ws["xy"][f], ws["desc"][f]
    return xy, desc


def _np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _ref_world_fuse(view, off, fr, kp, fuse_to=None):
    """tests/ref_fuse.world_fuse for every track of a view -> (results, fuse_to after, world_points after)"""
    T = len(view["sizes"])
    P = view["world_points"].shape[1]
    prev = np.tile(np.arange(P, dtype=np.int32), (T, 1)) if fuse_to is None else fuse_to
    rs, to, wp = [], [], []
    for t in range(T):
        r, f, w = rf.world_fuse(prev[t], view["world_points"][t], view["sizes"][t], off[t], fr[t], kp[t], 6, SCENE_KP)
        rs.append(r); to.append(f); wp.append(w)
    return rs, np.stack(to), np.stack(wp)


def _hold_csr(got, rs, desc_of=None):
    """(offsets, frame, kp, desc) of World.observations against the reference's merged rows, track by track"""
    off, fr, kp, desc = got
    for t, r in enumerate(rs):
        total = len(r["out_cam"])
        assert np.array_equal(off[t], r["out_offsets"]), t
        assert np.array_equal(fr[t, :total], r["out_cam"]) and np.array_equal(kp[t, :total], r["out_kp"]), t
        assert (fr[t, total:] == -1).all() and (kp[t, total:] == -1).all(), "slots past the total keep their bits"
        if desc_of is not None:
            assert np.array_equal(desc[t, :total], desc_of[t][r["out_cam"], r["out_kp"]]), t
            assert not desc[t, total:].any()


def test_world_fuse_observations_and_the_consumers(ctx, scenes):
    a, wa, cur = _scene_map(ctx, scenes)
    try:
        T = len(scenes)
        xy_all, desc_all = _xy_all(scenes)
        before = a.view()
        assert "world_fuse_to" not in before
        moff, mfr, mkp = _np(a.observations())
        own = _np(wa.observations(a))
        assert np.array_equal(own[0], moff) and np.array_equal(own[1], mfr) and np.array_equal(own[2], mkp), "no fusion: the map's own CSR"
        unfused_search = wa.search(a, cur, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H)
        stats = wa.fuse(a)
        ctx.synchronize()
        after = a.view()
        rs, to, wp = _ref_world_fuse(before, moff, mfr, mkp)
        st = stats.cpu().numpy()
        print("fuse: taking part, groups with more than one member, absorbed, kept:", st.tolist(), "of", [int(moff[t, before['sizes'][t]]) for t in range(T)], "entries")
        assert np.array_equal(st, np.stack([r["stats"] for r in rs])) and (st[:, 1] > 0).all() and (st[:, 2] > 0).all()
        assert all(st[t, 3] < moff[t, before["sizes"][t]] for t in range(T)), "duplicates dropped"
        assert np.array_equal(after["world_fuse_to"], to)
        assert np.array_equal(_bits(after["world_points"]), _bits(wp)), "NaN rows for the absorbed, every other row its own bits"
        absorbed = (to >= 0) & (to != np.arange(to.shape[1])[None, :])
        assert (after["world_points"].view(np.uint32)[absorbed] == [0x7FC00000] * 3 + [0]).all() and absorbed.any()
        _same(before, after, keys=[k for k in before if k != "world_points"])          # every array of the map, the rest of the world
        assert all(k in before for k in MAP_KEYS)
        _hold_csr(_np(wa.observations(a)), rs, desc_all)
        moff2, mfr2, mkp2 = _np(a.observations())
        assert np.array_equal(moff2, moff) and np.array_equal(mfr2, mfr) and np.array_equal(mkp2, mkp), "the map's log keeps its bits"

        # the three consumers = the batch entry points fed by hand with the merged CSR
        off_m, fr_m, kp_m, desc_m = wa.observations(a)
        wp_t, sizes_t = _t(after["world_points"]), _t(after["sizes"])
        from test_gpu_pnp import _pose_of
        RT = [_pose_of(after["world_Twc"][t, 5]) for t in range(T)]
        hand = ctx.search_projection(wp_t, sizes_t, off_m, desc_m, _t(np.stack([x[0] for x in RT])), _t(np.stack([x[1] for x in RT])), pc.SCENE_K,
                                     pc.SCENE_W, pc.SCENE_H, cur["xy"], cur["desc"], cur["n"])
        got = wa.search(a, cur, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H)
        ctx.synchronize()
        n = hand["n_corr"].cpu().numpy()
        assert np.array_equal(got["n_corr"].cpu().numpy(), n) and (n >= 8).all()
        for k in ("corr_point", "corr_kp"):
            for t in range(T):
                assert np.array_equal(got[k].cpu().numpy()[t, :n[t]], hand[k].cpu().numpy()[t, :n[t]]), (k, t)
        found = got["corr_point"].cpu().numpy()
        assert all(not absorbed[t, found[t, :n[t]]].any() for t in range(T)), "an absorbed point is invisible"
        print("search: found", n.tolist(), "after the fusion,", unfused_search["n_corr"].cpu().numpy().tolist(), "before it")
        _same(after, a.view())

        seeds = torch.arange(1, T + 1, dtype=torch.int32).cuda()
        mt = ctx.match_points(wp_t, sizes_t, off_m, desc_m, cur["xy"], cur["desc"], cur["n"])
        R0, T0 = _t(np.tile(pc.KEEP_R, (T, 1))), _t(np.tile(pc.KEEP_T, (T, 1)))
        pn = ctx.pnp_ransac(mt["corr_points"], mt["corr_xy"], mt["n_corr"], pc.SCENE_K, seeds, R0, T0, polish={})
        rl = wa.relocalise(a, cur, pc.SCENE_K)
        ctx.synchronize()
        assert np.array_equal(rl["n_corr"].cpu().numpy(), mt["n_corr"].cpu().numpy()) and (rl["found"].cpu().numpy() == 1).all()
        for k in ("winner", "n_inliers"):
            assert np.array_equal(rl[k].cpu().numpy(), pn[k].cpu().numpy()), k
        assert np.array_equal(_bits(rl["stats"].cpu().numpy()), _bits(pn["stats"].cpu().numpy()))
        _restore(ctx, wa, after)

        # the adjustment: the window gathered by hand from the merged CSR
        off_n, fr_n, kp_n = off_m.cpu().numpy(), fr_m.cpu().numpy(), kp_m.cpu().numpy()
        P, O = SCENE_MCAP, SCENE_OCAP
        R, Tv = np.zeros((T, 8, 9)), np.zeros((T, 8, 3))
        X = after["world_points"][:, :, :3].astype(np.float64)
        offs, cams, oxy = np.zeros((T, P + 1), np.int32), np.zeros((T, O), np.int32), np.zeros((T, O, 2), np.float32)
        for t in range(T):
            for f in range(6):
                R[t, f], Tv[t, f] = _pose_of(after["world_Twc"][t, f])
            N = int(after["sizes"][t])
            tot = off_n[t, N]
            cams[t, :tot], oxy[t, :tot] = fr_n[t, :tot], xy_all[t, fr_n[t, :tot], kp_n[t, :tot]]
            offs[t, :N + 1] = off_n[t, :N + 1]
        _, _, _, st_hand = ctx.adjust_windows(_t(R), _t(Tv), _t(np.full(T, 6, np.int32)), _t(X), sizes_t, _t(offs), _t(cams), _t(oxy), pc.SCENE_K)
        st_world = wa.adjust(a, _t(xy_all), pc.SCENE_K)
        ctx.synchronize()
        assert np.array_equal(_bits(st_world.cpu().numpy()), _bits(st_hand.cpu().numpy()))
        print("adjust after the fusion: participants, mean rho before / after, accepted", st_world.cpu().numpy().tolist())
        assert (st_world.cpu().numpy()[:, 0] > 0).all()

        # reset: every world call back to its bits without a fusion
        a.reset()
        ctx.synchronize()
        assert "world_fuse_to" not in a.view()
    finally:
        a.close(); wa.close()


def test_fusing_gives_the_adjustment_more_observations_per_point(ctx, scenes):
    """Derived, not measured: a merged row is the union of its members' rows, so among the points the adjustment can use (a finite
    world point with a non-empty row) the observations per point can only grow, and grow strictly where a group has two members
    with different observations."""
    a, wa, cur = _scene_map(ctx, scenes)
    try:
        xy_all, _ = _xy_all(scenes)

        def per_point():
            off = wa.observations(a, desc=False)[0].cpu().numpy()
            v = a.view()
            out = []
            for t in range(len(scenes)):
                rows = np.diff(off[t, :v["sizes"][t] + 1])
                usable = np.isfinite(v["world_points"][t, :v["sizes"][t], :3]).all(1) & (rows > 0)
                out.append((rows[usable].mean(), rows[usable].max(), int(usable.sum())))
            return out
        unfused = per_point()
        st0 = wa.adjust(a, _t(xy_all), pc.SCENE_K).cpu().numpy()
        a2, wa2, _ = _scene_map(ctx, scenes)
        try:
            wa2.fuse(a2)
            off = wa2.observations(a2, desc=False)[0].cpu().numpy()
            v = a2.view()
            fused = []
            for t in range(len(scenes)):
                rows = np.diff(off[t, :v["sizes"][t] + 1])
                usable = np.isfinite(v["world_points"][t, :v["sizes"][t], :3]).all(1) & (rows > 0)
                fused.append((rows[usable].mean(), rows[usable].max(), int(usable.sum())))
            st1 = wa2.adjust(a2, _t(xy_all), pc.SCENE_K).cpu().numpy()
        finally:
            a2.close(); wa2.close()
        for t in range(len(scenes)):
            print(f"track {t}: observations per usable point {unfused[t][0]:.2f} (max {unfused[t][1]}, {unfused[t][2]} points) -> "
                  f"{fused[t][0]:.2f} (max {fused[t][1]}, {fused[t][2]} points); adjustment participants {st0[t, 0]:.0f} -> {st1[t, 0]:.0f}")
            assert fused[t][0] > unfused[t][0] and fused[t][1] >= unfused[t][1] and fused[t][2] < unfused[t][2]
    finally:
        a.close(); wa.close()


def test_world_cull_and_a_second_fuse(ctx, scenes):
    a, wa, cur = _scene_map(ctx, scenes)
    try:
        T = len(scenes)
        xy_all, desc_all = _xy_all(scenes)
        rng = np.random.default_rng(5)
        noisy = xy_all.copy()
        for t, ws in enumerate(scenes):
            bad = rng.permutation(ws["n"])[:ws["n"] // 5]
            noisy[t, 3, bad] = rng.uniform(0, [pc.SCENE_W, pc.SCENE_H], (len(bad), 2)).astype(np.float32)
        before = a.view()
        moff, mfr, mkp = _np(a.observations())
        wa.fuse(a)
        ctx.synchronize()
        fused = a.view()
        rs, to, wp = _ref_world_fuse(before, moff, mfr, mkp)
        strict = dict(good10=10)                                       # one bad observation culls: groups with members among the culled
        stats = wa.cull(a, _t(noisy), pc.SCENE_K, **strict)
        ctx.synchronize()
        after = a.view()
        st = stats.cpu().numpy()
        want_to, want_wp = [], []
        for t in range(T):
            R, Tv = rf.cameras(fused["world_Twc"][t], 6)
            total = len(rs[t]["out_cam"])
            cam, kp = np.zeros(SCENE_OCAP, np.int32), np.zeros(SCENE_OCAP, np.int32)
            cam[:total], kp[:total] = rs[t]["out_cam"], rs[t]["out_kp"]
            c = rf.cull_item(fused["world_points"][t], fused["sizes"][t], rs[t]["out_offsets"], cam, kp, R, Tv, 6, noisy[t], pc.SCENE_K, **strict)
            assert np.array_equal(st[t], c["stats"]), (t, st[t], c["stats"])
            f, w = rf.world_cull_apply(to[t], fused["world_points"][t], c["keep"])
            want_to.append(f); want_wp.append(w)
            members = int(((to[t] >= 0) & (to[t] != np.arange(len(f))) & (f == -1)).sum())
            print(f"track {t}: taking part {st[t, 0]}, kept {st[t, 1]}, culled {st[t, 2]}, good observations {st[t, 3]}; members of culled survivors {members}")
        assert (st[:, 1] > 0).all() and (st[:, 2] > 0).all()
        assert np.array_equal(after["world_fuse_to"], np.stack(want_to))
        assert np.array_equal(_bits(after["world_points"]), _bits(np.stack(want_wp)))
        assert any((((to[t] >= 0) & (to[t] != np.arange(to.shape[1])) & (want_to[t] == -1)).any()) for t in range(T)), "a culled survivor with members"
        _same(fused, after, keys=[k for k in fused if k not in ("world_points", "world_fuse_to")])
        # a second fuse: from scratch on the map's log, the culled points masked
        rs2, to2, wp2 = _ref_world_fuse(after, moff, mfr, mkp, after["world_fuse_to"])
        st2 = wa.fuse(a).cpu().numpy()
        ctx.synchronize()
        again = a.view()
        assert np.array_equal(st2, np.stack([r["stats"] for r in rs2])) and (st2[:, 0] < st[:, 0] + np.stack([r["stats"] for r in rs])[:, 2]).all()
        assert np.array_equal(again["world_fuse_to"], to2) and np.array_equal(_bits(again["world_points"]), _bits(wp2))
        assert (again["world_fuse_to"][after["world_fuse_to"] == -1] == -1).all(), "culled points stay culled"
        _hold_csr(_np(wa.observations(a)), rs2, desc_all)
        # the world's calls still run on what is left
        got = wa.search(a, cur, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H)
        ctx.synchronize()
        found, n = got["corr_point"].cpu().numpy(), got["n_corr"].cpu().numpy()
        assert (n >= 8).all() and all((again["world_fuse_to"][t, found[t, :n[t]]] == found[t, :n[t]]).all() for t in range(T))
    finally:
        a.close(); wa.close()


def _frame(ctx, scenes, f):
    T = len(scenes)
    xy, desc = np.zeros((T, SCENE_KP, 2), np.float32), np.zeros((T, SCENE_KP, 32), np.uint8)
    for t, ws in enumerate(scenes):
        xy[t, :ws["n"]], desc[t, :ws["n"]] = ws["xy"][f], ws["desc"][f]
    d = dict(xy=_t(xy), desc=_t(desc), n=_t(np.array([ws["n"] for ws in scenes], np.int32)))
    d["nodes"] = ctx.kdtree_build(d["xy"], d["n"])
    return d


def _step(ctx, a, scenes, f, last, bgr):
    """one step of test_gpu_pnp._scene_map's loop: frame f behind `last`"""
    T = len(scenes)
    cur = _frame(ctx, scenes, f)
    matches, best, F = np.zeros((T, SCENE_KP, 2), np.int32), np.zeros((T, 4), np.int32), np.zeros((T, 9), np.float32)
    for t, ws in enumerate(scenes):
        m = ws["pairs"][f - 1]["matches"]
        matches[t, :len(m)], best[t], F[t] = m, (0, len(m), 0, len(m)), ws["pairs"][f - 1]["F"]
    a.step(last, cur, dict(matches=_t(matches), best=_t(best), F=_t(F)), bgr, pc.SCENE_K)
    return cur


def test_a_fuse_between_steps_and_reset(ctx, scenes):
    """Three steps, a fusion, two more steps: the world's CSR follows the log at once (it is formed where it is read); the second
    vslam_world_fuse equals a from-scratch reference on the whole log and turns the rows of the points absorbed since to NaN; a reset
    puts every world call back to the bits of a map that was never fused."""
    T = len(scenes)
    a = capi.PointMap(ctx, T, 6, SCENE_KP, SCENE_MCAP, SCENE_OCAP)
    wa = a.attach_world()
    bgr = torch.full((T, pc.SCENE_H, pc.SCENE_W, 3), 90, dtype=torch.uint8).cuda()
    try:
        def steps(lo, hi, last):
            for f in range(lo, hi):
                last = _step(ctx, a, scenes, f, last, bgr)
            ctx.synchronize()
            return last
        last = steps(1, 4, _frame(ctx, scenes, 0))
        v3 = a.view()
        o3 = _np(a.observations())
        wa.fuse(a)
        ctx.synchronize()
        rs3, to3, wp3 = _ref_world_fuse(v3, *o3)
        f3 = a.view()
        assert np.array_equal(f3["world_fuse_to"], to3) and np.array_equal(_bits(f3["world_points"]), _bits(wp3))
        last = steps(4, 6, last)
        v5 = a.view()
        o5 = _np(a.observations())
        assert (v5["sizes"] > v3["sizes"]).all() and np.array_equal(v5["world_fuse_to"], to3), "a step leaves d_fuse_to alone"
        rs5, to5, wp5 = _ref_world_fuse(v5, *o5, v5["world_fuse_to"])
        _hold_csr(_np(wa.observations(a, desc=False)), rs5)              # before the second fuse: already the whole log's groups
        st = wa.fuse(a).cpu().numpy()
        ctx.synchronize()
        f5 = a.view()
        assert np.array_equal(st, np.stack([r["stats"] for r in rs5]))
        assert np.array_equal(f5["world_fuse_to"], to5) and np.array_equal(_bits(f5["world_points"]), _bits(wp5))
        newly = np.isnan(f5["world_points"][:, :, 0]) & ~np.isnan(v5["world_points"][:, :, 0])
        grown = [int(((to5[t] != np.arange(to5.shape[1])) & (to3[t] == np.arange(to5.shape[1])) & (np.arange(to5.shape[1]) < v3["sizes"][t])).sum()) for t in range(T)]
        print("absorbed by the second fuse:", newly.sum(1).tolist(), "of them points that stood for themselves after the first:", grown)
        assert newly.any(1).all()
        # the same scenes on a map never fused = this one after a reset and the same steps
        b, wb, cur_b = _scene_map(ctx, scenes)
        try:
            want_search = wb.search(b, cur_b, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H)
            want_obs = _np(wb.observations(b))
            want_view = b.view()
        finally:
            b.close(); wb.close()
        a.reset()
        last = steps(1, 6, _frame(ctx, scenes, 0))
        got_view = a.view()
        assert "world_fuse_to" not in got_view
        _same(want_view, got_view)
        got_search = wa.search(a, last, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H)
        got_obs = _np(wa.observations(a))
        ctx.synchronize()
        for k in want_search:
            assert np.array_equal(got_search[k].cpu().numpy(), want_search[k].cpu().numpy()), k
        for x, y in zip(got_obs, want_obs):
            assert np.array_equal(x, y)
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
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            other.fuse(a)                                                # not the world attached to that map
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            other.cull(a, xy, pc.SCENE_K)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            other.observations(a)
        for bad in (dict(inlier_px=0.0), dict(min_good=0), dict(mature_good=0), dict(mature_age=-1), dict(good10=11)):
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                wa.cull(a, xy, pc.SCENE_K, **bad)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.cull(a, _t(xy_all[:, :5]), pc.SCENE_K)                    # fewer frames of keypoints than recorded
        Kb = pc.SCENE_K.copy()
        Kb[0, 0] = np.inf
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            wa.cull(a, xy, Kb)
        st = torch.full((T, 4), 5, dtype=torch.int32).cuda()
        Kh = np.ascontiguousarray(pc.SCENE_K.reshape(9))
        lib, h = ctx.lib, ctx.handle
        null = C.c_void_p(0)
        assert lib.vslam_world_fuse(h, null, a.handle, null) == -1 and lib.vslam_world_fuse(h, wa.handle, null, null) == -1
        assert lib.vslam_world_fuse(h, wa.handle, a.handle, C.c_void_p(st.data_ptr() + 2)) == -1
        kp = Kh.ctypes.data_as(C.c_void_p)
        assert lib.vslam_world_cull(h, wa.handle, a.handle, null, 6, kp, null, null) == -1
        assert lib.vslam_world_cull(h, wa.handle, a.handle, C.c_void_p(xy.data_ptr()), 6, null, null, null) == -1
        assert lib.vslam_world_cull(h, wa.handle, a.handle, C.c_void_p(xy.data_ptr() + 4), 6, kp, null, null) == -1
        assert lib.vslam_world_cull(h, wa.handle, a.handle, C.c_void_p(xy.data_ptr()), 6, kp, null, C.c_void_p(st.data_ptr() + 2)) == -1
        off, fr, pt, d = wa.observations(a)
        for k, (bad_ptr) in dict(off=off.data_ptr() + 2, fr=fr.data_ptr() + 2, pt=0, d=d.data_ptr() + 8).items():
            p = dict(off=off.data_ptr(), fr=fr.data_ptr(), pt=pt.data_ptr(), d=d.data_ptr())
            p[k] = bad_ptr
            assert lib.vslam_world_observations(h, wa.handle, a.handle, *[C.c_void_p(p[x]) for x in ("off", "fr", "pt", "d")]) == -1, k
        assert lib.vslam_world_fusion_view(null, null, null) == -1
        ctx.synchronize()
        after = a.view()
        assert "world_fuse_to" not in after and (st.cpu().numpy() == 5).all(), "nothing ran"
        _same(before, after)
        assert lib.vslam_world_fuse(h, wa.handle, a.handle, null) == 0   # d_stats may be NULL
        ctx.synchronize()
        assert "world_fuse_to" in a.view()
    finally:
        a.close(); wa.close(); other.close()


def test_world_fuse_stream_order_behind_a_stalled_stream(ctx, scenes):
    """vslam_world_cull (its inputs are device arrays; vslam_world_fuse takes none) on the session's context, as
    test_gpu_pnp.test_world_relocalise_stream_order_behind_a_stalled_stream does it: the keypoints are the inputs, a noisy copy the
    decoys; the world is put back before every run and what the call leaves in it is compared beside its statistics."""
    import header_calls as hc
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
        fv = C.c_void_p()
        ctx._check(ctx.lib.vslam_world_fusion_view(wa.handle, C.byref(fv), C.c_void_p(0)))
        from test_gpu_pnp import _put

        def before():
            _put(ctx, wa.arrays().d_world_points, start["world_points"])
            _put(ctx, fv.value, start["world_fuse_to"])

        def state():
            v = a.view()
            return {k: v[k] for k in ("world_points", "world_fuse_to", "world_Twc", "points", "sizes")}

        def make(noise):
            xy = xy_all.copy()
            if noise:
                rng = np.random.default_rng(noise)
                xy[:, 2:] += rng.uniform(-30, 30, xy[:, 2:].shape).astype(np.float32)
            return hc.world_cull(wa, a, _t(xy), 6, pc.SCENE_K, before, state)
        call, other = make(0), make(9)
        decoys = Decoys(call, other, None)
        sizing = choose_sizing(ctx, [call], stream)
        res = run_behind_stall(ctx, call, stream, decoys, sizing)
        assert res.rc == 0, res.msg
        assert res.pending_at_return, "vslam_world_cull waited for the device before it returned"
        assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
        assert set(res.got) == set(res.expected)
        for k in res.expected:
            assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"
        st = np.frombuffer(res.got["d_stats"].tobytes(), np.int32).reshape(T, 4)
        assert (st[:, 1] > 0).all() and (st[:, 2] > 0).all()
    finally:
        a.close(); wa.close()


# ------------------------------------------------------------------------------------------------ C++ surfaces
def test_cpp_surfaces_match_the_c_entry_points(ctx, three, cull_one, tmp_path):
    """tests/native/fuse_demo.cpp: vslam::fuse_points and vslam::cull_points (include/vslam/helpers.h) on one item each give the bits of
    the C entry points; vslam::World::fuse / cull / observations / fuse_to (include/vslam/World.h) are taken on a world attached to a
    map and World::fuse throws on one that is not."""
    import struct
    import subprocess
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path / "fuse_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "fuse_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    items, b, ref = three
    c, cb, cref = cull_one
    S, O = b["offsets"].shape[1] - 1, b["cam"].shape[1]
    cS, cO, Cs, Kp = cb["points"].shape[1], cb["cam"].shape[1], cb["R"].shape[1], cb["xy"].shape[2]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("5i", S, O, int(b["n"][0]), 6, 300))
        for k in ("offsets", "cam", "kp", "mask"):
            f.write(np.ascontiguousarray(b[k][0], np.int32).tobytes())
        f.write(struct.pack("6i", cS, cO, int(cb["n"][0]), Cs, int(cb["n_cams"][0]), Kp))
        f.write(np.asarray(c["K"], np.float32).tobytes())
        for k, dt in (("points", np.float32), ("offsets", np.int32), ("cam", np.int32), ("kp", np.int32), ("R", np.float64), ("T", np.float64),
                      ("xy", np.float32)):
            f.write(np.ascontiguousarray(cb[k][0], dt).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    zero = {k: np.zeros_like(v[:1]) for k, v in _fprefill(1, S, O).items()}
    one = {k: v[:1] for k, v in b.items()}
    want_f = rf.fuse_batch(one["n"], one["offsets"], one["cam"], one["kp"], 6, 300, one["mask"], prefill=zero)
    want = b"".join(np.ascontiguousarray(want_f[k], np.int32).tobytes() for k in rf.FUSE_OUTS)
    want += b"".join(np.ascontiguousarray(cref[k], np.int32).tobytes() for k in rf.CULL_OUTS)
    assert want_f["stats"][0, 2] > 0 and cref["stats"][0, 1] > 0 and cref["stats"][0, 2] > 0
    assert buf[:len(want)] == want
    tail = np.frombuffer(buf[len(want):], np.int32)
    assert not tail[:16].any(), "an empty attached map: nothing takes part in the fusion or the cull"
    assert tail[16] == 3 and not tail[17:17 + 2 * 33].any() and tail[-1] == 1, "fused and culled; empty rows; a world that is not attached is refused"
