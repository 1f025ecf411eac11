"""include/vslam_sim3.h on the device.  vslam_sim3_ransac against the serial program and the reference:

Every count of every hypothesis, the winner, the mask, the number of inliers, the compacted indices AND the unpolished (s, R, t) are
held EXACTLY to tests/native/sim3_serial.cpp -- the same header (vslam_amd/csrc/sim3_math.h) compiled unfused for the host -- and
through it to tests/ref_sim3.py, which the serial walk equals bit for bit (tests/test_sim3_serial.py).  The polish is held within
16 x ref_sim3.DELTA_REF of the reference.  Outputs are written over a sentinel fill and compared whole: what the rule does not
write keeps the caller's bits.  vslam_world_sim3 and vslam_world_apply_sim3 are held to the same reference on two tracks of one map and
world: on the map as vslam_map_step leaves it (where its ids are too sparse for a pair to be found: the test says why) and on the
same map with the ids, sizes and world of tests/sim3_cases.ref_tracks written into it -- integers and the unpolished similarities
bit for bit, every array apply_sim3 writes bit for bit, every array it must not write unchanged, the fusion followed."""
import numpy as np
import pytest
import torch

import ref_resect as rr
import ref_sim3 as r3
import sim3_cases as sc3
from vslam_amd import capi

pytestmark = pytest.mark.gpu
C = capi.C
SENT = dict(inlier=77, corr_index=79, n_inliers=81, winner=82, counts=83, stats=9.5)
TOL_POLISHED = 16 * r3.DELTA_REF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sc3.build_serial(tmp_path_factory.mktemp("sim3_serial"))


def _batch(cases, extra=0):
    """cases that share params and polish -> the arrays of one call; rows past each item's own (and `extra` more) are NaN"""
    Bt, S = len(cases), max(len(c["A"]) for c in cases) + extra
    b = dict(A=np.full((Bt, S, 3), np.nan), B=np.full((Bt, S, 3), np.nan), xa=np.full((Bt, S, 2), np.nan, np.float32),
             xb=np.full((Bt, S, 2), np.nan, np.float32), n=np.zeros(Bt, np.int32), seeds=np.zeros(Bt, np.uint32),
             scale=np.full(Bt, sc3.KEEP_S), R=np.tile(sc3.KEEP_R, (Bt, 1)), T=np.tile(sc3.KEEP_T, (Bt, 1)))
    for i, c in enumerate(cases):
        m = len(c["A"])
        for k in ("A", "B", "xa", "xb"):
            b[k][i, :m] = c[k]
        b["n"][i], b["seeds"][i] = c["n"], c["seed"] & 0xFFFFFFFF
    return b


def _prefill(Bt, S, H):
    shapes = dict(inlier=((Bt, S), np.int32), corr_index=((Bt, S), np.int32), n_inliers=((Bt,), np.int32), winner=((Bt,), np.int32),
                  counts=((Bt, H), np.int32), stats=((Bt, 4), np.float64))
    return {k: np.full(s, SENT[k], t) for k, (s, t) in shapes.items()}


def _cuda(b):
    return {k: torch.from_numpy(v.view(np.int32) if k == "seeds" else v).cuda() for k, v in b.items()}


def _device(ctx, cases, polish="case", extra=0):
    """-> the device's outputs for the cases as one batch, as numpy (scale, R, T included)"""
    b = _batch(cases, extra)
    p = cases[0]["params"]
    pol = cases[0]["polish"] if polish == "case" else polish
    Bt, S = b["A"].shape[:2]
    d = _cuda(b)
    out = {k: torch.from_numpy(v).cuda() for k, v in _prefill(Bt, S, p["hypotheses"]).items()}
    o = ctx.sim3_ransac(d["A"], d["xa"], d["B"], d["xb"], d["n"], cases[0]["K"], d["seeds"], d["scale"], d["R"], d["T"], polish=pol, out=out,
                        want_counts=True, **p)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _item(got, i, S):
    """item i of a device batch in the layout sim3_cases.hold_exact reads"""
    m = int(got["n_inliers"][i])
    assert 0 <= m <= S
    assert not got["inlier"][i, S:].any() and (got["corr_index"][i, m:] == SENT["corr_index"]).all()
    return dict(counts=got["counts"][i], winner=int(got["winner"][i]), n_inliers=m, inlier=got["inlier"][i, :S], corr_index=got["corr_index"][i, :m],
                s_raw=float(got["scale"][i]), R_raw=got["R"][i], t_raw=got["T"][i], s=float(got["scale"][i]), R=got["R"][i], t=got["T"][i],
                stats=got["stats"][i])


def _hold(name, ctx, cases, sers, extra=0):
    """one batch twice: unpolished, bit for bit against the serial walk; polished (where the cases are), integers again and the
    model within TOL_POLISHED of the serial walk's and the reference's"""
    H = cases[0]["params"]["hypotheses"]
    raw = _device(ctx, cases, polish=None, extra=extra)
    for i, (c, ser) in enumerate(zip(cases, sers)):
        it = _item(raw, i, len(c["A"]))
        sc3.hold_exact((name, i, "raw"), it, dict(ser, found=ser["winner"] >= 0), H)
        assert np.isnan(it["stats"]).all(), name
    if cases[0]["polish"] is None:
        return raw
    pol = _device(ctx, cases, extra=extra)
    for i, (c, ser) in enumerate(zip(cases, sers)):
        it = _item(pol, i, len(c["A"]))
        for k in ("counts", "winner", "n_inliers", "inlier", "corr_index"):
            assert np.array_equal(it[k], _item(raw, i, len(c["A"]))[k]), (name, i, k)
        if ser["winner"] < 0:
            assert sc3.same_bits(it["s"], sc3.KEEP_S) and sc3.same_bits(it["R"], sc3.KEEP_R) and sc3.same_bits(it["t"], sc3.KEEP_T), name
            assert it["stats"][0] == 0 and np.isnan(it["stats"][1:]).all(), name
            continue
        assert sc3.model_distance(it, ser) <= TOL_POLISHED, (name, i, sc3.model_distance(it, ser))
        assert it["stats"][0] == ser["stats"][0] and np.array_equal(np.isnan(it["stats"]), np.isnan(ser["stats"])), name
    return pol


# n: below the minimum, at it, small, around the count's tile of 256, several tiles, and VSLAM_MAX_KP once; hypotheses: one, three
# and sixteen workgroups of 64 models
SHAPES = [(3, 64), (4, 64), (12, 192), (255, 64), (256, 192), (257, 1024), (1025, 192), (16384, 64)]


@pytest.mark.parametrize("n,hyp", SHAPES)
def test_every_integer_and_the_unpolished_model_equal_the_serial_walk(ctx, exe, tmp_path, n, hyp):
    sc = r3.planted(n, 0.5 if n >= 12 else 0.0, 2)
    min_in = 6 if n == 12 else 4 if n < 12 else 8
    c = sc3.case(sc, seed=11 + n, polish=dict(min_links=6), hypotheses=hyp, min_inliers=min_in)
    ser = sc3.run_serial(exe, tmp_path, [c])[0]
    ref = sc3.reference(c)
    sc3.hold_exact(("serial", n), ser, ref, hyp)
    got = _hold(f"n{n}h{hyp}", ctx, [c], [ser], extra=0 if n == 16384 else 37)   # stride > n: the padding is NaN
    assert (ser["winner"] >= 0) == (n >= 4)
    if n >= 12:
        it = _item(got, 0, n)
        assert np.array_equal(it["inlier"].astype(bool), sc["planted"])
        assert sc3.model_distance(it, ref) <= TOL_POLISHED and it["stats"][3] >= 1
        assert r3.model_error(it["s"], it["R"], it["t"], sc) <= r3.PLANTED_POLISH_BOUND


def test_n_is_clamped_to_the_stride(ctx, exe, tmp_path):
    sc = r3.planted(300, 0.5, 4)
    c = sc3.case(sc, seed=3)
    ser = sc3.run_serial(exe, tmp_path, [c])[0]
    over = dict(c, n=100000)
    got = _device(ctx, [over], polish=None)
    sc3.hold_exact("clamped", _item(got, 0, 300), dict(ser, found=True), c["params"]["hypotheses"])
    under = _device(ctx, [dict(c, n=-5)], polish=None)
    assert under["winner"][0] == -1 and (under["counts"][0] == -1).all() and not under["inlier"].any()


def test_hand_cases(ctx, exe, tmp_path):
    hc = sc3.hand_cases()
    sers = sc3.run_serial(exe, tmp_path, [c for c, _ in hc.values()])
    for (name, (c, found)), ser in zip(hc.items(), sers):
        got = _hold(name, ctx, [c], [ser], extra=5)
        assert (got["winner"][0] >= 0) == found, name
        if not found:   # left alone or not enough: the model outputs keep their bits
            assert sc3.same_bits(got["scale"][0], sc3.KEEP_S) and sc3.same_bits(got["R"][0], sc3.KEEP_R) and sc3.same_bits(got["T"][0], sc3.KEEP_T)


def test_a_batch_of_three_with_one_left_alone(ctx, exe, tmp_path):
    scs = [r3.planted(300, 0.5, 5), r3.planted(40, 0.5, 3), r3.planted(700, 0.6, 9)]
    cases = [sc3.case(s, seed=i + 1, polish={}) for i, s in enumerate(scs)]
    cases[1]["B"] = cases[1]["B"].copy()
    cases[1]["B"][4, 0] = np.nan                       # the middle item is left alone
    sers = sc3.run_serial(exe, tmp_path, cases)
    got = _hold("three", ctx, cases, sers)
    assert got["winner"][1] == -1 and (got["counts"][1] == -1).all() and got["n_inliers"][1] == 0
    for i in (0, 2):
        assert got["winner"][i] >= 0 and np.array_equal(got["inlier"][i, :len(scs[i]["A"])].astype(bool), scs[i]["planted"])


def test_bits_depend_on_the_item_alone(ctx):
    a, b, c3 = (sc3.case(r3.planted(n, 0.5, s), seed=s, polish={}) for n, s in ((500, 1), (90, 2), (260, 3)))
    one, again = _device(ctx, [a]), _device(ctx, [a])
    three = _device(ctx, [b, c3, a])                    # slot 2 of a batch of 3
    zero = _device(ctx, [a, b, c3])                     # slot 0
    mid = _device(ctx, [b, a, c3])                      # slot 1
    assert one["winner"][0] >= 0 and one["stats"][0, 3] >= 1
    m = int(one["n_inliers"][0])
    for k in one:
        assert np.array_equal(one[k].view(np.uint8), again[k].view(np.uint8)), k
        for other, slot in ((three, 2), (zero, 0), (mid, 1)):
            x, y = one[k][0], other[k][slot]
            if k == "inlier":
                x, y = x[:500], y[:500]
            elif k == "corr_index":
                x, y = x[:m], y[:m]
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (k, slot)


def test_the_refinement_alone_with_and_without_a_mask(ctx):
    """vslam_sim3_refine from a start 1 degree / 3 % / 0.05 off: within 16 x DELTA_REF of the reference; items it leaves alone keep
    their bits"""
    rows_, starts, masks, scenes = [], [], [], []
    for n, share, seed in r3.POLISH_CASES[::4]:
        sc, rows, start = r3.polish_case(n, share, seed)
        rows_.append((sc["A"], sc["xa"], sc["B"], sc["xb"]))
        starts.append(start); masks.append(sc["planted"].astype(np.int32)); scenes.append(sc)
    sc, rows, start = r3.polish_case(*r3.POLISH_CASES[0])
    rows_.append((sc["A"], sc["xa"], sc["B"], sc["xb"])); starts.append((-1.0, start[1], start[2])); masks.append(sc["planted"].astype(np.int32))
    Bt, S = len(rows_), max(len(r[0]) for r in rows_) + 3
    A, B = np.full((Bt, S, 3), np.nan), np.full((Bt, S, 3), np.nan)
    xa, xb = np.full((Bt, S, 2), np.nan, np.float32), np.full((Bt, S, 2), np.nan, np.float32)
    mask, n = np.ones((Bt, S), np.int32), np.zeros(Bt, np.int32)
    for i, (r, m) in enumerate(zip(rows_, masks)):
        k = len(r[0])
        A[i, :k], xa[i, :k], B[i, :k], xb[i, :k], mask[i, :k], n[i] = r[0], r[1], r[2], r[3], m, k
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    s_io, R_io, T_io = t(np.array([s[0] for s in starts])), t(np.stack([s[1] for s in starts])), t(np.stack([s[2] for s in starts]))
    _, _, _, stats = ctx.sim3_refine(t(A), t(xa), t(B), t(xb), t(n), scenes[0]["K"], s_io, R_io, T_io, mask=t(mask))
    ctx.synchronize()
    s_o, R_o, T_o = s_io.cpu().numpy(), R_io.cpu().numpy(), T_io.cpu().numpy()
    for i in range(Bt - 1):
        rs, rR, rt, rstats, info = r3.refine(*rows_[i], n[i], masks[i], scenes[i]["K"], *starts[i])
        got = dict(s=float(s_o[i]), R=R_o[i], t=T_o[i])
        assert info["moved"] and sc3.model_distance(got, dict(s=rs, R=rR, t=rt)) <= TOL_POLISHED, i
        assert r3.model_error(got["s"], got["R"], got["t"], scenes[i]) <= r3.POLISH_BOUND, i
    assert sc3.same_bits(s_o[-1], -1.0) and sc3.same_bits(R_o[-1], starts[-1][1]) and sc3.same_bits(T_o[-1], starts[-1][2])
    assert np.isnan(stats.cpu().numpy()[-1, 1:]).all()
    # without a mask: every row below n takes part
    sc, rows, start = r3.polish_case(*r3.POLISH_CASES[1])
    s1, R1, T1 = t(np.array([start[0]])), t(start[1][None]), t(start[2][None])
    ctx.sim3_refine(t(rows[0][None]), t(rows[1][None]), t(rows[2][None]), t(rows[3][None]), t(np.array([len(rows[0])], np.int32)), sc["K"], s1, R1, T1)
    ctx.synchronize()
    rs, rR, rt, _, info = r3.refine(*rows, len(rows[0]), None, sc["K"], *start)
    got = dict(s=float(s1.cpu().numpy()[0]), R=R1.cpu().numpy()[0], t=T1.cpu().numpy()[0])
    assert info["moved"] and sc3.model_distance(got, dict(s=rs, R=rR, t=rt)) <= TOL_POLISHED


# ------------------------------------------------------------------------------------------------ refusals, alignment, stream order
ARGS = ("A", "xa", "B", "xb", "n", "seeds", "scale", "R", "T", "inlier", "corr_index", "n_inliers", "winner", "counts", "stats")
OPTIONAL = ("corr_index", "counts", "stats")
ALIGN = dict(A=8, xa=8, B=8, xb=8, scale=8, R=8, T=8, stats=8, n=4, seeds=4, inlier=4, corr_index=4, n_inliers=4, winner=4, counts=4)


def _tensors(c):
    b = _batch([c])
    d = _cuda(b)
    d.update({k: torch.from_numpy(v).cuda() for k, v in _prefill(1, b["A"].shape[1], c["params"]["hypotheses"]).items()})
    return d


def _raw(ctx, d, c, over=None, params=None, polish=None, K=True, **sizes):
    ptr = {k: d[k].data_ptr() for k in ARGS}
    ptr.update(over or {})
    sz = dict(batch=1, stride=d["A"].shape[1])
    sz.update(sizes)
    Kh = np.ascontiguousarray(np.asarray(c["K"], np.float32).reshape(9))
    prm = capi.Sim3Params.make(ctx.lib, **c["params"]) if params is None else params
    v = lambda k: C.c_void_p(ptr[k])
    return ctx.lib.vslam_sim3_ransac(ctx.handle, v("A"), v("xa"), v("B"), v("xb"), v("n"), sz["batch"], sz["stride"],
                                     Kh.ctypes.data_as(C.c_void_p) if K else C.c_void_p(0), v("seeds"), C.byref(prm),
                                     C.byref(polish) if polish is not None else C.c_void_p(0), v("scale"), v("R"), v("T"), v("inlier"),
                                     v("corr_index"), v("n_inliers"), v("winner"), v("counts"), v("stats"))


def test_invalid_arguments_are_refused_before_anything_is_queued(ctx, exe, tmp_path):
    c = sc3.case(r3.planted(300, 0.5, 5), seed=1)
    d = _tensors(c)
    before = {k: v.cpu().numpy().copy() for k, v in d.items()}
    for bad in (dict(hypotheses=0), dict(hypotheses=32), dict(hypotheses=100), dict(hypotheses=1088), dict(min_inliers=3), dict(inlier_px=0.0),
                dict(inlier_px=-1.0), dict(inlier_px=float("nan")), dict(inlier_px=float("inf"))):
        assert _raw(ctx, d, c, params=capi.Sim3Params.make(ctx.lib, **bad)) == -1, bad
    for bad in (dict(max_iterations=0), dict(rounds=5), dict(min_links=5), dict(huber_px=0.0), dict(gate_px=float("nan"))):
        assert _raw(ctx, d, c, polish=capi.ResectParams.make(ctx.lib, **bad)) == -1, bad
    for k in ARGS:
        if k not in OPTIONAL:
            assert _raw(ctx, d, c, over={k: 0}) == -1, k
    assert _raw(ctx, d, c, K=False) == -1
    for kw in (dict(batch=0), dict(batch=-1), dict(stride=0), dict(stride=-5)):
        assert _raw(ctx, d, c, **kw) == -1, kw
    assert _raw(ctx, d, c, stride=16385) == -4
    for k, need in ALIGN.items():                       # one pointer at a time, one byte off and half its requirement off
        for off in (1, need // 2):
            assert _raw(ctx, d, c, over={k: d[k].data_ptr() + off}) == -1, (k, off)
            assert "d_" in ctx.lib.vslam_last_error(ctx.handle).decode()
    assert ctx.lib.vslam_sim3_ransac(C.c_void_p(0), *[C.c_void_p(0)] * 5, 1, 300, *[C.c_void_p(0)] * 13) == -1
    # the refinement's own refusals
    ref_args = lambda **o: [C.c_void_p(o.get(k, d[k].data_ptr())) for k in ("A", "xa", "B", "xb", "n")]
    Kh = np.ascontiguousarray(np.asarray(c["K"], np.float32).reshape(9))
    tail = lambda **o: [C.c_void_p(o.get(k, d[k].data_ptr())) for k in ("scale", "R", "T", "stats")]
    call = lambda batch=1, stride=300, mask=0, prm=None, **o: ctx.lib.vslam_sim3_refine(
        ctx.handle, *ref_args(**o), batch, stride, C.c_void_p(mask), Kh.ctypes.data_as(C.c_void_p), C.byref(prm) if prm is not None else C.c_void_p(0),
        *tail(**o))
    for k in ("A", "xa", "B", "xb", "n", "scale", "R", "T"):
        assert call(**{k: 0}) == -1, k
        assert call(**{k: d[k].data_ptr() + 1}) == -1, k
    assert call(batch=0) == -1 and call(stride=0) == -1 and call(stride=16385) == -4
    assert call(mask=d["inlier"].data_ptr() + 2) == -1 and call(stats=d["stats"].data_ptr() + 4) == -1
    assert call(prm=capi.ResectParams.make(ctx.lib, min_links=5)) == -1
    ctx.synchronize()
    for k, v in d.items():
        assert np.array_equal(v.cpu().numpy().view(np.uint8), before[k].view(np.uint8)), (k, "nothing ran")
    assert _raw(ctx, d, c) == 0                          # and the next call is exact
    ctx.synchronize()
    ser = sc3.run_serial(exe, tmp_path, [c])[0]
    got = {k: v.cpu().numpy() for k, v in d.items()}
    sc3.hold_exact("after the refusals", _item(got, 0, 300), dict(ser, found=True), c["params"]["hypotheses"])
    d2 = _tensors(c)                                     # the optional ones may be NULL
    assert _raw(ctx, d2, c, over=dict(corr_index=0, counts=0, stats=0)) == 0
    ctx.synchronize()
    for k in ("scale", "R", "T", "inlier", "n_inliers", "winner"):
        assert np.array_equal(d2[k].cpu().numpy().view(np.uint8), d[k].cpu().numpy().view(np.uint8)), k
    for k in OPTIONAL:
        assert np.array_equal(d2[k].cpu().numpy().view(np.uint8), before[k].view(np.uint8)), k


def test_every_pointer_exactly_at_its_alignment_gives_the_aligned_bits(ctx):
    from offset_views import offset_view
    c = sc3.case(r3.planted(300, 0.5, 5), seed=1, polish={})
    pol = capi.ResectParams.make(ctx.lib)
    base = _tensors(c)
    assert _raw(ctx, base, c, polish=pol) == 0
    ctx.synchronize()
    want = {k: v.cpu().numpy() for k, v in base.items()}
    assert want["winner"][0] >= 0
    for nm, need in ALIGN.items():
        d = _tensors(c)
        v, whole, check = offset_view(tuple(d[nm].shape), d[nm].dtype, need // d[nm].element_size())
        assert v.data_ptr() % need == 0 and v.data_ptr() % (2 * need) != 0, nm
        v.copy_(d[nm])
        d[nm] = v
        assert _raw(ctx, d, c, polish=pol) == 0, nm
        ctx.synchronize()
        check(nm)
        for k in d:
            assert np.array_equal(d[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)), (nm, k)


def _calls(ctx, seed, polish=True):
    import sim3_calls as s3c
    structs = (capi.Sim3Params.make(ctx.lib), capi.ResectParams.make(ctx.lib) if polish else None)
    c = sc3.case(r3.planted(300, 0.5, seed), seed=seed)
    d = _tensors(c)
    sc, rows, start = r3.polish_case(257, 0.5, seed)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    rd = dict(A=t(sc["A"][None]), xa=t(sc["xa"][None]), B=t(sc["B"][None]), xb=t(sc["xb"][None]), n=t(np.array([257], np.int32)),
              mask=t(sc["planted"].astype(np.int32)[None]), scale=t(np.array([start[0]])), R=t(start[1][None]), T=t(start[2][None]))
    return {"vslam_sim3_ransac": s3c.ransac(d, c["K"], *structs), "vslam_sim3_refine": s3c.refine(rd, sc["K"], structs[1])}, structs


def test_outputs_depend_on_the_arguments_not_on_the_workspace(ctx):
    import entry_calls as ec
    import sim3_calls as s3c
    calls, keep = _calls(ctx, 5)
    assert sorted(calls) == sorted(s3c.ENTRIES)
    first = {}
    for name, call in calls.items():
        rc, msg, first[name], _ = ec.run(ctx, call)
        assert rc == 0, (name, msg)
    assert np.frombuffer(first["vslam_sim3_ransac"]["d_n_inliers"].tobytes(), np.int32)[0] == 150
    assert {"sim3_models", "sim3_index"} <= set(ctx.workspace_slots())
    for fill in (0x00, 0x5A, 0xFF):
        for name, call in calls.items():
            ctx.workspace_fill(fill)
            rc, msg, got, _ = ec.run(ctx, call)
            assert rc == 0 and not ec._same(first[name], got), (name, fill, ec._same(first[name], got))
    # behind a call of itself at another shape and with other contents
    other = sc3.case(r3.planted(700, 0.6, 9), seed=4, hypotheses=256)
    for name, call in calls.items():
        _device(ctx, [other], polish={})
        rc, msg, got, _ = ec.run(ctx, call)
        assert rc == 0 and not ec._same(first[name], got), (name, ec._same(first[name], got))


@pytest.mark.parametrize("entry", ["vslam_sim3_ransac", "vslam_sim3_refine"])
def test_stream_order_behind_a_stalled_stream(ctx, entry):
    """On the session's context and the stream it is bound to (torch's default stream), as tests/test_gpu_pnp.py does and for its
    reason: the test makes no stream and no context of its own."""
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    stream = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == stream
    (calls, keep), (others, keep2) = _calls(ctx, 5), _calls(ctx, 6)
    call, other = calls[entry], others[entry]
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


# ------------------------------------------------------------------------------------------------ the world on exact scenes
import pnp_cases as pc

W_KP, W_FRAMES = 64, 6
W_MCAP, W_OCAP = W_FRAMES * W_KP, 4 * W_FRAMES * W_KP
W_PAIRS = ((0, 3, 1, 5), (0, 5, 1, 2), (0, 2, 0, 4), (1, 1, 1, 5), (0, 4, 7, 1), (0, 9, 1, 1))   # the last two: no such track, no such frame


def _put(ctx, ptr, a):
    a = np.ascontiguousarray(a)
    ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, C.c_void_p(ptr), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)))


@pytest.fixture
def two_tracks(ctx):
    """pnp_cases.world_scene of 60 points and 7 frames fed to two tracks of ONE map and world through vslam_map_step: track 0 sees
    scene frames 0 .. 5, track 1 scene frames 1 .. 6, so its world has another origin, orientation and unit.  -> dict(map, world,
    ws, shift (scene frame of each track's frame 0), xy (tracks, frames, kp, 2) on the device)"""
    seed, ws = pc.first_world_scene(60, frames=W_FRAMES + 1)
    shift = (0, 1)
    a = capi.PointMap(ctx, 2, W_FRAMES, W_KP, W_MCAP, W_OCAP)
    wa = a.attach_world()
    bgr = torch.full((2, pc.SCENE_H, pc.SCENE_W, 3), 90, dtype=torch.uint8).cuda()
    n = ws["n"]
    xy_all = np.zeros((2, W_FRAMES, W_KP, 2), np.float32)

    def frame(f):
        xy, desc = np.zeros((2, W_KP, 2), np.float32), np.zeros((2, W_KP, 32), np.uint8)
        for t in range(2):
            xy[t, :n], desc[t, :n] = ws["xy"][f + shift[t]], ws["desc"][f + shift[t]]
        xy_all[:, f] = xy
        d = dict(xy=torch.from_numpy(xy).cuda(), desc=torch.from_numpy(desc).cuda(), n=torch.full((2,), n, dtype=torch.int32).cuda())
        d["nodes"] = ctx.kdtree_build(d["xy"], d["n"])
        return d
    last = frame(0)
    for f in range(1, W_FRAMES):
        cur = frame(f)
        matches, best, F = np.zeros((2, W_KP, 2), np.int32), np.zeros((2, 4), np.int32), np.zeros((2, 9), np.float32)
        for t in range(2):
            p = ws["pairs"][f - 1 + shift[t]]
            m = p["matches"]
            matches[t, :len(m)], best[t], F[t] = m, (0, len(m), 0, len(m)), p["F"]
        a.step(last, cur, dict(matches=torch.from_numpy(matches).cuda(), best=torch.from_numpy(best).cuda(), F=torch.from_numpy(F).cuda()), bgr,
               pc.SCENE_K)
        last = cur
    ctx.synchronize()
    yield dict(map=a, world=wa, ws=ws, shift=shift, xy=torch.from_numpy(xy_all).cuda(), n=n)
    a.close(); wa.close()


def _items(tt, pairs=W_PAIRS):
    """the arrays of one vslam_world_sim3 call: every scene point matched, in the order of the scene's points"""
    ws, n = tt["ws"], tt["n"]
    I = len(pairs)
    matches, nm = np.full((I, W_KP, 2), -3, np.int32), np.zeros(I, np.int32)
    xy_a, xy_b = np.full((I, W_KP, 2), np.nan, np.float32), np.full((I, W_KP, 2), np.nan, np.float32)
    for i, (ta, fa, tb, fb) in enumerate(pairs):
        Fa = min(fa + tt["shift"][min(ta, 1)], W_FRAMES)
        Fb = min(fb + tt["shift"][min(tb, 1)], W_FRAMES)
        matches[i, :n], nm[i] = np.stack([ws["perm"][Fa], ws["perm"][Fb]], 1), n
        xy_a[i, :n], xy_b[i, :n] = ws["xy"][Fa], ws["xy"][Fb]
    return dict(pairs=np.array(pairs, np.int32), matches=matches, n_matches=nm, xy_a=xy_a, xy_b=xy_b)


def _world_sim3(tt, it, polish, **params):
    d = {k: torch.from_numpy(v).cuda() for k, v in it.items()}
    o = tt["world"].sim3(tt["map"], d["pairs"], d["matches"], d["n_matches"], d["xy_a"], d["xy_b"], pc.SCENE_K, polish=polish, **params)
    tt["world"].ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _reference_item(view, it, i, polish, **params):
    ta, fa, tb, fb = (int(v) for v in it["pairs"][i])
    T, Fr = view["world_Twc"].shape[:2]
    if not (0 <= ta < T and 0 <= tb < T and 0 <= fa < view["frames"] and 0 <= fb < view["frames"]):
        return None
    fuse = view.get("world_fuse_to")
    side = lambda t, f: dict(ids=view["map_point_ids"][t, f], points=view["world_points"][t], Twc=view["world_Twc"][t, f],
                             fuse_to=None if fuse is None else fuse[t])
    return r3.world_sim3(side(ta, fa), side(tb, fb), it["matches"][i], it["n_matches"][i], it["xy_a"][i], it["xy_b"][i], W_KP, pc.SCENE_K,
                         i + 1, polish=polish, **params)


def _hold_world(view, it, got, polish, **params):
    """integers bit for bit; the unpolished similarity bit for bit, the polished one within TOL_POLISHED relative to its size"""
    found = 0
    for i in range(len(it["pairs"])):
        ref = _reference_item(view, it, i, polish, **params)
        if ref is None:
            assert got["found"][i] == 0 and got["n_corr"][i] == 0 and got["winner"][i] == -1 and got["n_inliers"][i] == 0, i
            assert (got["point_a"][i] == -1).all() and not got["R_w"][i].any()
            continue
        m = ref["n_corr"]
        assert got["n_corr"][i] == m and got["found"][i] == int(ref["found"]) and got["winner"][i] == ref["winner"], (i, got["n_corr"][i], m)
        assert got["n_inliers"][i] == ref["n_inliers"], i
        assert np.array_equal(got["point_a"][i, :m], ref["point_a"]) and np.array_equal(got["point_b"][i, :m], ref["point_b"]), i
        assert (got["point_a"][i, m:] == -1).all() and (got["point_b"][i, m:] == -1).all(), i
        if not ref["found"]:
            assert not got["R"][i].any() and not got["R_w"][i].any() and got["s_w"][i] == 0, i
            continue
        found += 1
        pairs = (("scale", "s"), ("R", "R"), ("T", "t"), ("s_w", "s_w"), ("R_w", "R_w"), ("t_w", "t_w"))
        for kd, kr in pairs:
            if polish is None:
                assert sc3.same_bits(got[kd][i], ref[kr]), (i, kd)
            else:
                size = max(1.0, float(np.abs(np.asarray(ref[kr])).max()))
                assert np.abs(got[kd][i] - ref[kr]).max() <= 1e-9 * size, (i, kd, np.abs(got[kd][i] - ref[kr]).max())
    return found


def test_world_sim3_gathers_what_the_reference_gathers_and_writes_nothing_else(ctx, two_tracks):
    """On this map none of these pairs is FOUND, by the reference as by the device (the map sets map_point_ids by association
    alone -- include/vslam_fuse.h, "Why" -- and what the gather is left with is printed), so this holds what can be held here: the gathered
    ids, counts and winner equal tests/ref_sim3.py bit for bit for every item, the two items without such a track or frame gather nothing,
    and neither the world nor the map changes a bit.  The found path, vslam_world_apply_sim3 and the fusion are held further down, on
    this map with the ids and the world of two reference tracks written into it."""
    tt = two_tracks
    a, wa = tt["map"], tt["world"]
    before = a.view()
    assert before["frames"] == W_FRAMES and (before["world_links"][:, 2:] >= 8).all(), before["world_links"].tolist()
    it = _items(tt)
    raw = _world_sim3(tt, it, None)
    _hold_world(before, it, raw, None)
    have = (before["map_point_ids"][:, :, :tt["n"]] >= 0).sum(2)
    print("keypoints with a map point, per track and frame:", have.tolist(), "of", tt["n"], "; map points", before["sizes"].tolist())
    print("gathered", raw["n_corr"].tolist(), "found", raw["found"].tolist())
    # the evidence for include/vslam_sim3.h's note on the ids: frames 0 and 1 of a track have none, and what two frames share is
    # below min_inliers
    assert (have[:, :2] == 0).all() and (raw["n_corr"] < 8).all() and not raw["found"].any()
    after = a.view()
    for k in before:   # it writes nothing into the world or the map
        if isinstance(before[k], np.ndarray):
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ the world with planted ids
# vslam_map_step sets map_point_ids by association alone (see the test above), so the found path is reached on a map whose ids, sizes
# and world are WRITTEN: the two tracks of sim3_cases.ref_tracks (ref_world.World over one scene from different first frames), which
# is the CPU test's own data.  The map and world are real (two tracks stepped to six frames, so `frames` is 6); only their arrays
# are replaced.
P_PAIRS = ((0, 3, 1, 5), (0, 5, 1, 2), (0, 2, 0, 4), (1, 1, 1, 5), (0, 4, 7, 1), (0, 9, 1, 1))


def _fuse_ptr(wa):
    p, st = C.c_void_p(), C.c_int32()
    wa.ctx._check(wa.lib.vslam_world_fusion_view(wa.handle, C.byref(p), C.byref(st)))
    return p.value, st.value


def _plant(ctx, tt, rt, fuse_to=None):
    a, wa = tt["map"], tt["world"]
    ma, wo = a.arrays(), wa.arrays()
    n = rt["n"]
    ids = np.full((2, W_FRAMES, W_KP), -1, np.int32)
    pts = np.zeros((2, W_MCAP, 4), np.float32)
    Twc, pose = np.zeros((2, W_FRAMES, 16)), np.zeros((2, W_FRAMES, 16), np.float32)
    scale, carry, cidx = np.zeros((2, W_FRAMES)), np.zeros((2, W_KP, 3)), np.full((2, W_KP), -1, np.int32)
    sizes = np.zeros(2, np.int32)
    for t, tr in enumerate(rt["tracks"]):
        ids[t, :, :n], sizes[t] = tr["ids"], tr["size"]
        pts[t, :tr["size"]] = tr["points"]
        Twc[t], pose[t], scale[t] = tr["Twc"], tr["pose"], tr["scale"]
        carry[t, :n], cidx[t, :n] = tr["carry"], tr["carry_index"]
    for ptr, v in ((ma.d_map_point_ids, ids), (ma.d_sizes, sizes), (wo.d_world_points, pts), (wo.d_Twc, Twc), (wo.d_pose, pose),
                   (wo.d_scale, scale), (wo.d_carry, carry), (wo.d_carry_index, cidx)):
        _put(ctx, ptr, v)
    if fuse_to is not None:
        p, st = _fuse_ptr(wa)
        assert p and (st & 1)
        _put(ctx, p, fuse_to)
    ctx.synchronize()


def _planted_items(rt, pairs=P_PAIRS):
    n = rt["n"]
    I = len(pairs)
    matches, nm = np.full((I, W_KP, 2), -3, np.int32), np.zeros(I, np.int32)
    xy_a, xy_b = np.full((I, W_KP, 2), np.nan, np.float32), np.full((I, W_KP, 2), np.nan, np.float32)
    last = len(rt["xy"]) - 1
    for i, (ta, fa, tb, fb) in enumerate(pairs):
        Fa = min(fa + rt["tracks"][min(ta, 1)]["first"], last)
        Fb = min(fb + rt["tracks"][min(tb, 1)]["first"], last)
        matches[i, :n], nm[i] = np.stack([rt["perm"][Fa], rt["perm"][Fb]], 1), n
        xy_a[i, :n], xy_b[i, :n] = rt["xy"][Fa], rt["xy"][Fb]
    return dict(pairs=np.array(pairs, np.int32), matches=matches, n_matches=nm, xy_a=xy_a, xy_b=xy_b)


def _psim3(tt, it, polish, **params):
    d = {k: torch.from_numpy(v).cuda() for k, v in it.items()}
    o = tt["world"].sim3(tt["map"], d["pairs"], d["matches"], d["n_matches"], d["xy_a"], d["xy_b"], rr.kmat(), polish=polish, **params)
    tt["world"].ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _pref(view, it, i, polish):
    ta, fa, tb, fb = (int(v) for v in it["pairs"][i])
    if not (0 <= ta < 2 and 0 <= tb < 2 and 0 <= fa < view["frames"] and 0 <= fb < view["frames"]):
        return None
    fuse = view.get("world_fuse_to")
    side = lambda t, f: dict(ids=view["map_point_ids"][t, f], points=view["world_points"][t], Twc=view["world_Twc"][t, f],
                             fuse_to=None if fuse is None else fuse[t])
    return r3.world_sim3(side(ta, fa), side(tb, fb), it["matches"][i], it["n_matches"][i], it["xy_a"][i], it["xy_b"][i], W_KP, rr.kmat(), i + 1,
                         polish=polish)


def _phold(view, it, got, polish):
    """-> (items found, pairs gathered): integers bit for bit; the unpolished similarities bit for bit, polished ones to 1e-9"""
    found = gathered = 0
    for i in range(len(it["pairs"])):
        ref = _pref(view, it, i, polish)
        if ref is None:
            assert got["found"][i] == 0 and got["n_corr"][i] == 0 and got["winner"][i] == -1 and got["n_inliers"][i] == 0, i
            continue
        m = ref["n_corr"]
        gathered += m
        assert got["n_corr"][i] == m and got["found"][i] == int(ref["found"]) and got["winner"][i] == ref["winner"], (i, got["n_corr"][i], m)
        assert got["n_inliers"][i] == ref["n_inliers"], i
        assert np.array_equal(got["point_a"][i, :m], ref["point_a"]) and np.array_equal(got["point_b"][i, :m], ref["point_b"]), i
        assert (got["point_a"][i, m:] == -1).all() and (got["point_b"][i, m:] == -1).all(), i
        if not ref["found"]:
            assert not got["R"][i].any() and not got["R_w"][i].any() and got["s_w"][i] == 0, i
            continue
        found += 1
        for kd, kr in (("scale", "s"), ("R", "R"), ("T", "t"), ("s_w", "s_w"), ("R_w", "R_w"), ("t_w", "t_w")):
            if polish is None:
                assert sc3.same_bits(got[kd][i], ref[kr]), (i, kd)
            else:
                size = max(1.0, float(np.abs(np.asarray(ref[kr])).max()))
                assert np.abs(got[kd][i] - ref[kr]).max() <= 1e-9 * size, (i, kd)
    return found, gathered


def _land(view, rt, got, i):
    """item i = (0, fa, 1, fb): the largest distance, in scene units, between a point of track 1 carried into track 0's world and the
    same physical point as track 0 holds it; the CPU test's bound: 4 x the larger of the tracks' own errors (ref_world.run_scene)"""
    a, b = rt["tracks"]
    Xa, Xb = (view["world_points"][t, :, :3].astype(np.float64) for t in (0, 1))
    mapped = got["s_w"][i] * (Xb @ got["R_w"][i].reshape(3, 3).T) + got["t_w"][i]
    worst = 0.0
    for r, tid in enumerate(b["truth"]):
        for j in np.flatnonzero(a["truth"] == tid):
            worst = max(worst, float(np.abs(mapped[r] - Xa[j]).max()) * a["g"])
    return worst, 4.0 * max(a["err"], b["err"])


def test_world_sim3_found_apply_sim3_and_the_identity_afterwards(ctx, two_tracks):
    tt = two_tracks
    a, wa = tt["map"], tt["world"]
    rt = sc3.ref_tracks(2)
    _plant(ctx, tt, rt)
    before = a.view()
    it = _planted_items(rt)
    raw = _psim3(tt, it, None)
    found, gathered = _phold(before, it, raw, None)
    assert found == 4 and gathered == 155 and raw["found"].tolist() == [1, 1, 1, 1, 0, 0], (found, gathered, raw["found"].tolist())
    pol = _psim3(tt, it, dict(min_links=8))
    assert _phold(before, it, pol, dict(min_links=8))[0] == 4
    for k in ("found", "n_corr", "n_inliers", "winner", "point_a", "point_b"):
        assert np.array_equal(raw[k], pol[k]), k
    after = a.view()
    for k in before:   # it writes nothing into the world or the map
        if isinstance(before[k], np.ndarray):
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    for i in (0, 1):
        for name, got in (("unpolished", raw), ("polished", pol)):
            worst, bound = _land(before, rt, got, i)
            print(f"item {i} {name}: {got['n_corr'][i]} pairs, {got['n_inliers'][i]} inliers, track 1 lands on track 0 within {worst:.2e} (bound {bound:.2e})")
            assert worst <= bound, (i, name, worst, bound)
    # ---- apply: track 1 into track 0's world; track 0 listed with apply == 0
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dt)).cuda()
    s2 = np.array([raw["s_w"][0], 3.0]); R2 = np.stack([raw["R_w"][0], np.eye(3).reshape(9)]); t2 = np.stack([raw["t_w"][0], np.ones(3)])
    wa.apply_sim3(a, [1, 0], dev(s2, np.float64), dev(R2, np.float64), dev(t2, np.float64), apply=dev([1, 0], np.int32))
    ctx.synchronize()
    moved = a.view()
    track = dict(Twc=before["world_Twc"][1], pose=before["world_pose"][1], scale=before["world_scale"][1], carry=before["world_carry"][1],
                 carry_index=before["world_carry_index"][1], points=before["world_points"][1], size=int(before["sizes"][1]))
    want = r3.apply_sim3(track, float(s2[0]), R2[0], t2[0])
    written = (("world_Twc", "Twc"), ("world_pose", "pose"), ("world_scale", "scale"), ("world_carry", "carry"), ("world_points", "points"))
    for kd, kr in written:
        assert np.array_equal(np.ascontiguousarray(moved[kd][1]).view(np.uint8), np.ascontiguousarray(want[kr]).view(np.uint8)), kd
        assert np.array_equal(moved[kd][0].view(np.uint8), before[kd][0].view(np.uint8)), (kd, "track 0: apply == 0")
        assert not np.array_equal(moved[kd][1].view(np.uint8), before[kd][1].view(np.uint8)), kd
    for k in before:
        if isinstance(before[k], np.ndarray) and k not in [w[0] for w in written]:
            assert np.array_equal(before[k].view(np.uint8), moved[k].view(np.uint8)), (k, "not the call's to write")
    # the same query is now the identity within the same bound
    again = _psim3(tt, it, None)
    assert _phold(moved, it, again, None)[0] == 4
    far = float(np.abs(rt["scene"]["points"]).max())
    g = rt["tracks"][0]["g"]
    bound = _land(before, rt, raw, 0)[1]
    off = max(abs(again["s_w"][0] - 1.0) * far, float(np.abs(again["R_w"][0] - np.eye(3).reshape(9)).max()) * far,
              float(np.abs(again["t_w"][0]).max()) * g)
    print(f"after apply_sim3 the query is {off:.2e} from the identity (bound {bound:.2e})")
    assert off <= bound
    wa.reset()   # reset undoes it
    ctx.synchronize()
    z = wa.view()
    assert np.array_equal(z["Twc"][1, 0], np.eye(4).reshape(16)) and (z["scale"] == 1.0).all()


def test_world_sim3_follows_the_fusion_an_absorbed_and_a_culled_point(ctx, two_tracks):
    tt = two_tracks
    a, wa = tt["map"], tt["world"]
    rt = sc3.ref_tracks(2)
    wa.fuse(a)                       # makes d_fuse_to and the state "a fusion exists"; its contents are then written
    _plant(ctx, tt, rt, fuse_to=np.tile(np.arange(W_MCAP, dtype=np.int32), (2, 1)))
    it = _planted_items(rt, P_PAIRS[:2])
    plain = _psim3(tt, it, None)
    assert _phold(a.view(), it, plain, None)[0] == 2
    # absorbed: a row of track 0 that item 0 gathers now stands behind another row of the SAME physical point; culled: another is -1
    tr = rt["tracks"][0]
    ga = plain["point_a"][0, :plain["n_corr"][0]]
    absorbed = next(int(r) for r in ga if (np.flatnonzero(tr["truth"] == tr["truth"][r]) != r).any())
    survivor = int(next(j for j in np.flatnonzero(tr["truth"] == tr["truth"][absorbed]) if j != absorbed))
    culled = int(next(r for r in ga if r not in (absorbed, survivor)))
    ft = np.tile(np.arange(W_MCAP, dtype=np.int32), (2, 1))
    ft[0, absorbed], ft[0, culled] = survivor, -1
    _plant(ctx, tt, rt, fuse_to=ft)
    view = a.view()
    assert np.array_equal(view["world_fuse_to"], ft)
    fused = _psim3(tt, it, None)
    assert _phold(view, it, fused, None)[0] == 2
    m = fused["n_corr"][0]
    assert m == plain["n_corr"][0] - 1, "the culled point's match is not taken"
    ids = fused["point_a"][0, :m].tolist()
    assert absorbed not in ids and culled not in ids and survivor in ids


def test_world_calls_refuse_what_the_header_says(ctx, two_tracks):
    tt = two_tracks
    a, wa = tt["map"], tt["world"]
    rt = sc3.ref_tracks(2)
    _plant(ctx, tt, rt)
    it = _planted_items(rt, P_PAIRS[:2])
    d = {k: torch.from_numpy(v).cuda() for k, v in it.items()}
    cols = [d["pairs"][:, k].contiguous() for k in range(4)]
    I = 2
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    o = dict(scale=torch.full((I,), 7.5, **f64), R=torch.full((I, 9), 7.5, **f64), T=torch.full((I, 3), 7.5, **f64), s_w=torch.full((I,), 7.5, **f64),
             R_w=torch.full((I, 9), 7.5, **f64), t_w=torch.full((I, 3), 7.5, **f64), found=torch.full((I,), 77, **i32), n_corr=torch.full((I,), 77, **i32),
             n_inliers=torch.full((I,), 77, **i32), winner=torch.full((I,), 77, **i32), stats=torch.full((I, 4), 7.5, **f64))
    seeds = torch.arange(1, I + 1, **i32)
    Kh = np.ascontiguousarray(rr.kmat().reshape(9))
    names = ("track_a", "frame_a", "track_b", "frame_b", "matches", "n_matches", "xy_a", "xy_b", "seeds", "scale", "R", "T", "s_w", "R_w", "t_w",
             "found", "n_corr", "n_inliers", "winner", "stats")
    ptr = dict(zip(names[:4], (c.data_ptr() for c in cols)))
    ptr.update(matches=d["matches"].data_ptr(), n_matches=d["n_matches"].data_ptr(), xy_a=d["xy_a"].data_ptr(), xy_b=d["xy_b"].data_ptr(),
               seeds=seeds.data_ptr(), **{k: v.data_ptr() for k, v in o.items()})

    def call(world=wa.handle, pmap=a.handle, items=I, K=True, prm=None, pol=None, **over):
        p = dict(ptr, **over)
        v = lambda k: C.c_void_p(p[k])
        return ctx.lib.vslam_world_sim3(ctx.handle, world, pmap, v("track_a"), v("frame_a"), v("track_b"), v("frame_b"), items, v("matches"),
                                        v("n_matches"), v("xy_a"), v("xy_b"), Kh.ctypes.data_as(C.c_void_p) if K else C.c_void_p(0), v("seeds"),
                                        C.byref(prm) if prm is not None else C.c_void_p(0), C.byref(pol) if pol is not None else C.c_void_p(0),
                                        v("scale"), v("R"), v("T"), v("s_w"), v("R_w"), v("t_w"), v("found"), v("n_corr"), v("n_inliers"), v("winner"),
                                        C.c_void_p(0), C.c_void_p(0), v("stats"))
    align = dict(matches=8, xy_a=8, xy_b=8, scale=8, R=8, T=8, s_w=8, R_w=8, t_w=8, stats=8, track_a=4, frame_a=4, track_b=4, frame_b=4, n_matches=4,
                 seeds=4, found=4, n_corr=4, n_inliers=4, winner=4)
    for k in names:
        if k != "stats":
            assert call(**{k: 0}) == -1, k
        for off in (1, align[k] // 2):
            assert call(**{k: ptr[k] + off}) == -1, (k, off)
    assert call(items=0) == -1 and call(items=-2) == -1 and call(K=False) == -1
    assert call(world=C.c_void_p(0)) == -1 and call(pmap=C.c_void_p(0)) == -1
    assert call(prm=capi.Sim3Params.make(ctx.lib, hypotheses=100)) == -1 and call(pol=capi.ResectParams.make(ctx.lib, min_links=5)) == -1
    other = capi.World(ctx, 2, W_FRAMES, W_KP)
    other_map = capi.PointMap(ctx, 2, W_FRAMES, W_KP, W_MCAP, W_OCAP)
    short = other_map.attach_world()       # a world that is attached, but to another map
    try:
        assert call(world=other.handle) == -1, "a world that is not the one attached to that map"
        assert call(world=short.handle) == -1, "a world attached to another map"
        s, R, t = torch.ones(2, **f64), torch.eye(3, **f64).reshape(1, 9).repeat(2, 1).contiguous(), torch.ones((2, 3), **f64)
        ap = torch.ones(2, **i32)
        before = a.view()

        def apply(tracks, world=wa.handle, items=None, **over):
            h = np.ascontiguousarray(np.asarray(tracks, np.int32))
            p = dict(s=s.data_ptr(), R=R.data_ptr(), t=t.data_ptr(), apply=ap.data_ptr(), h=h.ctypes.data)
            p.update(over)
            return ctx.lib.vslam_world_apply_sim3(ctx.handle, world, a.handle, C.c_void_p(p["h"]), C.c_void_p(p["s"]), C.c_void_p(p["R"]),
                                                  C.c_void_p(p["t"]), C.c_void_p(p["apply"]), len(h) if items is None else items)
        assert apply([0, 0]) == -1, "a track listed twice"
        assert apply([1, 1]) == -1 and apply([0, 2]) == -1 and apply([-1]) == -1 and apply([0, 1], items=0) == -1 and apply([0, 1, 0], items=3) == -1
        assert apply([0], world=other.handle) == -1 and apply([0], world=C.c_void_p(0)) == -1
        for k in ("h", "s", "R", "t", "apply"):
            assert apply([0, 1], **{k: 0}) == -1, k
        for k, need in (("s", 8), ("R", 8), ("t", 8), ("apply", 4)):
            assert apply([0, 1], **{k: dict(s=s, R=R, t=t, apply=ap)[k].data_ptr() + need // 2}) == -1, k
        ctx.synchronize()
        after = a.view()
        for k in before:
            if isinstance(before[k], np.ndarray):
                assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), (k, "nothing ran")
        for k, v in o.items():
            assert (v.cpu().numpy() == (77 if v.dtype == torch.int32 else 7.5)).all(), (k, "nothing ran")
        assert call() == 0 and apply([1]) == 0    # and the next calls are taken
        ctx.synchronize()
        assert (o["found"].cpu().numpy() == 1).all()
        assert not np.array_equal(a.view()["world_Twc"][1], before["world_Twc"][1])
    finally:
        other_map.close(); short.close(); other.close()


def _world_calls(ctx, tt, rt, variant):
    """the Calls of the two world entry points on the planted world, at one of two contents"""
    import sim3_calls as s3c
    a, wa = tt["map"], tt["world"]
    pairs = (P_PAIRS[:4], ((0, 4, 1, 2), (1, 5, 0, 1), (1, 2, 1, 4), (0, 1, 0, 5)))[variant]
    it = _planted_items(rt, pairs)
    d = {k: torch.from_numpy(v).cuda() for k, v in it.items() if k != "pairs"}
    for j, k in enumerate(("track_a", "frame_a", "track_b", "frame_b")):
        d[k] = torch.from_numpy(np.ascontiguousarray(it["pairs"][:, j])).cuda()
    d["seeds"] = torch.arange(1 + variant, 5 + variant, dtype=torch.int32).cuda()
    rng = np.random.default_rng(40 + variant)
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dt)).cuda()
    Rm = [r3._rodrigues(rng.normal(size=3) * 0.2).reshape(9) for _ in range(2)]
    ad = dict(s=t(rng.uniform(0.5, 2.0, 2), np.float64), R=t(np.stack(Rm), np.float64), t=t(rng.normal(size=(2, 3)), np.float64),
              apply=t([1, 1], np.int32))

    def state():
        v = wa.view()
        return {k: v[k] for k in ("Twc", "pose", "scale", "carry", "carry_index", "points", "links")}
    # both start from the planted world: the second call of a pair would otherwise see what the first one's apply left
    return {"vslam_world_sim3": s3c.world_sim3(wa, a, d, rr.kmat(), None, capi.ResectParams.make(ctx.lib)).replaced(before=lambda: _plant(ctx, tt, rt)),
            "vslam_world_apply_sim3": s3c.world_apply_sim3(wa, a, ([1, 0], [0, 1])[variant], ad, lambda: _plant(ctx, tt, rt), state)}


def test_world_calls_depend_on_their_arguments_not_on_the_workspace(ctx, two_tracks):
    import entry_calls as ec
    import sim3_calls as s3c
    rt = sc3.ref_tracks(2)
    _plant(ctx, two_tracks, rt)
    calls = _world_calls(ctx, two_tracks, rt, 0)
    assert sorted(calls) == sorted(s3c.WORLD_ENTRIES)
    first = {}
    for name, call in calls.items():
        rc, msg, first[name], _ = ec.run(ctx, call)
        assert rc == 0, (name, msg)
    assert (np.frombuffer(first["vslam_world_sim3"]["d_found"].tobytes(), np.int32) == 1).all()
    planted = np.stack([tr["Twc"] for tr in rt["tracks"]])
    assert not np.array_equal(np.frombuffer(first["vslam_world_apply_sim3"]["state:Twc"].tobytes(), np.float64).reshape(planted.shape), planted)
    for fill in (0x00, 0x5A):
        for name, call in calls.items():
            ctx.workspace_fill(fill)
            rc, msg, got, _ = ec.run(ctx, call)
            assert rc == 0 and not ec._same(first[name], got), (name, fill, ec._same(first[name], got))
    for name, call in calls.items():   # behind a call of the batch entry at another shape
        _device(ctx, [sc3.case(r3.planted(700, 0.6, 9), seed=4, hypotheses=256)], polish={})
        rc, msg, got, _ = ec.run(ctx, call)
        assert rc == 0 and not ec._same(first[name], got), (name, ec._same(first[name], got))


@pytest.mark.parametrize("entry", ["vslam_world_sim3", "vslam_world_apply_sim3"])
def test_world_calls_keep_stream_order_behind_a_stalled_stream(ctx, two_tracks, entry):
    """on the session's context and torch's default stream, as above.  For vslam_world_apply_sim3 this also holds that the host list is
    read before the call returns: its decoy is swapped in behind the call."""
    from entry_calls import Decoys
    from stream_order import choose_sizing, run_behind_stall
    rt = sc3.ref_tracks(2)
    _plant(ctx, two_tracks, rt)
    stream = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == stream
    import entry_calls as ec
    call, other = _world_calls(ctx, two_tracks, rt, 0)[entry], _world_calls(ctx, two_tracks, rt, 1)[entry]
    # every argument's decoy is the other call's (d_matches here is a list of keypoint pairs of two recorded frames with a count of its
    # own, not the front end's list that entry_calls permutes under d_best)
    decoys = Decoys.__new__(Decoys)
    decoys.tensors, decoys.same, decoys.params = {k: other.ins[k].clone() for k in call.ins}, set(), None
    decoys.hosts = {k: ec.host_decoy(k, v, other.hosts[k]) for k, v in call.hosts.items()}
    sizing = choose_sizing(ctx, [call], stream)
    res = run_behind_stall(ctx, call, stream, decoys, sizing)
    assert res.rc == 0, res.msg
    assert res.pending_at_return, f"{entry} waited for the device before it returned"
    assert res.pending_after_tail and res.pending_after_wait, "the stall ended before T_wait had passed"
    assert set(res.got) == set(res.expected)
    for k in res.expected:
        assert np.array_equal(res.expected[k], res.got[k]), f"behind a stalled stream {k} differs from the plain run"


def test_cpp_surfaces_match_the_python_call(ctx, tmp_path):
    """tests/native/sim3_demo.cpp: vslam::sim3_ransac and vslam::sim3_refine (include/vslam/helpers.h) on one item give the bits of
    Context.sim3_ransac / Context.sim3_refine; vslam::World::sim3 and apply_sim3 (include/vslam/World.h) are taken on a world
    attached to an (empty) map, find nothing there, and apply_sim3 throws on a track listed twice."""
    import os
    import struct
    import subprocess
    from vslam_amd import build
    if not os.path.exists(build.HOST_LIB):   # build() has made it; nothing is compiled again here but the demo itself
        build.build_host()
    root = sc3.ROOT
    exe = str(tmp_path / "sim3_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tests", "native", "sim3_demo.cpp"),
                    "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(root, "vslam_amd")], check=True)
    c = sc3.case(r3.planted(300, 0.5, 5), seed=1)
    S = 300
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(c["K"], np.float32).tobytes())
        f.write(struct.pack("3i", S, c["n"], c["seed"]))
        for a, dt in (([sc3.KEEP_S], np.float64), (sc3.KEEP_R, np.float64), (sc3.KEEP_T, np.float64), (c["A"], np.float64), (c["B"], np.float64),
                      (c["xa"], np.float32), (c["xb"], np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    d = _cuda(_batch([c]))
    o = ctx.sim3_ransac(d["A"], d["xa"], d["B"], d["xb"], d["n"], c["K"], d["seeds"], d["scale"], d["R"], d["T"])   # outputs start zeroed
    ctx.synchronize()
    want = b"".join(o[k].cpu().numpy().tobytes() for k in ("scale", "R", "T", "inlier", "corr_index", "n_inliers", "winner"))
    assert int(o["n_inliers"][0]) == 150
    _, _, _, stats = ctx.sim3_refine(d["A"], d["xa"], d["B"], d["xb"], d["n"], c["K"], d["scale"], d["R"], d["T"], mask=o["inlier"])
    ctx.synchronize()
    assert float(stats[0, 3]) >= 1
    want += b"".join(v.cpu().numpy().tobytes() for v in (d["scale"], d["R"], d["T"], stats))
    assert buf[:len(want)] == want
    assert struct.unpack("5i", buf[len(want):]) == (0, 0, 0, 0, 1), "an empty attached map: nothing found; a track listed twice is refused"
