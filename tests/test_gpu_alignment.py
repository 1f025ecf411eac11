"""The pointer-alignment contract of include/vslam_amd.h, entry point by entry point, generated from
tests/alignment_contract.py.  One argument is moved at a time, off the base of its allocation (tests/offset_views.py):

  * an argument that REQUIRES A bytes, at every power-of-two byte offset from its element size up to A / 2: the call is refused
    (VSLAM_ERR_INVALID, vslam_last_error names the argument), every output buffer and every piece of resident state keeps its
    bytes, and the next all-aligned call on the same context gives the all-aligned bits;
  * the same argument exactly A bytes into a larger allocation: accepted, every output equal to the all-aligned result bit for
    bit, the guard bands on both sides of the view untouched (the check is on the address, not on "starts an allocation");
  * an argument declared ANY ADDRESS, at 1, 2, 3, 4 and 8 bytes (u8 / s8 arrays: across these a plane meets every kernel its
    dispatch can choose) or one element (others): accepted, bit for bit, guard bands intact -- inputs and outputs alike.

Nothing is launched at a broken alignment except through an argument the contract declares tolerant.  Everything is a status
code or a bitwise comparison against the all-aligned run of the same call, which the rest of the suite pins to the oracle.
The fixture is the smallest that passes through every stage: 2 pairs of 128 x 96 frames (synth.frames_numpy), 64 keypoint
slots, 64 hypotheses (tests/entry_calls.py, which holds the Call of every entry point)."""
import ctypes as C

import numpy as np
import pytest
import torch

import alignment_contract as ac
from entry_calls import (ENTRIES, FR, H, HYP, INVALID, KP, MAXC, NOT_LAUNCHED, PAIRS, SEED, THR, W, Call, Dbl, Fl, I, P, _bytes,
                         _same, build_calls, build_scene, close_scene, run)
from offset_views import offset_view, sentinel_fill
from vslam_amd import capi

pytestmark = pytest.mark.gpu


def offsets_for(req, elem):
    """-> (element offsets that must be refused, element offsets that must be accepted)."""
    if req == ac.ANY:
        return [], ([1, 2, 3, 4, 8] if elem == 1 else [1])
    bad, b = [], elem
    while b <= req // 2:
        bad.append(b // elem)
        b *= 2
    return bad, [max(req // elem, 1)]


def run_matrix(ctx, call):
    rows = [(a, r) for e, a, r in ac.CONTRACT if e == call.entry and r != ac.HOST]
    assert rows, call.entry
    named = set(call.ins) | set(call.inouts) | set(call.outs) | call.absent
    assert {a for a, _ in rows} == named, (call.entry, sorted({a for a, _ in rows} ^ named))
    rc, msg, ref, _ = run(ctx, call)
    assert rc == 0, (call.entry, msg)
    # what a refused call must leave behind: outputs still the sentinel, in-out arrays and resident state as they were
    if call.before:
        call.before()
    untouched = {}
    for name, (shape, dtype) in call.outs.items():
        if name not in call.scratch:
            untouched[name] = _bytes(sentinel_fill(torch.empty(shape, dtype=dtype, device="cuda")))
    for name, src in call.inouts.items():
        untouched[name] = _bytes(src)
    if call.state:
        untouched.update({"state:" + k: np.ascontiguousarray(v).view(np.uint8).copy() for k, v in call.state().items()
                          if isinstance(v, np.ndarray)})
    failures, cases = [], 0
    for arg, req in rows:
        if arg in call.absent:
            continue
        like = call.ins.get(arg, call.inouts.get(arg))
        elem = like.element_size() if like is not None else torch.empty((), dtype=call.outs[arg][1]).element_size()
        bad, good = offsets_for(req, elem)
        for k in bad:
            cases += 1
            tag = f"{call.entry}({arg}) {k * elem} bytes off a {req}-byte boundary"
            rc, msg, got, check = run(ctx, call, arg, k)
            if rc != INVALID:
                failures.append(f"{tag}: returned {rc}, not VSLAM_ERR_INVALID")
                continue
            if arg not in msg:
                failures.append(f"{tag}: vslam_last_error does not name the argument: {msg!r}")
            check(tag)
            diff = _same(untouched, got)
            if diff:
                failures.append(f"{tag}: a refused call changed {diff}")
            rc, msg, again, _ = run(ctx, call)
            if rc != 0 or _same(ref, again):
                failures.append(f"{tag}: the next aligned call gives rc {rc} {msg!r}, differs in {_same(ref, again) if rc == 0 else '-'}")
        for k in good:
            cases += 1
            tag = f"{call.entry}({arg}) at +{k * elem} bytes" + (" (any address)" if req == ac.ANY else f" (needs {req})")
            rc, msg, got, check = run(ctx, call, arg, k)
            if rc != 0:
                failures.append(f"{tag}: refused: {rc} {msg!r}")
                continue
            check(tag)
            diff = _same(ref, got)
            if diff:
                failures.append(f"{tag}: differs from the all-aligned result in {diff}")
    print(f"{call.entry}: {cases} cases over {len(rows)} device arguments")
    assert not failures, "\n".join(failures)
    return ref


@pytest.fixture(scope="module")
def scene(ctx):
    s = build_scene(ctx, SEED)
    yield s
    close_scene(s)


@pytest.fixture(scope="module")
def calls(ctx, scene):
    return build_calls(ctx, scene)


def test_every_entry_point_with_device_memory_is_launched_or_accounted_for(calls):
    assert sorted(calls) == ENTRIES, sorted(set(calls) ^ set(ENTRIES))
    assert not set(NOT_LAUNCHED) & set(calls)


@pytest.mark.parametrize("entry", ENTRIES)
def test_alignment_matrix(ctx, calls, entry):
    ref = run_matrix(ctx, calls[entry])
    if entry in ("vslam_render_points", "vslam_map_render", "vslam_world_render"):
        assert ref["d_bgr_out"].any(), "something is drawn"


def test_describe_kernels_agree_at_a_width_that_is_a_multiple_of_4_only(ctx, scene):
    """At 128 columns the blurred plane meets the tile-staged kernel (16-byte base), the patch-staged one (4-byte base) and the
    byte kernel (odd base) in the matrix above; at 132 columns the first is out of reach and the other two must agree.  The
    detector's two dispatch sites (the selection's and the response's) see the same odd base of the gray plane here."""
    s = scene
    i32, f32, u8 = torch.int32, torch.float32, torch.uint8
    describe = Call("vslam_orb_describe",
                    [P("d_blurred"), I(FR), I(132), I(H), P("d_xy_in"), P("d_n_in"), I(KP), Fl(s.ca), Fl(s.sa), P("d_pattern"),
                     P("d_xy_out"), P("d_desc"), P("d_n_out")],
                    ins={"d_blurred": s.blur132, "d_xy_in": s.xy_det132, "d_n_in": s.n_det132, "d_pattern": s.pat},
                    outs={"d_xy_out": ((FR, KP, 2), f32), "d_desc": ((FR, KP, 32), u8), "d_n_out": ((FR,), i32)})
    detect = Call("vslam_good_features", [P("d_gray"), I(FR), I(132), I(H), I(MAXC), Dbl(0.01), Dbl(3.0), I(KP), P("d_xy"), P("d_n")],
                  ins={"d_gray": s.gray132}, outs={"d_xy": ((FR, KP, 2), f32), "d_n": ((FR,), i32)})
    blur = Call("vslam_gaussian7", [P("d_gray"), I(FR), I(132), I(H), P("d_out")], ins={"d_gray": s.gray132},
                outs={"d_out": ((FR, H, 132), u8)})
    extract = Call("vslam_extract_features",
                   [P("d_bgr"), I(FR), I(132), I(H), I(3 * 132), ("params", s.ca, s.sa), I(KP), P("d_xy"), P("d_desc"), P("d_nodes"),
                    P("d_n"), P("d_n_detected")],
                   ins={"d_bgr": s.bgr132, "params->d_pattern": s.pat},
                   outs={"d_xy": ((FR, KP, 2), f32), "d_desc": ((FR, KP, 32), u8), "d_nodes": ((FR, KP), i32), "d_n": ((FR,), i32),
                         "d_n_detected": ((FR,), i32)})
    for call in (describe, detect, blur, extract):
        ref = run_matrix(ctx, call)
        counts = ref.get("d_n_out", ref.get("d_n"))
        if counts is not None:
            assert (counts.view(np.int32) >= 8).all(), (call.entry, counts.view(np.int32))


def test_odd_kp_stride_rows_on_8_byte_boundaries(ctx, scene):
    """kp_stride 63 with all-aligned bases: row 1 of every (x, y) / index-pair array then starts 504 bytes in -- on an 8-byte and
    not a 16-byte boundary, inside a legal call.  Slot by slot the batch must give what the pairs give at kp_stride 64."""
    s, f = scene, scene.fp
    K1 = KP - 1
    assert int(f["n"].max()) <= K1

    def cut(t):
        return t[:, :K1].contiguous()
    xy1, xy2, d1, d2 = cut(s.xy1), cut(s.xy2), cut(s.desc1), cut(s.desc2)
    pairs64, m64, knn64 = ctx.match_knn2_ratio(s.desc1, s.n1, s.desc2, s.n2, want_knn=True)
    pairs, m, knn = ctx.match_knn2_ratio(d1, s.n1, d2, s.n2, want_knn=True)
    ctx.synchronize()
    assert torch.equal(m, m64)
    for p in range(PAIRS):       # slots past the counts are not written
        assert torch.equal(pairs[p, :int(m[p])], pairs64[p, :int(m[p])]) and int(m[p]) >= 8, p
        assert torch.equal(knn[p, :int(s.n1[p])], knn64[p, :int(s.n1[p])]), p
    rf = ctx.ransac_fundamental(xy1, xy2, pairs, m, s.sets, THR)
    ctx.synchronize()
    assert torch.equal(rf["best"], s.rf["best"]) and torch.equal(rf["F"].view(torch.int32), s.rf["F"].view(torch.int32))
    assert torch.equal(rf["matches"], cut(s.rf["matches"])) and torch.equal(rf["mask"], cut(s.rf["mask"]))
    assert torch.equal(rf["hypF"].view(torch.int32), s.rf["hypF"].view(torch.int32))
    mf = ctx.match_features(xy1, d1, s.n1, xy2, d2, s.n2, s.seeds, HYP, THR)
    ctx.synchronize()
    assert torch.equal(mf["best"], f["best"]) and torch.equal(mf["matches"], cut(f["matches"]))
    assert torch.equal(mf["F"].view(torch.int32), f["F"].view(torch.int32))
    nodes = ctx.kdtree_build(cut(f["xy"]), f["n"])
    ctx.synchronize()
    for fr in range(FR):
        k = int(f["n"][fr])
        assert torch.equal(nodes[fr, :k], f["nodes"][fr, :k]), fr
    pts = ctx.triangulate(xy1, xy2, mf["matches"], mf["best"], scene.Kh, f["c2"])
    idx, n_in, err = ctx.reprojection_filter(pts, xy1, xy2, mf["matches"], mf["best"], scene.Kh, f["c2"], cut(s.ids_free))
    Fr, _ = ctx.refit_fundamental(xy1, xy2, mf["matches"], mf["best"], mf["F"])
    Fr64, _ = ctx.refit_fundamental(s.xy1, s.xy2, f["matches"], f["best"], f["F"])
    ctx.synchronize()
    for p in range(PAIRS):
        k = int(f["best"][p, 3])
        assert torch.equal(pts[p, :k].view(torch.int32), f["points4d"][p, :k].view(torch.int32)), p
    assert torch.equal(n_in, f["n_inliers"]) and torch.equal(err.view(torch.int64), f["error"].view(torch.int64))
    for p in range(PAIRS):
        assert torch.equal(idx[p, :int(n_in[p])], f["inlier_idx"][p, :int(n_in[p])]), p
    assert torch.equal(Fr.view(torch.int32), Fr64.view(torch.int32))
    # the whole front end at 63 slots per frame: the same frames, the same seeds
    out = ctx.frontend_pairs(s.bgr, PAIRS, MAXC, s.ca, s.sa, s.pat, s.seeds, HYP, THR, kp_stride=K1)
    ctx.synchronize()
    assert torch.equal(out["n"], f["n"]) and torch.equal(out["best"], f["best"])
    assert torch.equal(out["xy"].view(torch.int32), cut(f["xy"]).view(torch.int32)) and torch.equal(out["desc"], cut(f["desc"]))
    assert torch.equal(out["matches"], cut(f["matches"])) and torch.equal(out["F"].view(torch.int32), f["F"].view(torch.int32))


def test_pipeline_refuses_at_once_and_the_slot_stays_usable(ctx, scene):
    """vslam_pipeline_submit_pairs on two contexts: a descriptor array one byte off is refused at once, ticket -1, no failure
    filed under any ticket; the next submits -- the second of them on the refused slot -- are exact, and drain() is clean."""
    s, f = scene, scene.fp
    pipe = capi.Pipeline(0, n_ctx=2)
    try:
        def outputs():
            out = capi.Pipeline.alloc_outputs(torch, FR, PAIRS, KP, "cuda")
            for t in out.values():
                sentinel_fill(t)
            torch.cuda.synchronize()
            return out

        def submit(out):
            p = pipe.contexts[0]._params(MAXC, s.ca, s.sa, s.pat)
            t = C.c_int64(12345)
            rc = pipe.lib.vslam_pipeline_submit_pairs(
                pipe.handle, C.c_void_p(s.bgr.data_ptr()), I(PAIRS), I(W), I(H), I(3 * W), C.byref(p), I(KP),
                C.c_void_p(s.seeds.data_ptr()), I(HYP), Fl(THR), *(C.c_void_p(out[k].data_ptr()) for k in
                                                                  ("xy", "desc", "nodes", "n", "matches", "best", "F")),
                C.c_void_p(0), C.byref(t))
            return rc, t.value
        bad = outputs()
        desc_view, _, check = offset_view((FR, KP, 32), torch.uint8, 1)
        torch.cuda.synchronize()
        rc, ticket = submit(dict(bad, desc=desc_view))
        assert rc == INVALID and ticket == -1
        assert "d_desc" in pipe.lib.vslam_pipeline_last_error(pipe.handle).decode()
        torch.cuda.synchronize()
        check("pipeline")
        for k, t in bad.items():
            assert bool((t.view(torch.uint8) == 0xA5).all()), k
        assert bool((desc_view == 0xA5).all())
        for _ in range(2):           # slot 1, then slot 0: the one that was refused
            out = capi.Pipeline.alloc_outputs(torch, FR, PAIRS, KP, "cuda")     # filled as the fixture's were
            rc, ticket = submit(out)
            assert rc == 0 and ticket >= 0
            pipe.wait(ticket)
            for k in ("n", "best", "matches", "desc", "nodes"):
                assert torch.equal(out[k], f[k]), k
            for k in ("xy", "F"):
                assert torch.equal(out[k].view(torch.int32), f[k].view(torch.int32)), k
        pipe.drain()
    finally:
        pipe.close()
