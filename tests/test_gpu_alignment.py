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
slots, 64 hypotheses."""
import ctypes as C

import numpy as np
import pytest
import torch

import alignment_contract as ac
from offset_views import offset_view, sentinel_fill
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu

SEED, W, H, PAIRS, FR = 35, 128, 96, 2, 4
MAXC, KP, HYP, THR = 60, 64, 64, 10.0
GRID_CAP = 256
RW, RH = 64, 48            # rendered image
INVALID = -1

I, Fl, Dbl, U32 = C.c_int, C.c_float, C.c_double, C.c_uint32


def P(name):
    return ("p", name)


def _K(w, h):
    return np.array([525, 0, w // 2, 0, 525, h // 2, 0, 0, 1], np.float32)     # src/vslam.cpp:32


class Call:
    """One entry point with everything it is handed.  Tensors are named as the header names the arguments
    (`params->d_pattern`, `pose->d_R` for struct members)."""

    def __init__(self, entry, argv, ins=None, inouts=None, outs=None, scratch=(), absent=(), before=None, state=None, keep=()):
        self.entry, self.argv = entry, argv
        self.ins, self.inouts, self.outs = dict(ins or {}), dict(inouts or {}), dict(outs or {})
        self.scratch = set(scratch)      # outputs whose contents are bookkeeping that may depend on timing: never compared
        self.absent = set(absent)        # optional device arguments this call passes as NULL
        self.before, self.state = before, state
        self.keep = keep                 # host arrays the argv points into


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def run(ctx, call, moved=None, offset=0):
    """-> (rc, message, {name: bytes of every output / in-out tensor and state array}, guard check or None)."""
    t = dict(call.ins)
    for name, src in call.inouts.items():
        t[name] = src.clone()
    for name, (shape, dtype) in call.outs.items():
        t[name] = sentinel_fill(torch.empty(shape, dtype=dtype, device="cuda"))
    check = None
    if moved is not None:
        like = t[moved]
        view, _whole, check = offset_view(tuple(like.shape), like.dtype, offset)
        if moved in call.ins or moved in call.inouts:
            view.copy_(like)
        t[moved] = view
    if call.before:
        call.before()
    argv = []
    for a in call.argv:
        if isinstance(a, tuple) and a[0] == "p":
            argv.append(C.c_void_p(t[a[1]].data_ptr()) if a[1] in t else C.c_void_p(0))
        elif isinstance(a, tuple) and a[0] == "params":
            p = capi.ExtractParams()
            p.max_corners, p.quality, p.min_distance, p.cos_a, p.sin_a = MAXC, 0.01, 3.0, a[1], a[2]
            p.d_pattern = t["params->d_pattern"].data_ptr()
            argv.append(C.byref(p))
        elif isinstance(a, tuple) and a[0] == "pose":
            po = capi.PoseOutputs(*(C.c_void_p(t["pose->d_" + k].data_ptr())
                                    for k in ("R", "t", "c2", "points4d", "inlier_idx", "n_inliers", "error")))
            argv.append(C.byref(po))
        else:
            argv.append(a)
    torch.cuda.synchronize()             # the fills above, whatever stream the context runs on
    rc = getattr(ctx.lib, call.entry)(ctx.handle, *argv)
    msg = (ctx.lib.vslam_last_error(ctx.handle) or b"").decode() if rc else ""
    status = ctx.lib.vslam_ctx_synchronize(ctx.handle)
    if status == -2:     # VSLAM_ERR_HIP: nothing more is started on a device that has just faulted
        pytest.exit(f"HIP error behind {call.entry} (moved {moved} by {offset} elements): "
                    f"{(ctx.lib.vslam_last_error(ctx.handle) or b'').decode()}", returncode=3)
    assert status == 0, (call.entry, moved, offset, status)
    got = {name: _bytes(t[name]) for name in list(call.outs) + list(call.inouts) if name not in call.scratch}
    if call.state:
        got.update({"state:" + k: np.ascontiguousarray(v).view(np.uint8).copy() for k, v in call.state().items()
                    if isinstance(v, np.ndarray)})
    return rc, msg, got, check


def _same(a, b):
    return sorted(k for k in a if not np.array_equal(a[k], b[k]))


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


# ---------------------------------------------------------------------------------------------------------------- the fixture
class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    s = Scene()
    dev = "cuda"
    s.ca, s.sa = synth.keypoint_rotation()
    s.pat = torch.from_numpy(synth.brief_pattern()).to(dev)
    s.Kh = _K(W, H)
    s.Kp = s.Kh.ctypes.data_as(C.c_void_p)
    bgr_np = synth.frames_numpy(SEED, PAIRS, W, H)
    s.bgr = torch.from_numpy(bgr_np).to(dev)
    s.seeds = torch.from_numpy((np.arange(PAIRS, dtype=np.uint32) + SEED * 7).view(np.int32).copy()).to(dev)
    s.fp = ctx.frontend_pairs_pose(s.bgr, PAIRS, MAXC, s.ca, s.sa, s.pat, s.seeds, HYP, THR, s.Kh, kp_stride=KP)
    ctx.synchronize()
    f = s.fp
    best = f["best"].cpu().numpy()
    n = f["n"].cpu().numpy()
    print("fixture: keypoints", n, "best", best.tolist(), "reprojection inliers", f["n_inliers"].cpu().numpy())
    assert (n >= 8).all() and (best[:, 0] >= 0).all() and (best[:, 3] >= 8).all(), "every stage needs a model on both pairs"
    s.xy1, s.xy2 = f["xy"][:PAIRS].contiguous(), f["xy"][PAIRS:].contiguous()
    s.desc1, s.desc2 = f["desc"][:PAIRS].contiguous(), f["desc"][PAIRS:].contiguous()
    s.n1, s.n2 = f["n"][:PAIRS].contiguous(), f["n"][PAIRS:].contiguous()
    s.nodes2 = f["nodes"][PAIRS:].contiguous()
    s.gray = ctx.bgr2gray(s.bgr)
    s.blur = ctx.gaussian7(s.gray)
    s.xy_det, s.n_det = ctx.good_features(s.gray, MAXC, kp_stride=KP)
    s.pairs, s.m, _ = ctx.match_knn2_ratio(s.desc1, s.n1, s.desc2, s.n2, want_knn=True)
    s.sets = ctx.ransac_sets(s.seeds, s.m, HYP)
    s.rf = ctx.ransac_fundamental(s.xy1, s.xy2, s.pairs, s.m, s.sets, THR)
    s.ids_free = torch.full((PAIRS, KP), -1, dtype=torch.int32, device=dev)
    # a width that is a multiple of 4 and not of 16, for the plane-reading stages
    s.bgr132 = torch.from_numpy(synth.frames_numpy(SEED, PAIRS, 132, H)).to(dev)
    s.gray132 = ctx.bgr2gray(s.bgr132)
    s.blur132 = ctx.gaussian7(s.gray132)
    s.xy_det132, s.n_det132 = ctx.good_features(s.gray132, MAXC, kp_stride=KP)
    # a map of the pairs' own triangulated points, each observed once by the keypoint it was matched to in the current frame
    ctx.synchronize()
    matches = f["matches"].cpu().numpy()
    desc2 = s.desc2.cpu().numpy()
    obs_desc = np.zeros((PAIRS, KP, 32), np.uint8)
    offsets = np.zeros((PAIRS, KP + 1), np.int32)
    for p in range(PAIRS):
        k = int(best[p, 3])
        obs_desc[p, :k] = desc2[p, matches[p, :k, 1]]
        offsets[p] = np.minimum(np.arange(KP + 1), k)
    s.obs_desc, s.obs_offsets = torch.from_numpy(obs_desc).to(dev), torch.from_numpy(offsets).to(dev)
    s.n_map = torch.from_numpy(best[:, 3].astype(np.int32)).to(dev)
    s.colors = torch.from_numpy(np.random.default_rng(SEED).integers(1, 256, (PAIRS, KP, 3), dtype=np.uint8)).to(dev)
    # resident state: one map and world for the stepping calls (reset in front of every call), one pair left stepped for the
    # calls that only read them
    s.pmap = capi.PointMap(ctx, PAIRS, 3, KP, KP, 4 * KP)
    s.world = capi.World(ctx, PAIRS, 3, KP, min_links=1)
    s.pmap_done = capi.PointMap(ctx, PAIRS, 3, KP, KP, 4 * KP)
    s.world_done = s.pmap_done.attach_world(min_links=1)
    last = dict(xy=s.xy1, desc=s.desc1, n=s.n1)
    cur = dict(xy=s.xy2, desc=s.desc2, nodes=s.nodes2, n=s.n2)
    s.pmap_done.step(last, cur, f, s.bgr[PAIRS:].contiguous(), s.Kh)
    ctx.synchronize()
    v = s.pmap_done.view()
    print("fixture: map sizes", v["sizes"], "observations", v["n_obs"], "world links", v["world_links"][:, 1])
    s.world_pose = torch.from_numpy(v["world_pose"]).to(dev)
    s.view = capi.View.default(RW, RH, ctx.lib)
    for i in range(16):
        s.view.mv[i] = 1.0 if i % 5 == 0 else 0.0        # the viewer is the pair's first camera
    s.view.fu = s.view.fv = 10.0                          # wide: frame 0's frustum and every point in front of it are in view
    s.view.point_size = 3
    torch.cuda.synchronize()
    yield s
    s.pmap.close(); s.world.close(); s.pmap_done.close(); s.world_done.close()


def _front_outs(frames, pairs):
    i32, f32 = torch.int32, torch.float32
    return {"d_xy": ((frames, KP, 2), f32), "d_desc": ((frames, KP, 32), torch.uint8), "d_nodes": ((frames, KP), i32),
            "d_n": ((frames,), i32), "d_matches": ((pairs, KP, 2), i32), "d_best": ((pairs, 4), i32), "d_F": ((pairs, 9), f32)}


_POSE_OUTS = {"pose->d_R": ((PAIRS, 9), torch.float32), "pose->d_t": ((PAIRS, 3), torch.float32),
              "pose->d_c2": ((PAIRS, 12), torch.float32), "pose->d_points4d": ((PAIRS, KP, 4), torch.float32),
              "pose->d_inlier_idx": ((PAIRS, KP), torch.int32), "pose->d_n_inliers": ((PAIRS,), torch.int32),
              "pose->d_error": ((PAIRS,), torch.float64)}
_FRONT_ARGS = [P("d_xy"), P("d_desc"), P("d_nodes"), P("d_n"), P("d_matches"), P("d_best"), P("d_F")]


def build_calls(ctx, s):
    i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
    f = s.fp
    B, K = PAIRS, KP
    img = [I(W), I(H), I(3 * W)]
    params = ("params", s.ca, s.sa)
    ransac_in = {"d_xy1": s.xy1, "d_xy2": s.xy2, "d_pairs": s.pairs, "d_m": s.m}
    pose_in = {"d_xy1": s.xy1, "d_xy2": s.xy2, "d_matches": f["matches"], "d_best": f["best"]}
    ransac_out = {"d_F": ((B, 9), f32), "d_mask": ((B, K), u8), "d_best": ((B, 4), i32), "d_matches": ((B, K, 2), i32),
                  "d_hyp_count": ((B, HYP), i32), "d_hyp_sum": ((B, HYP), f32)}
    tree = {"d_nodes": f["nodes"], "d_xy": f["xy"], "d_n": f["n"]}
    queries = (f["xy"] + 0.5).contiguous()
    c1 = np.array([525, 0, W // 2, 0, 0, 525, H // 2, 0, 0, 0, 1, 0], np.float32)
    c2 = np.ascontiguousarray(f["c2"][0].cpu().numpy())
    seeds3 = torch.from_numpy((np.arange(FR - 1, dtype=np.uint32) + SEED * 7).view(np.int32).copy()).cuda()
    seq = torch.stack([s.bgr[:PAIRS], s.bgr[PAIRS:]], dim=1).contiguous()          # (tracks, 2 frames, H, W, 3)
    seeds_t = s.seeds.reshape(PAIRS, 1).contiguous()
    lo, hi = torch.zeros((B,), dtype=i32, device="cuda"), s.n_map.clone()
    render_out = {"d_bgr_out": ((B, RH, 3 * RW), u8), "d_depth_out": ((B, RH, RW), f32)}
    render_tail = [C.byref(s.view), I(RW), I(RH), I(3 * RW), P("d_bgr_out"), P("d_depth_out")]

    def map_state(pmap):
        def state():
            v = pmap.view()
            off, fr, pt = pmap.observations()
            v.update(offsets=off.cpu().numpy(), obs_frames=fr.cpu().numpy(), obs_points=pt.cpu().numpy())
            return v
        return state

    calls = [
        Call("vslam_match_knn2_ratio", [P("d_desc1"), P("d_n1"), P("d_desc2"), P("d_n2"), I(B), I(K), P("d_pairs"), P("d_m"), P("d_knn")],
             ins={"d_desc1": s.desc1, "d_n1": s.n1, "d_desc2": s.desc2, "d_n2": s.n2},
             outs={"d_pairs": ((B, K, 2), i32), "d_m": ((B,), i32), "d_knn": ((B, K, 4), i32)}),
        Call("vslam_ransac_sets", [P("d_seeds"), P("d_m"), I(B), I(HYP), P("d_sets"), P("d_draw_scratch")],
             ins={"d_seeds": s.seeds, "d_m": s.m}, outs={"d_sets": ((B, HYP, 8), i32), "d_draw_scratch": ((B, HYP * 8), i32)},
             scratch=["d_draw_scratch"]),
        Call("vslam_ransac_fundamental",
             [P("d_xy1"), P("d_xy2"), P("d_pairs"), P("d_m"), P("d_sets"), I(B), I(K), I(HYP), Fl(THR), P("d_F"), P("d_mask"), P("d_best"),
              P("d_matches"), P("d_hypF"), P("d_hyp_count"), P("d_hyp_sum")],
             ins=dict(ransac_in, d_sets=s.sets), outs=dict(ransac_out, d_hypF=((B, HYP, 9), f32)),
             scratch=["d_hyp_count", "d_hyp_sum"]),       # which losing hypotheses are abandoned early is not fixed
        Call("vslam_ransac_solve", [P("d_xy1"), P("d_xy2"), P("d_pairs"), P("d_m"), P("d_sets"), I(B), I(K), I(HYP), P("d_hypF")],
             ins=dict(ransac_in, d_sets=s.sets), outs={"d_hypF": ((B, HYP, 9), f32)}),
        Call("vslam_ransac_evaluate",
             [P("d_xy1"), P("d_xy2"), P("d_pairs"), P("d_m"), P("d_hypF"), I(B), I(K), I(HYP), Fl(THR), P("d_F"), P("d_mask"), P("d_best"),
              P("d_matches"), P("d_hyp_count"), P("d_hyp_sum")],
             ins=dict(ransac_in, d_hypF=s.rf["hypF"]), outs=ransac_out, scratch=["d_hyp_count", "d_hyp_sum"]),
        Call("vslam_refit_fundamental", [P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(B), I(K), P("d_F_in"), P("d_F_out"), P("d_stats")],
             ins=dict(pose_in, d_F_in=f["F"]), outs={"d_F_out": ((B, 9), f32), "d_stats": ((B, 4), f64)}),
        Call("vslam_refine_pairs",
             [P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(B), I(K), s.Kp, Fl(16.0), I(20), P("d_R"), P("d_t"), P("d_c2"),
              P("d_points4d"), P("d_stats")],
             ins=pose_in, inouts={"d_R": f["R"], "d_t": f["t"], "d_points4d": f["points4d"]},
             outs={"d_c2": ((B, 12), f32), "d_stats": ((B, 4), f64)}),
        Call("vslam_kdtree_build", [P("d_xy"), P("d_n"), I(FR), I(K), P("d_nodes")], ins={"d_xy": f["xy"], "d_n": f["n"]},
             outs={"d_nodes": ((FR, K), i32)}),
        Call("vslam_kdtree_radius",
             [P("d_nodes"), P("d_xy"), P("d_n"), I(FR), I(K), P("d_queries"), P("d_nq"), I(K), Fl(12.0), P("d_hits"), P("d_counts"), I(8)],
             ins=dict(tree, d_queries=queries, d_nq=f["n"]), outs={"d_hits": ((FR, K, 8), i32), "d_counts": ((FR, K), i32)}),
        Call("vslam_kdtree_nearest",
             [P("d_nodes"), P("d_xy"), P("d_n"), I(FR), I(K), P("d_queries"), P("d_nq"), I(K), Fl(1e9), P("d_best_idx")],
             ins=dict(tree, d_queries=queries, d_nq=f["n"]), outs={"d_best_idx": ((FR, K), i32)}),
        Call("vslam_kdtree_cell_table", [P("d_nodes"), P("d_xy"), P("d_n"), I(FR), I(K), I(2 * K), P("d_table"), P("d_ok")],
             ins=tree, outs={"d_table": ((FR, 2 * K, 2), i32), "d_ok": ((FR,), i32)},
             scratch=["d_table"]),                        # colliding keys take their slots in arrival order
        Call("vslam_extract_features",
             [P("d_bgr"), I(FR)] + img + [params, I(K), P("d_xy"), P("d_desc"), P("d_nodes"), P("d_n"), P("d_n_detected")],
             ins={"d_bgr": s.bgr, "params->d_pattern": s.pat},
             outs={k: v for k, v in list(_front_outs(FR, B).items())[:4]} | {"d_n_detected": ((FR,), i32)}),
        Call("vslam_extract_features_grid",
             [P("d_bgr"), I(FR)] + img + [I(1), I(1), P("d_pattern"), I(GRID_CAP), P("d_xy"), P("d_desc"), P("d_angle_octave"), P("d_n")],
             ins={"d_pattern": s.pat}, inouts={"d_bgr": s.bgr},
             outs={"d_xy": ((FR, GRID_CAP, 2), f32), "d_desc": ((FR, GRID_CAP, 32), u8), "d_angle_octave": ((FR, GRID_CAP, 2), f32),
                   "d_n": ((FR,), i32)}),
        Call("vslam_bgr2gray", [P("d_bgr"), I(FR)] + img + [P("d_gray")], ins={"d_bgr": s.bgr}, outs={"d_gray": ((FR, H, W), u8)}),
        Call("vslam_min_eigen", [P("d_gray"), I(FR), I(W), I(H), P("d_eig")], ins={"d_gray": s.gray}, outs={"d_eig": ((FR, H, W), f32)}),
        Call("vslam_good_features", [P("d_gray"), I(FR), I(W), I(H), I(MAXC), Dbl(0.01), Dbl(3.0), I(K), P("d_xy"), P("d_n")],
             ins={"d_gray": s.gray}, outs={"d_xy": ((FR, K, 2), f32), "d_n": ((FR,), i32)}),
        Call("vslam_gaussian7", [P("d_gray"), I(FR), I(W), I(H), P("d_out")], ins={"d_gray": s.gray}, outs={"d_out": ((FR, H, W), u8)}),
        Call("vslam_orb_describe",
             [P("d_blurred"), I(FR), I(W), I(H), P("d_xy_in"), P("d_n_in"), I(K), Fl(s.ca), Fl(s.sa), P("d_pattern"), P("d_xy_out"),
              P("d_desc"), P("d_n_out")],
             ins={"d_blurred": s.blur, "d_xy_in": s.xy_det, "d_n_in": s.n_det, "d_pattern": s.pat},
             outs={"d_xy_out": ((FR, K, 2), f32), "d_desc": ((FR, K, 32), u8), "d_n_out": ((FR,), i32)}),
        Call("vslam_extract_Rt", [P("d_F"), P("d_best"), I(B), s.Kp, P("d_R"), P("d_t"), P("d_c2")],
             ins={"d_F": f["F"], "d_best": f["best"]}, outs={"d_R": ((B, 9), f32), "d_t": ((B, 3), f32), "d_c2": ((B, 12), f32)}),
        Call("vslam_triangulate",
             [P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(B), I(K), s.Kp, P("d_c2"), P("d_points4d")],
             ins=dict(pose_in, d_c2=f["c2"]), outs={"d_points4d": ((B, K, 4), f32)}),
        Call("vslam_triangulate_points",
             [P("d_p1"), P("d_p2"), I(K), c1.ctypes.data_as(C.c_void_p), c2.ctypes.data_as(C.c_void_p), P("d_points4d")],
             ins={"d_p1": s.xy1[0].contiguous(), "d_p2": s.xy2[0].contiguous()}, outs={"d_points4d": ((K, 4), f32)}, keep=(c1, c2)),
        Call("vslam_reprojection_filter",
             [P("d_points4d"), P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(B), I(K), s.Kp, P("d_c2"), P("d_map_point_ids"),
              Fl(4.0), P("d_inlier_idx"), P("d_n_inliers"), P("d_error")],
             ins=dict(pose_in, d_points4d=f["points4d"], d_c2=f["c2"], d_map_point_ids=s.ids_free),
             outs={"d_inlier_idx": ((B, K), i32), "d_n_inliers": ((B,), i32), "d_error": ((B,), f64)}),
        Call("vslam_associate_map_points",
             [P("d_map_points"), P("d_n_map"), I(B), I(K), P("d_c2"), I(W), I(H), P("d_nodes"), P("d_xy"), P("d_desc"), P("d_n"), I(K),
              P("d_obs_offsets"), P("d_obs_desc"), I(K), Fl(2.0), U32(64), P("d_map_point_ids"), P("d_claim")],
             ins={"d_map_points": f["points4d"], "d_n_map": s.n_map, "d_c2": f["c2"], "d_nodes": s.nodes2, "d_xy": s.xy2,
                  "d_desc": s.desc2, "d_n": s.n2, "d_obs_offsets": s.obs_offsets, "d_obs_desc": s.obs_desc},
             inouts={"d_map_point_ids": s.ids_free}, outs={"d_claim": ((B, K), i32)}),
        Call("vslam_match_features",
             [P("d_xy1"), P("d_desc1"), P("d_n1"), P("d_xy2"), P("d_desc2"), P("d_n2"), I(B), I(K), P("d_seeds"), I(HYP), Fl(THR),
              P("d_matches"), P("d_best"), P("d_F"), P("d_prelim_m")],
             ins={"d_xy1": s.xy1, "d_desc1": s.desc1, "d_n1": s.n1, "d_xy2": s.xy2, "d_desc2": s.desc2, "d_n2": s.n2, "d_seeds": s.seeds},
             outs={"d_matches": ((B, K, 2), i32), "d_best": ((B, 4), i32), "d_F": ((B, 9), f32), "d_prelim_m": ((B,), i32)}),
        Call("vslam_frontend_pairs", [P("d_bgr"), I(B)] + img + [params, I(K), P("d_seeds"), I(HYP), Fl(THR)] + _FRONT_ARGS,
             ins={"d_bgr": s.bgr, "params->d_pattern": s.pat, "d_seeds": s.seeds}, outs=_front_outs(FR, B)),
        Call("vslam_frontend_pairs_pose",
             [P("d_bgr"), I(B)] + img + [params, I(K), P("d_seeds"), I(HYP), Fl(THR)] + _FRONT_ARGS +
             [s.Kp, P("d_map_point_ids"), Fl(4.0), ("pose",)],
             ins={"d_bgr": s.bgr, "params->d_pattern": s.pat, "d_seeds": s.seeds, "d_map_point_ids": s.ids_free},
             outs=dict(_front_outs(FR, B), **_POSE_OUTS)),
        Call("vslam_frontend_sequence", [P("d_bgr"), I(FR)] + img + [params, I(K), P("d_seeds"), I(HYP), Fl(THR)] + _FRONT_ARGS,
             ins={"d_bgr": s.bgr, "params->d_pattern": s.pat, "d_seeds": seeds3}, outs=_front_outs(FR, FR - 1)),
        Call("vslam_pack_records", [P("d_F"), P("d_best"), P("d_matches"), I(B), I(K), P("d_records")],
             ins={"d_F": f["F"], "d_best": f["best"], "d_matches": f["matches"]}, outs={"d_records": ((B, 13 + K), i32)}),
        Call("vslam_map_step",
             [s.pmap.handle, P("d_xy_last"), P("d_desc_last"), P("d_n_last"), P("d_xy_cur"), P("d_desc_cur"), P("d_nodes_cur"), P("d_n_cur"),
              P("d_matches"), P("d_best"), P("d_F"), P("d_bgr_cur")] + img + [s.Kp, Fl(2.0), U32(64), Fl(4.0)],
             ins={"d_xy_last": s.xy1, "d_desc_last": s.desc1, "d_n_last": s.n1, "d_xy_cur": s.xy2, "d_desc_cur": s.desc2,
                  "d_nodes_cur": s.nodes2, "d_n_cur": s.n2, "d_matches": f["matches"], "d_best": f["best"], "d_F": f["F"],
                  "d_bgr_cur": s.bgr[PAIRS:].contiguous()},
             before=s.pmap.reset, state=map_state(s.pmap)),
        Call("vslam_track_sequences",
             [s.pmap.handle, P("d_bgr"), I(2)] + img + [params, P("d_seeds"), I(HYP), Fl(THR), s.Kp, Fl(2.0), U32(64), Fl(4.0)] + _FRONT_ARGS,
             ins={"d_bgr": seq, "params->d_pattern": s.pat, "d_seeds": seeds_t}, outs=_front_outs(FR, FR - 1),
             before=s.pmap.reset, state=map_state(s.pmap)),
        Call("vslam_map_observations", [s.pmap_done.handle, P("d_offsets"), P("d_frame_ids"), P("d_point_ids")],
             outs={"d_offsets": ((B, K + 1), i32), "d_frame_ids": ((B, 4 * K), i32), "d_point_ids": ((B, 4 * K), i32)}),
        Call("vslam_render_points",
             [P("d_points"), P("d_colors"), P("d_sizes"), I(B), I(K), P("d_pose"), I(2), I(3)] + render_tail,
             ins={"d_points": f["points4d"], "d_colors": s.colors, "d_sizes": s.n_map, "d_pose": s.world_pose}, outs=render_out),
        Call("vslam_map_render", [s.pmap_done.handle, I(0), I(B)] + render_tail, outs=render_out),
        Call("vslam_world_render", [s.world_done.handle, s.pmap_done.handle, I(0), I(B)] + render_tail, outs=render_out),
        Call("vslam_world_step",
             [s.world.handle, P("d_matches"), P("d_best"), P("d_points4d"), P("d_R"), P("d_t"), P("d_n_last"), P("d_n_cur")],
             ins={"d_matches": f["matches"], "d_best": f["best"], "d_points4d": f["points4d"], "d_R": f["R"], "d_t": f["t"],
                  "d_n_last": s.n1, "d_n_cur": s.n2},
             before=s.world.reset, state=s.world.view),
        Call("vslam_world_lift", [s.world_done.handle, I(1), P("d_points"), I(K), P("d_lo"), P("d_hi"), P("d_out")],
             ins={"d_points": f["points4d"], "d_lo": lo, "d_hi": hi}, outs={"d_out": ((B, K, 4), f32)}),
        Call("vslam_debug_stream_copy", [P("d_src"), P("d_dst"), C.c_size_t(4096), I(16)],
             ins={"d_src": s.gray.reshape(-1)[:4096].contiguous()}, outs={"d_dst": ((4096,), u8)}),
    ]
    return {c.entry: c for c in calls}


# Entry points with device-pointer arguments that this file does not launch, and why.
NOT_LAUNCHED = {
    "vslam_dev_free": "takes back what vslam_dev_alloc returned: there is no other address to hand it",
    "vslam_copy_h2d": "hipMemcpy, byte granular; any address by the runtime's own contract",
    "vslam_copy_d2h": "hipMemcpy, byte granular",
    "vslam_upload_async": "hipMemcpyAsync, byte granular",
    "vslam_download_async": "hipMemcpyAsync, byte granular",
    "vslam_pipeline_submit_pairs": "test_pipeline_refuses_at_once_and_the_slot_stays_usable",
    "vslam_pipeline_submit_pairs_pose": "the same wrapper around vslam_frontend_pairs_pose, whose matrix runs on a plain context",
    "vslam_pipeline_submit_sequence": "the same wrapper around vslam_frontend_sequence, whose matrix runs on a plain context",
    "vslam_multi_frontend_pairs": "host images; params->d_pattern must be NULL",
    "vslam_multi_frontend_pairs_resident": "one host thread and context per device around vslam_frontend_pairs",
    "vslam_gather_records": "needs an RCCL communicator; its arrays have their element's own alignment only",
    "vslam_gather_records_v": "needs an RCCL communicator; its arrays have their element's own alignment only",
}

ENTRIES = sorted({e for e, _, r in ac.CONTRACT if r != ac.HOST} - set(NOT_LAUNCHED))


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
