"""One Call per entry point of include/vslam_amd.h that takes device memory, on the smallest fixture that passes through every
stage: 2 pairs of 128 x 96 frames (synth.frames_numpy), 64 keypoint slots, 64 hypotheses.  Shared by the tests that hold the C
ABI to a contract entry by entry: tests/test_gpu_alignment.py (where a pointer may point) and tests/test_gpu_stream_order.py
(when the memory behind it is read and written).

  build_scene(ctx, seed)      the tensors, host arguments and resident maps / worlds every call is made of
  build_calls(ctx, scene)     {entry point: Call}
  run(ctx, call)              the fully synchronised run of one Call: inputs complete before it, outputs read after a wait
  decoy_scene / build_decoys  a second valid value for every input of every Call (see DECOYS below)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import alignment_contract as ac
from offset_views import offset_view, sentinel_fill
from vslam_amd import capi, synth

SEED, W, H, PAIRS, FR = 35, 128, 96, 2, 4
MAXC, KP, HYP, THR = 60, 64, 64, 10.0
GRID_CAP = 256
RW, RH = 64, 48            # rendered image
INVALID = -1

I, Fl, Dbl, U32 = C.c_int, C.c_float, C.c_double, C.c_uint32
POSE_MEMBERS = ("R", "t", "c2", "points4d", "inlier_idx", "n_inliers", "error")


def P(name):
    return ("p", name)


def Hst(name):
    """A host argument (an array or a struct the entry point copies at the call), by the name the header gives it."""
    return ("h", name)


def _K(w, h):
    return np.array([525, 0, w // 2, 0, 525, h // 2, 0, 0, 1], np.float32)     # src/vslam.cpp:32


class Call:
    """One entry point with everything it is handed.  Tensors are named as the header names the arguments
    (`params->d_pattern`, `pose->d_R` for struct members); host arrays and structs likewise, in `hosts`."""

    def __init__(self, entry, argv, ins=None, inouts=None, outs=None, scratch=(), absent=(), before=None, state=None, hosts=None):
        self.entry, self.argv = entry, argv
        self.ins, self.inouts, self.outs = dict(ins or {}), dict(inouts or {}), dict(outs or {})
        self.scratch = set(scratch)      # outputs whose contents are bookkeeping that may depend on timing: never compared
        self.absent = set(absent)        # optional device arguments this call passes as NULL
        self.before, self.state = before, state
        self.hosts = dict(hosts or {})   # numpy arrays and ctypes structs the argv points at

    def replaced(self, **kw):
        """A copy with some of ins / inouts / outs / hosts / argv / absent / before / state exchanged."""
        c = Call(self.entry, self.argv, self.ins, self.inouts, self.outs, self.scratch, self.absent, self.before, self.state,
                 self.hosts)
        for k, v in kw.items():
            assert hasattr(c, k), k
            setattr(c, k, v)
        return c


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def params_struct(values, pattern_ptr):
    """vslam_extract_params from (max_corners, quality, min_distance, cos_a, sin_a) and the table's device address."""
    p = capi.ExtractParams()
    p.max_corners, p.quality, p.min_distance, p.cos_a, p.sin_a = values
    p.d_pattern = pattern_ptr
    return p


def marshal(call, t, hosts=None):
    """-> (argv for ctypes, {name: the host object behind each host argument, "params" and "pose" structs included}).  `t`: the
    device tensors by name (a name that is missing is passed as NULL); `hosts`: the arrays / structs to point at instead of
    the call's own."""
    hosts = call.hosts if hosts is None else hosts
    argv, live = [], {}
    for a in call.argv:
        if isinstance(a, tuple) and a[0] == "p":
            argv.append(C.c_void_p(t[a[1]].data_ptr()) if a[1] in t else C.c_void_p(0))
        elif isinstance(a, tuple) and a[0] == "h":
            h = hosts[a[1]]
            live[a[1]] = h
            argv.append(h.ctypes.data_as(C.c_void_p) if isinstance(h, np.ndarray) else C.byref(h))
        elif isinstance(a, tuple) and a[0] in ("params", "params_values"):     # the fixture's parameters, or all five given
            values = (MAXC, 0.01, 3.0, a[1], a[2]) if a[0] == "params" else a[1]
            p = params_struct(values, t["params->d_pattern"].data_ptr())
            live["params"] = p
            argv.append(C.byref(p))
        elif isinstance(a, tuple) and a[0] == "pose":
            po = capi.PoseOutputs(*(C.c_void_p(t["pose->d_" + k].data_ptr()) for k in POSE_MEMBERS))
            live["pose"] = po
            argv.append(C.byref(po))
        else:
            argv.append(a)
    return argv, live


def state_bytes(call):
    if not call.state:
        return {}
    return {"state:" + k: np.ascontiguousarray(v).view(np.uint8).copy() for k, v in call.state().items() if isinstance(v, np.ndarray)}


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
    argv, _live = marshal(call, t)
    torch.cuda.synchronize()             # the fills above, whatever stream the context runs on
    rc = getattr(ctx.lib, call.entry)(ctx.handle, *argv)
    msg = (ctx.lib.vslam_last_error(ctx.handle) or b"").decode() if rc else ""
    status = ctx.lib.vslam_ctx_synchronize(ctx.handle)
    if status == -2:     # VSLAM_ERR_HIP: nothing more is started on a device that has just faulted
        pytest.exit(f"HIP error behind {call.entry} (moved {moved} by {offset} elements): "
                    f"{(ctx.lib.vslam_last_error(ctx.handle) or b'').decode()}", returncode=3)
    assert status == 0, (call.entry, moved, offset, status)
    got = {name: _bytes(t[name]) for name in list(call.outs) + list(call.inouts) if name not in call.scratch}
    got.update(state_bytes(call))
    return rc, msg, got, check


def _same(a, b):
    return sorted(k for k in a if not np.array_equal(a[k], b[k]))


# ---------------------------------------------------------------------------------------------------------------- the fixture
class Scene:
    pass


def build_scene(ctx, seed, pattern=None, angle_deg=-1.0):
    """Everything the calls are made of, from `seed`.  Asserts that every stage has a model on both pairs; close_scene() before
    the context goes.  pattern / angle_deg: another rBRIEF table (256 x 4 int8) and keypoint angle than the reference's."""
    s = Scene()
    s.seed = seed
    dev = "cuda"
    s.ca, s.sa = synth.keypoint_rotation(angle_deg)
    s.pat = torch.from_numpy(synth.brief_pattern() if pattern is None else pattern).to(dev)
    s.Kh = _K(W, H)
    bgr_np = synth.frames_numpy(seed, PAIRS, W, H)
    s.bgr = torch.from_numpy(bgr_np).to(dev)
    s.seeds = torch.from_numpy((np.arange(PAIRS, dtype=np.uint32) + seed * 7).view(np.int32).copy()).to(dev)
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
    s.bgr132 = torch.from_numpy(synth.frames_numpy(seed, PAIRS, 132, H)).to(dev)
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
    s.colors = torch.from_numpy(np.random.default_rng(seed).integers(1, 256, (PAIRS, KP, 3), dtype=np.uint8)).to(dev)
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
    return s


def close_scene(s):
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


def map_state(pmap):
    """-> a function that reads everything resident in `pmap` (its attached world included) back to the host."""
    def state():
        v = pmap.view()
        off, fr, pt = pmap.observations()
        v.update(offsets=off.cpu().numpy(), obs_frames=fr.cpu().numpy(), obs_points=pt.cpu().numpy())
        return v
    return state


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
    seeds3 = torch.from_numpy((np.arange(FR - 1, dtype=np.uint32) + s.seed * 7).view(np.int32).copy()).cuda()
    seq = torch.stack([s.bgr[:PAIRS], s.bgr[PAIRS:]], dim=1).contiguous()          # (tracks, 2 frames, H, W, 3)
    seeds_t = s.seeds.reshape(PAIRS, 1).contiguous()
    lo, hi = torch.zeros((B,), dtype=i32, device="cuda"), s.n_map.clone()
    render_out = {"d_bgr_out": ((B, RH, 3 * RW), u8), "d_depth_out": ((B, RH, RW), f32)}
    render_tail = [Hst("h_view"), I(RW), I(RH), I(3 * RW), P("d_bgr_out"), P("d_depth_out")]

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
             [P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(B), I(K), Hst("h_K"), Fl(16.0), I(20), P("d_R"), P("d_t"), P("d_c2"),
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
        Call("vslam_extract_Rt", [P("d_F"), P("d_best"), I(B), Hst("h_K"), P("d_R"), P("d_t"), P("d_c2")],
             ins={"d_F": f["F"], "d_best": f["best"]}, outs={"d_R": ((B, 9), f32), "d_t": ((B, 3), f32), "d_c2": ((B, 12), f32)}),
        Call("vslam_triangulate",
             [P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(B), I(K), Hst("h_K"), P("d_c2"), P("d_points4d")],
             ins=dict(pose_in, d_c2=f["c2"]), outs={"d_points4d": ((B, K, 4), f32)}),
        Call("vslam_triangulate_points",
             [P("d_p1"), P("d_p2"), I(K), Hst("h_c1"), Hst("h_c2"), P("d_points4d")],
             ins={"d_p1": s.xy1[0].contiguous(), "d_p2": s.xy2[0].contiguous()}, outs={"d_points4d": ((K, 4), f32)}, hosts={"h_c1": c1, "h_c2": c2}),
        Call("vslam_reprojection_filter",
             [P("d_points4d"), P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(B), I(K), Hst("h_K"), P("d_c2"), P("d_map_point_ids"),
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
             [Hst("h_K"), P("d_map_point_ids"), Fl(4.0), ("pose",)],
             ins={"d_bgr": s.bgr, "params->d_pattern": s.pat, "d_seeds": s.seeds, "d_map_point_ids": s.ids_free},
             outs=dict(_front_outs(FR, B), **_POSE_OUTS)),
        Call("vslam_frontend_sequence", [P("d_bgr"), I(FR)] + img + [params, I(K), P("d_seeds"), I(HYP), Fl(THR)] + _FRONT_ARGS,
             ins={"d_bgr": s.bgr, "params->d_pattern": s.pat, "d_seeds": seeds3}, outs=_front_outs(FR, FR - 1)),
        Call("vslam_pack_records", [P("d_F"), P("d_best"), P("d_matches"), I(B), I(K), P("d_records")],
             ins={"d_F": f["F"], "d_best": f["best"], "d_matches": f["matches"]}, outs={"d_records": ((B, 13 + K), i32)}),
        Call("vslam_map_step",
             [s.pmap.handle, P("d_xy_last"), P("d_desc_last"), P("d_n_last"), P("d_xy_cur"), P("d_desc_cur"), P("d_nodes_cur"), P("d_n_cur"),
              P("d_matches"), P("d_best"), P("d_F"), P("d_bgr_cur")] + img + [Hst("h_K"), Fl(2.0), U32(64), Fl(4.0)],
             ins={"d_xy_last": s.xy1, "d_desc_last": s.desc1, "d_n_last": s.n1, "d_xy_cur": s.xy2, "d_desc_cur": s.desc2,
                  "d_nodes_cur": s.nodes2, "d_n_cur": s.n2, "d_matches": f["matches"], "d_best": f["best"], "d_F": f["F"],
                  "d_bgr_cur": s.bgr[PAIRS:].contiguous()},
             before=s.pmap.reset, state=map_state(s.pmap)),
        Call("vslam_track_sequences",
             [s.pmap.handle, P("d_bgr"), I(2)] + img + [params, P("d_seeds"), I(HYP), Fl(THR), Hst("h_K"), Fl(2.0), U32(64), Fl(4.0)] + _FRONT_ARGS,
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
    for c in calls:     # the host arguments every call shares: the camera matrix and the viewer
        for a in c.argv:
            if isinstance(a, tuple) and a[0] == "h" and a[1] not in c.hosts:
                c.hosts[a[1]] = {"h_K": s.Kh, "h_view": s.view}[a[1]]
    return {c.entry: c for c in calls}


# Entry points with device-pointer arguments that build_calls does not launch, and why.
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


# --------------------------------------------------------------------------------------------------------------------- DECOYS
# A decoy is a second value for an input: same shape and dtype, valid in ANY mixture with the real arguments (a kernel that
# sees one stale argument still stays inside every array), and different enough that reading it instead of the real one
# changes a compared output.  tests/test_gpu_stream_order.py leaves decoys where a kernel that runs too early would read.
#   * value-like arguments (pixels, coordinates, descriptor bits, seeds, F / R / t / c2, points, colours, queries, poses, the
#     rBRIEF table) come from a second scene: another seed, another table, another keypoint angle;
#   * index lists are the real ones permuted inside their used range, so that they index what the real counts allow;
#   * counts and structural arrays keep the real values: a count from another scene can point past what a real array holds,
#     and a k-d tree or a CSR offset row is only valid as a whole.  These are the arguments no test can be sensitive to, the
#     ONLY ones: EXEMPT lists them entry point by entry point (a name is exempt where it is a count or a structure, not
#     wherever it appears), STRUCTURAL gives each kind its reason, and the sensitivity test holds the list to exactly this
#     set.  d_sizes, the per-track point count of vslam_render_points, is a count like d_n_map and is listed with them.
STRUCTURAL = {
    "d_n1": "keypoint count of the first frames: bounds every read of d_xy1 / d_desc1",
    "d_n2": "keypoint count of the second frames",
    "d_n": "keypoint count per frame: bounds the tree walk and every per-keypoint array",
    "d_nq": "query count per frame",
    "d_n_in": "detected-corner count per frame",
    "d_n_last": "keypoint count of the last frames",
    "d_n_cur": "keypoint count of the current frames",
    "d_m": "match count per pair: the used range of d_pairs and the modulus of d_sets",
    "d_best": "winner / inlier count per pair: the used range of d_matches",
    "d_n_map": "map size per track: the used range of d_map_points and d_obs_offsets",
    "d_sizes": "map size per track: the used range of d_points and d_colors",
    "d_lo": "first row of the lifted range",
    "d_hi": "end of the lifted range",
    "d_nodes": "k-d tree: a permutation of [0, n) that is only valid as a whole",
    "d_nodes_cur": "k-d tree of the current frames",
    "d_obs_offsets": "CSR offsets into d_obs_desc: monotone rows that are only valid as a whole",
    "d_map_point_ids": "keypoint -> map point assignment: indices bounded by the real map size",
}
EXEMPT = {
    "vslam_match_knn2_ratio": {"d_n1", "d_n2"},
    "vslam_ransac_sets": {"d_m"},
    "vslam_ransac_fundamental": {"d_m"},
    "vslam_ransac_solve": {"d_m"},
    "vslam_ransac_evaluate": {"d_m"},
    "vslam_refit_fundamental": {"d_best"},
    "vslam_refine_pairs": {"d_best"},
    "vslam_kdtree_build": {"d_n"},
    "vslam_kdtree_radius": {"d_nodes", "d_n", "d_nq"},
    "vslam_kdtree_nearest": {"d_nodes", "d_n", "d_nq"},
    "vslam_kdtree_cell_table": {"d_nodes", "d_n"},
    "vslam_orb_describe": {"d_n_in"},
    "vslam_extract_Rt": {"d_best"},
    "vslam_triangulate": {"d_best"},
    "vslam_reprojection_filter": {"d_best", "d_map_point_ids"},
    "vslam_associate_map_points": {"d_n_map", "d_nodes", "d_n", "d_obs_offsets", "d_map_point_ids"},
    "vslam_match_features": {"d_n1", "d_n2"},
    "vslam_frontend_pairs_pose": {"d_map_point_ids"},
    "vslam_pack_records": {"d_best"},
    "vslam_map_step": {"d_n_last", "d_n_cur", "d_nodes_cur", "d_best"},
    "vslam_render_points": {"d_sizes"},
    "vslam_world_step": {"d_best", "d_n_last", "d_n_cur"},
    "vslam_world_lift": {"d_lo", "d_hi"},
}
INDEX_LISTS = {"d_pairs": "d_m", "d_matches": "d_best", "d_sets": "d_m"}     # list -> the argument that holds its used range
# the first candidate (found with the CPU oracle); the next ones follow if a scene has no model on both pairs
DECOY_SEED = 47
DECOY_ANGLE = 20.0
DECOY_PARAMS = (40, 0.05, 5.0)     # max_corners, quality, min_distance of the decoy vslam_extract_params


def decoy_scene(ctx, first_seed=DECOY_SEED, tries=16):
    """The second scene: the first of `tries` seeds from first_seed on that satisfies build_scene's own assertion."""
    for seed in range(first_seed, first_seed + tries):
        try:
            return build_scene(ctx, seed, pattern=synth.synthetic_pattern(seed), angle_deg=DECOY_ANGLE)
        except AssertionError as e:
            print(f"decoy scene: seed {seed} refused ({e})")
    raise AssertionError(f"no seed in [{first_seed}, {first_seed + tries}) gives a model on both pairs")


def _used(call, name):
    """Rows of index list `name` that are in use, per item."""
    src = call.ins[INDEX_LISTS[name]].cpu().numpy()
    return src[:, 3] if src.ndim == 2 else src


def _permuted(call, name):
    real = call.ins[name]
    d = real.cpu().numpy().copy()
    used = _used(call, name)
    for p, k in enumerate(used):
        k = int(k)
        if name == "d_sets":
            d[p] = (d[p] + 1) % max(k, 1)             # another 8-subset of [0, m): still distinct, still in range
        elif k > 1:
            d[p, :k, 1] = np.roll(d[p, :k, 1], 1)      # every query index meets its neighbour's train index
    return torch.from_numpy(d).to(real.device)


def host_decoy(name, real, other):
    """A decoy for host argument `name`; `other`: the same argument of the second scene's call."""
    if name == "h_K":
        return np.array([500, 0, W // 2 + 3, 0, 510, H // 2 - 2, 0, 0, 1], np.float32)
    if name == "h_view":
        return real.copy(fu=7.0, fv=9.0, point_size=1)
    if name == "h_c1":
        d = real.copy()
        d[[0, 5]], d[[2, 6]] = 500.0, (W // 2 + 3, H // 2 - 2)
        return d
    return other.copy()      # h_c2: the second scene's camera


class Decoys:
    """For one Call: `tensors` {name: decoy of every ins / inouts tensor}, `hosts` {name: decoy of every host array / struct},
    `params` (values of the decoy vslam_extract_params, or None), `same` = the names whose decoy IS the real value."""

    def __init__(self, call, other, other_scene):
        self.tensors, self.same = {}, set()
        for name, real in list(call.ins.items()) + list(call.inouts.items()):
            if name in EXEMPT.get(call.entry, ()):
                d = real.clone()
                self.same.add(name)
            elif name in INDEX_LISTS:
                d = _permuted(call, name)
            else:
                d = other.ins.get(name, other.inouts.get(name)).clone()
            assert d.shape == real.shape and d.dtype == real.dtype, (call.entry, name)
            self.tensors[name] = d
        self.hosts = {name: host_decoy(name, real, other.hosts[name]) for name, real in call.hosts.items()}
        self.params = None
        if any(isinstance(a, tuple) and a[0] == "params" for a in call.argv):
            self.params = DECOY_PARAMS + (other_scene.ca, other_scene.sa)

    def call_with(self, call, names=None, hosts=(), params=False):
        """`call` with the named device inputs (all of them when None), host arguments and extract parameters exchanged for
        their decoys: what a plain run() then computes is what a kernel that read the decoys would have."""
        names = list(self.tensors) if names is None else names
        ins = {k: (self.tensors[k] if k in names else v) for k, v in call.ins.items()}
        inouts = {k: (self.tensors[k] if k in names else v) for k, v in call.inouts.items()}
        h = {k: (self.hosts[k] if k in hosts else v) for k, v in call.hosts.items()}
        argv = call.argv
        if params:
            argv = [DecoyParams(self.params) if isinstance(a, tuple) and a[0] == "params" else a for a in argv]
        return call.replaced(ins=ins, inouts=inouts, hosts=h, argv=argv)


def DecoyParams(values):
    return ("params_values", values)


def stream_order_calls(ctx, s, resident=True):
    """build_calls(ctx, s) with the inputs exchanged that leave an argument without any effect there, so that a decoy in ANY
    argument but the EXEMPT ones shows in a compared output (close_stream_order_calls(s) before the context goes):
      * vslam_frontend_sequence gets the frames pair by pair (last 0, current 0, last 1, current 1): with all the last frames in
        front no consecutive two show the same scene, no pair has a model, and the seeds are never used;
      * vslam_render_points draws the frusta of the map's two cameras (the only use of d_pose) seen from six baselines behind
        them: the world's poses stay at the identity on a fixture whose pairs never reach min_links;
      * vslam_kdtree_cell_table's table is compared, as a sorted list of its slots (canonical(): which slot a key takes depends
        on arrival order, which keys and ranks it holds does not);
      * vslam_map_step runs on a map of four frames, and its state is read a second and a third time behind two probe steps
        that associate only at descriptor distance 0 -- against the keypoints of the current frames carrying the LAST frames'
        descriptors, then their own: a step leaves d_desc_last and d_desc_cur nowhere but in the map's observation log, which
        only the association of a later step reads (resident=False: not this one -- for a scene that only lends its tensors)."""
    calls = build_calls(ctx, s)
    c = calls["vslam_frontend_sequence"]
    order = [p + k * PAIRS for p in range(PAIRS) for k in (0, 1)]
    calls[c.entry] = c.replaced(ins=dict(c.ins, d_bgr=s.bgr[order].contiguous()))
    c = calls["vslam_render_points"]
    pose = torch.from_numpy(s.pmap_done.view()["pose"]).to(s.bgr.device)       # the map's own: frame 1 one baseline from frame 0
    view = capi.View.look_at((0.5, -1.0, -6.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0), RW, RH, ctx.lib, fu=40.0, fv=40.0, point_size=3)
    calls[c.entry] = c.replaced(ins=dict(c.ins, d_pose=pose), hosts=dict(c.hosts, h_view=view))
    c = calls["vslam_kdtree_cell_table"]
    calls[c.entry] = c.replaced(scratch=set())
    if not resident:
        return calls
    c = calls["vslam_map_step"]
    s.pmap4 = capi.PointMap(ctx, PAIRS, 4, KP, KP, 8 * KP)
    calls[c.entry] = c.replaced(argv=[s.pmap4.handle] + c.argv[1:], before=s.pmap4.reset, state=probed_map_state(s.pmap4, s))
    return calls


def close_stream_order_calls(s):
    s.pmap4.close()


def probed_map_state(pmap, s):
    f = s.fp
    matches, best = f["matches"].cpu().numpy(), f["best"].cpu().numpy()
    desc1 = s.desc1.cpu().numpy()
    carried = np.zeros_like(desc1)
    for p in range(PAIRS):
        k = int(best[p, 3])
        carried[p, matches[p, :k, 1]] = desc1[p, matches[p, :k, 0]]
    carried = torch.from_numpy(carried).to(s.desc1.device)
    last = dict(xy=s.xy1, desc=s.desc1, n=s.n1)
    bgr_cur = s.bgr[PAIRS:].contiguous()
    read = map_state(pmap)

    def state():
        v = read()
        for tag, desc in (("behind_probe_last", carried), ("behind_probe_cur", s.desc2)):
            pmap.step(last, dict(xy=s.xy2, desc=desc, nodes=s.nodes2, n=s.n2), f, bgr_cur, s.Kh, dist_threshold=1)
            v.update({tag + ":" + k: x for k, x in read().items()})
        return v
    return state


def canonical(entry, got):
    """`got` with the outputs whose layout depends on timing put into an order that does not."""
    if entry == "vslam_kdtree_cell_table" and "d_table" in got:
        slots = got["d_table"].view(np.uint32).reshape(FR, 2 * KP, 2)
        rows = [f[np.lexsort((f[:, 1], f[:, 0]))] for f in slots]
        got = dict(got, d_table=np.ascontiguousarray(np.stack(rows)).view(np.uint8).reshape(-1))
    return got


def build_decoys(calls, other_calls, other_scene):
    return {e: Decoys(c, other_calls[e], other_scene) for e, c in calls.items()}

