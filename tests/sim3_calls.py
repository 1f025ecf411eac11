"""The Calls (tests/entry_calls.Call) of the entry points include/vslam_sim3.h declares that queue work on the context's stream, as
tests/header_calls.py has them for the other headers: the argument list of the C prototype with every device tensor named as the
header names it."""
import ctypes as C

import torch

from entry_calls import Call, Hst, P
from header_calls import _K9, _ref

i32, f64 = torch.int32, torch.float64

ENTRIES = ["vslam_sim3_ransac", "vslam_sim3_refine"]
_INS = ("A", "xa", "B", "xb", "n")


def ransac(d, K, params, polish):
    """d: A, xa, B, xb, n, seeds, scale, R, T (test_gpu_sim3._tensors); params / polish: capi.Sim3Params, capi.ResectParams or None"""
    Bt, S = d["A"].shape[:2]
    H = params.hypotheses
    argv = [P("d_A"), P("d_xa"), P("d_B"), P("d_xb"), P("d_n"), Bt, S, Hst("h_K"), P("d_seeds"), C.byref(params), _ref(polish),
            P("d_scale"), P("d_R"), P("d_T"), P("d_inlier"), P("d_corr_index"), P("d_n_inliers"), P("d_winner"), P("d_counts"), P("d_stats")]
    ins = {"d_" + k: d[k] for k in _INS}
    ins["d_seeds"] = d["seeds"]
    return Call("vslam_sim3_ransac", argv, ins=ins, inouts={"d_scale": d["scale"], "d_R": d["R"], "d_T": d["T"]},
                outs={"d_inlier": ((Bt, S), i32), "d_corr_index": ((Bt, S), i32), "d_n_inliers": ((Bt,), i32), "d_winner": ((Bt,), i32),
                      "d_counts": ((Bt, H), i32), "d_stats": ((Bt, 4), f64)}, hosts={"h_K": _K9(K)})


def refine(d, K, params=None):
    """d: A, xa, B, xb, n, mask, scale, R, T"""
    Bt, S = d["A"].shape[:2]
    argv = [P("d_A"), P("d_xa"), P("d_B"), P("d_xb"), P("d_n"), Bt, S, P("d_mask"), Hst("h_K"), _ref(params), P("d_scale"), P("d_R"), P("d_T"),
            P("d_stats")]
    ins = {"d_" + k: d[k] for k in _INS}
    ins["d_mask"] = d["mask"]
    return Call("vslam_sim3_refine", argv, ins=ins, inouts={"d_scale": d["scale"], "d_R": d["R"], "d_T": d["T"]},
                outs={"d_stats": ((Bt, 4), f64)}, hosts={"h_K": _K9(K)})


WORLD_ENTRIES = ["vslam_world_sim3", "vslam_world_apply_sim3"]   # built on a live map and world


def world_sim3(world, pmap, d, K, params=None, polish=None):
    """d: track_a, frame_a, track_b, frame_b, seeds (items,) i32; matches (items, kp_stride, 2), n_matches (items,) i32; xy_a, xy_b
    (items, kp_stride, 2) f32.  The call writes nothing but its outputs, so it has no state"""
    I, Kp = d["matches"].shape[:2]
    argv = [world.handle, pmap.handle, P("d_track_a"), P("d_frame_a"), P("d_track_b"), P("d_frame_b"), I, P("d_matches"), P("d_n_matches"),
            P("d_xy_a"), P("d_xy_b"), Hst("h_K"), P("d_seeds"), _ref(params), _ref(polish), P("d_scale"), P("d_R"), P("d_T"), P("d_s_w"), P("d_R_w"),
            P("d_t_w"), P("d_found"), P("d_n_corr"), P("d_n_inliers"), P("d_winner"), P("d_point_a"), P("d_point_b"), P("d_stats")]
    names = ("track_a", "frame_a", "track_b", "frame_b", "matches", "n_matches", "xy_a", "xy_b", "seeds")
    return Call("vslam_world_sim3", argv, ins={"d_" + k: d[k] for k in names},
                outs={"d_scale": ((I,), f64), "d_R": ((I, 9), f64), "d_T": ((I, 3), f64), "d_s_w": ((I,), f64), "d_R_w": ((I, 9), f64),
                      "d_t_w": ((I, 3), f64), "d_found": ((I,), i32), "d_n_corr": ((I,), i32), "d_n_inliers": ((I,), i32), "d_winner": ((I,), i32),
                      "d_point_a": ((I, Kp), i32), "d_point_b": ((I, Kp), i32), "d_stats": ((I, 4), f64)}, hosts={"h_K": _K9(K)})


def world_apply_sim3(world, pmap, tracks, d, before, state):
    """tracks: the host list; d: s (items,), R (items, 9), t (items, 3) f64, apply (items,) i32; before puts the world into the state
    the call starts from, state returns the arrays it writes"""
    import numpy as np
    h = np.ascontiguousarray(np.asarray(tracks, np.int32))
    argv = [world.handle, pmap.handle, Hst("h_track"), P("d_s"), P("d_R"), P("d_t"), P("d_apply"), len(h)]
    return Call("vslam_world_apply_sim3", argv, ins={"d_s": d["s"], "d_R": d["R"], "d_t": d["t"], "d_apply": d["apply"]}, before=before,
                state=state, hosts={"h_track": h})
