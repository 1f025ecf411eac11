"""The Calls (tests/entry_calls.Call) of the entry points that the five newer headers declare (include/vslam_search.h, vslam_pnp.h,
vslam_resect.h, vslam_adjust.h, vslam_fuse.h), as entry_calls.build_calls has them for include/vslam_amd.h: the argument list of the C
prototype with every device tensor named as the header names it.  Each function takes the device tensors its test file already
prepares (the dicts of that file's own helpers) and only gives them their places: the stalled-stream test of each header and
tests/test_gpu_workspace.py build their calls here, so the two hold the same call.

ENTRIES lists every entry point of the five headers that takes device memory; tests/test_gpu_workspace.py holds that list to the
headers."""
import ctypes as C

import numpy as np
import torch

from entry_calls import Call, Hst, P

i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
NULL = C.c_void_p(0)

ENTRIES = ["vslam_search_projection", "vslam_map_observation_descriptors", "vslam_world_search", "vslam_pnp_ransac", "vslam_match_points",
           "vslam_world_relocalise", "vslam_resect_poses", "vslam_world_step_resect", "vslam_adjust_windows", "vslam_world_adjust",
           "vslam_fuse_points", "vslam_cull_points", "vslam_world_fuse", "vslam_world_cull", "vslam_world_observations"]


def _K9(K):
    return np.ascontiguousarray(np.asarray(K, np.float32).reshape(9)).copy()


def _ref(struct):
    return C.byref(struct) if struct is not None else NULL


# ------------------------------------------------------------------------------------------------------------ vslam_search.h
def _corr_outs(B, S, Kp, stats_dtype=i32):
    return {"d_kp_of_point": ((B, S), i32), "d_dist": ((B, S), i32), "d_corr_points": ((B, Kp, 3), f64), "d_corr_xy": ((B, Kp, 2), f32),
            "d_corr_point": ((B, Kp), i32), "d_corr_kp": ((B, Kp), i32), "d_n_corr": ((B,), i32), "d_stats": ((B, 4), stats_dtype)}


def search_projection(d, K, width, height, params=None):
    """d: points, n_points, offsets, obs_desc, R, T, xy, desc, n_kp (test_gpu_search._cuda); `params` a capi.SearchParams or None"""
    B, S, Kp, O = d["points"].shape[0], d["points"].shape[1], d["xy"].shape[1], d["obs_desc"].shape[1]
    argv = [P("d_points"), P("d_n_points"), S, P("d_obs_offsets"), P("d_obs_desc"), O, P("d_R"), P("d_T"), Hst("h_K"), width, height,
            P("d_xy"), P("d_desc"), P("d_n_kp"), Kp, NULL, B, _ref(params), P("d_kp_of_point"), P("d_dist"),
            P("d_corr_points"), P("d_corr_xy"), P("d_corr_point"), P("d_corr_kp"), P("d_n_corr"), P("d_stats")]
    return Call("vslam_search_projection", argv,
                ins={"d_points": d["points"], "d_n_points": d["n_points"], "d_obs_offsets": d["offsets"], "d_obs_desc": d["obs_desc"],
                     "d_R": d["R"], "d_T": d["T"], "d_xy": d["xy"], "d_desc": d["desc"], "d_n_kp": d["n_kp"]},
                outs=_corr_outs(B, S, Kp), hosts={"h_K": _K9(K)})


def map_observation_descriptors(pmap):
    T, M, O = pmap.tracks, pmap.map_capacity, pmap.obs_capacity
    return Call("vslam_map_observation_descriptors", [pmap.handle, P("d_offsets"), P("d_desc")],
                outs={"d_offsets": ((T, M + 1), i32), "d_desc": ((T, O, 32), u8)})


def world_search(world, pmap, cur, K, width, height, resect=None, before=None, state=None):
    """cur: xy, desc, n of the frame searched in; resect: a capi.ResectParams (the call then writes the world: give `before` and
    `state`) or None (search only)"""
    T, Kp = world.tracks, world.kp_stride
    argv = [world.handle, pmap.handle, P("d_xy_cur"), P("d_desc_cur"), P("d_n_cur"), Hst("h_K"), width, height, NULL, _ref(resect),
            P("d_corr_point"), P("d_corr_kp"), P("d_n_corr"), P("d_stats") if resect is not None else NULL]
    outs = {"d_corr_point": ((T, Kp), i32), "d_corr_kp": ((T, Kp), i32), "d_n_corr": ((T,), i32)}
    if resect is not None:
        outs["d_stats"] = ((T, 4), f64)
    return Call("vslam_world_search", argv, ins={"d_xy_cur": cur["xy"], "d_desc_cur": cur["desc"], "d_n_cur": cur["n"]}, outs=outs,
                before=before, state=state, hosts={"h_K": _K9(K)})


# --------------------------------------------------------------------------------------------------------------- vslam_pnp.h
def pnp_ransac(d, K, params, polish):
    """d: points, xy, n, seeds, R, T (test_gpu_pnp._tensors); params / polish: capi.PnpParams, capi.ResectParams or None"""
    B, S = d["points"].shape[:2]
    H = params.hypotheses
    argv = [P("d_points"), P("d_xy"), P("d_n"), B, S, Hst("h_K"), P("d_seeds"), C.byref(params), _ref(polish), P("d_R"), P("d_T"),
            P("d_inlier"), P("d_corr_points"), P("d_corr_xy"), P("d_corr_index"), P("d_n_inliers"), P("d_winner"), P("d_counts"), P("d_stats")]
    return Call("vslam_pnp_ransac", argv, ins={"d_points": d["points"], "d_xy": d["xy"], "d_n": d["n"], "d_seeds": d["seeds"]},
                inouts={"d_R": d["R"], "d_T": d["T"]},
                outs={"d_inlier": ((B, S), i32), "d_corr_points": ((B, S, 3), f64), "d_corr_xy": ((B, S, 2), f32), "d_corr_index": ((B, S), i32),
                      "d_n_inliers": ((B,), i32), "d_winner": ((B,), i32), "d_counts": ((B, H, 4), i32), "d_stats": ((B, 4), f64)},
                hosts={"h_K": _K9(K)})


def match_points(d):
    """d: points, n_points, offsets, obs_desc, xy, desc, n_kp (the arrays of test_gpu_pnp._match_batch on the device)"""
    B, S, Kp, O = d["points"].shape[0], d["points"].shape[1], d["xy"].shape[1], d["obs_desc"].shape[1]
    argv = [P("d_points"), P("d_n_points"), S, P("d_obs_offsets"), P("d_obs_desc"), O, P("d_xy"), P("d_desc"), P("d_n_kp"), Kp, NULL, B,
            NULL, P("d_kp_of_point"), P("d_dist"), P("d_corr_points"), P("d_corr_xy"), P("d_corr_point"), P("d_corr_kp"), P("d_n_corr"),
            P("d_stats")]
    return Call("vslam_match_points", argv,
                ins={"d_points": d["points"], "d_n_points": d["n_points"], "d_obs_offsets": d["offsets"], "d_obs_desc": d["obs_desc"],
                     "d_xy": d["xy"], "d_desc": d["desc"], "d_n_kp": d["n_kp"]}, outs=_corr_outs(B, S, Kp))


def world_relocalise(world, pmap, ins, K, polish, before, state):
    """ins: d_xy_cur, d_desc_cur, d_n_cur, d_seeds"""
    T, Kp = world.tracks, world.kp_stride
    argv = [world.handle, pmap.handle, P("d_xy_cur"), P("d_desc_cur"), P("d_n_cur"), Hst("h_K"), P("d_seeds"), NULL, NULL, _ref(polish),
            P("d_found"), P("d_winner"), P("d_n_inliers"), P("d_corr_point"), P("d_corr_kp"), P("d_n_corr"), P("d_stats")]
    return Call("vslam_world_relocalise", argv, ins=ins,
                outs={"d_found": ((T,), i32), "d_winner": ((T,), i32), "d_n_inliers": ((T,), i32), "d_corr_point": ((T, Kp), i32),
                      "d_corr_kp": ((T, Kp), i32), "d_n_corr": ((T,), i32), "d_stats": ((T, 4), f64)},
                before=before, state=state, hosts={"h_K": _K9(K)})


# ------------------------------------------------------------------------------------------------------------ vslam_resect.h
def resect_poses(points, xy, n, R, T, K, params=None):
    B, S = points.shape[:2]
    argv = [P("d_points"), P("d_xy"), P("d_n"), B, S, Hst("h_K"), _ref(params), P("d_R"), P("d_T"), P("d_stats")]
    return Call("vslam_resect_poses", argv, ins={"d_points": points, "d_xy": xy, "d_n": n}, inouts={"d_R": R, "d_T": T},
                outs={"d_stats": ((B, 4), f64)}, hosts={"h_K": _K9(K)})


def world_step_resect(world, b, K, before, state):
    """b: matches, best, X, R, t, n_last, n_cur, xy (test_gpu_resect._pair_batch)"""
    argv = [world.handle, P("d_matches"), P("d_best"), P("d_points4d"), P("d_R"), P("d_t"), P("d_n_last"), P("d_n_cur"), P("d_xy_cur"),
            Hst("h_K")]
    return Call("vslam_world_step_resect", argv,
                ins={"d_matches": b["matches"], "d_best": b["best"], "d_points4d": b["X"], "d_R": b["R"], "d_t": b["t"], "d_n_last": b["n_last"],
                     "d_n_cur": b["n_cur"], "d_xy_cur": b["xy"]}, before=before, state=state, hosts={"h_K": _K9(K)})


# ------------------------------------------------------------------------------------------------------------ vslam_adjust.h
def adjust_windows(b, K, params=None):
    """b: R, T, nc, X, n, off, cam, xy (test_gpu_adjust._batch)"""
    B, Cs, Ps, Os = b["R"].shape[0], b["R"].shape[1], b["X"].shape[1], b["cam"].shape[1]
    argv = [P("d_R"), P("d_T"), P("d_n_cams"), Cs, P("d_points"), P("d_n_points"), Ps, P("d_obs_offsets"), P("d_obs_cam"), P("d_obs_xy"),
            Os, B, Hst("h_K"), _ref(params), P("d_stats")]
    return Call("vslam_adjust_windows", argv,
                ins={"d_n_cams": b["nc"], "d_n_points": b["n"], "d_obs_offsets": b["off"], "d_obs_cam": b["cam"], "d_obs_xy": b["xy"]},
                inouts={"d_R": b["R"], "d_T": b["T"], "d_points": b["X"]}, outs={"d_stats": ((B, 4), f64)}, hosts={"h_K": _K9(K)})


def world_adjust(world, pmap, xy, xy_frames, K, window, before, state, params=None):
    argv = [world.handle, pmap.handle, P("d_xy"), xy_frames, Hst("h_K"), window, _ref(params), P("d_stats")]
    return Call("vslam_world_adjust", argv, ins={"d_xy": xy}, outs={"d_stats": ((world.tracks, 4), f64)}, before=before, state=state,
                hosts={"h_K": _K9(K)})


# -------------------------------------------------------------------------------------------------------------- vslam_fuse.h
def fuse_points(d, cam_stride, kp_stride):
    """d: n, offsets, cam, kp, mask as device tensors (ref_fuse.batch_fuse's arrays); a mask of None is passed as NULL"""
    B, S, O = d["offsets"].shape[0], d["offsets"].shape[1] - 1, d["cam"].shape[1]
    argv = [P("d_n_points"), S, P("d_obs_offsets"), P("d_obs_cam"), P("d_obs_kp"), O, cam_stride, kp_stride, P("d_mask"), B, P("d_fuse_to"),
            P("d_out_offsets"), P("d_out_cam"), P("d_out_kp"), P("d_out_src"), P("d_stats")]
    mask = {"d_mask": d["mask"]} if d.get("mask") is not None else {}
    return Call("vslam_fuse_points", argv,
                ins=dict({"d_n_points": d["n"], "d_obs_offsets": d["offsets"], "d_obs_cam": d["cam"], "d_obs_kp": d["kp"]}, **mask),
                outs={"d_fuse_to": ((B, S), i32), "d_out_offsets": ((B, S + 1), i32), "d_out_cam": ((B, O), i32), "d_out_kp": ((B, O), i32),
                      "d_out_src": ((B, O), i32), "d_stats": ((B, 4), i32)})


def cull_points(d, K):
    """d: points, n, offsets, cam, kp, R, T, n_cams, xy as device tensors (test_gpu_fuse._cull_batch's arrays)"""
    B, S, O, Cs, Kp = d["points"].shape[0], d["points"].shape[1], d["cam"].shape[1], d["R"].shape[1], d["xy"].shape[2]
    argv = [P("d_points"), P("d_n_points"), S, P("d_obs_offsets"), P("d_obs_cam"), P("d_obs_kp"), O, P("d_R"), P("d_T"), P("d_n_cams"), Cs,
            P("d_xy"), Kp, Hst("h_K"), B, NULL, P("d_keep"), P("d_counts"), P("d_stats")]
    return Call("vslam_cull_points", argv,
                ins={"d_points": d["points"], "d_n_points": d["n"], "d_obs_offsets": d["offsets"], "d_obs_cam": d["cam"], "d_obs_kp": d["kp"],
                     "d_R": d["R"], "d_T": d["T"], "d_n_cams": d["n_cams"], "d_xy": d["xy"]},
                outs={"d_keep": ((B, S), i32), "d_counts": ((B, S, 2), i32), "d_stats": ((B, 4), i32)}, hosts={"h_K": _K9(K)})


def world_fuse(world, pmap, before, state):
    return Call("vslam_world_fuse", [world.handle, pmap.handle, P("d_stats")], outs={"d_stats": ((world.tracks, 4), i32)}, before=before,
                state=state)


def world_cull(world, pmap, xy, xy_frames, K, before, state):
    argv = [world.handle, pmap.handle, P("d_xy"), xy_frames, Hst("h_K"), NULL, P("d_stats")]
    return Call("vslam_world_cull", argv, ins={"d_xy": xy}, outs={"d_stats": ((world.tracks, 4), i32)}, before=before, state=state,
                hosts={"h_K": _K9(K)})


def world_observations(world, pmap):
    T, M, O = pmap.tracks, pmap.map_capacity, pmap.obs_capacity
    argv = [world.handle, pmap.handle, P("d_offsets"), P("d_frame_ids"), P("d_point_ids"), P("d_desc")]
    return Call("vslam_world_observations", argv,
                outs={"d_offsets": ((T, M + 1), i32), "d_frame_ids": ((T, O), i32), "d_point_ids": ((T, O), i32), "d_desc": ((T, O, 32), u8)})
