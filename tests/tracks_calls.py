"""The Calls (tests/entry_calls.Call) of the entry points include/vslam_tracks.h declares, as tests/header_calls.py has them for the
five headers before it: the argument list of the C prototype with every device tensor named as the header names it."""
import ctypes as C

import torch

from entry_calls import Call, Hst, P
from header_calls import NULL, _K9, _ref

i32, f32, f64 = torch.int32, torch.float32, torch.float64

ENTRIES = ["vslam_triangulate_tracks", "vslam_world_retriangulate"]


def triangulate_tracks(d, K, params=None, in_place=False):
    """d: points, n, offsets, cam, kp, R, T, n_cams, xy as device tensors (ref_tracks.batch_tracks' arrays); `params` a capi.TrackParams or
    None; in_place: d_out_points is d_points itself (one in-out tensor under both names of the prototype)"""
    B, S, O, Cs, Kp = d["points"].shape[0], d["points"].shape[1], d["cam"].shape[1], d["R"].shape[1], d["xy"].shape[2]
    argv = [P("d_points"), P("d_n_points"), S, P("d_obs_offsets"), P("d_obs_cam"), P("d_obs_kp"), O, P("d_R"), P("d_T"), P("d_n_cams"), Cs,
            P("d_xy"), Kp, Hst("h_K"), B, _ref(params), P("d_points") if in_place else P("d_out_points"), P("d_status"), P("d_counts"),
            P("d_info"), P("d_stats")]
    ins = {"d_n_points": d["n"], "d_obs_offsets": d["offsets"], "d_obs_cam": d["cam"], "d_obs_kp": d["kp"], "d_R": d["R"], "d_T": d["T"],
           "d_n_cams": d["n_cams"], "d_xy": d["xy"]}
    outs = {"d_status": ((B, S), i32), "d_counts": ((B, S, 2), i32), "d_info": ((B, S, 3), f64), "d_stats": ((B, 4), i32)}
    if in_place:
        return Call("vslam_triangulate_tracks", argv, ins=ins, inouts={"d_points": d["points"]}, outs=outs, hosts={"h_K": _K9(K)})
    outs["d_out_points"] = ((B, S, 4), f32)
    return Call("vslam_triangulate_tracks", argv, ins=dict(ins, d_points=d["points"]), outs=outs, hosts={"h_K": _K9(K)})


def world_retriangulate(world, pmap, xy, xy_frames, K, before, state, params=None):
    T = world.tracks
    argv = [world.handle, pmap.handle, P("d_xy"), xy_frames, Hst("h_K"), _ref(params), P("d_status"), P("d_stats")]
    return Call("vslam_world_retriangulate", argv, ins={"d_xy": xy}, outs={"d_status": ((T, pmap.map_capacity), i32), "d_stats": ((T, 4), i32)},
                before=before, state=state, hosts={"h_K": _K9(K)})
