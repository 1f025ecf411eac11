"""The Call (tests/entry_calls.Call) of vslam_fuse_project, as tests/graph_calls.py has it for include/vslam_graph.h: the argument list
of the C prototype with every device tensor named as the header names it."""
import torch

from entry_calls import Call, Hst, P
from header_calls import _K9, _ref

i32 = torch.int32

ENTRIES = ["vslam_fuse_project"]
INS = dict(d_points="points", d_n_points="n", d_obs_offsets="offsets", d_obs_cam="cam", d_obs_kp="kp", d_obs_desc="obs_desc", d_R="R", d_T="T",
           d_n_cams="n_cams", d_xy="xy", d_desc="desc", d_n_kp="n_kp", d_cam_mask="cam_mask")
# where each device pointer may point (include/vslam_fuse_project.h, "Refusals")
ALIGN = dict(d_points=16, d_n_points=4, d_obs_offsets=4, d_obs_cam=4, d_obs_kp=4, d_obs_desc=16, d_R=8, d_T=8, d_n_cams=4, d_xy=8, d_desc=16, d_n_kp=4,
             d_cam_mask=4, d_found_point=4, d_found_cam=4, d_found_kp=4, d_found_dist=4, d_found_holder=4, d_n_found=4, d_stats=4)
OPTIONAL = ("d_cam_mask", "d_stats")


def fuse_project(d, K, width, height, found_stride, params=None):
    """d: ref_fuse_project.batch_of()'s arrays as cuda tensors (points (B, S, 4), offsets (B, S + 1), cam / kp (B, O), obs_desc (B, O, 32), R
    (B, Cs, 9), T (B, Cs, 3), n / n_cams (B,), xy (B, Cs, Kp, 2), desc (B, Cs, Kp, 32), n_kp / cam_mask (B, Cs)); params: capi.SearchParams or
    None"""
    B, S = d["points"].shape[:2]
    O, Cs, Kp = d["cam"].shape[1], d["R"].shape[1], d["xy"].shape[2]
    argv = [P("d_points"), P("d_n_points"), S, P("d_obs_offsets"), P("d_obs_cam"), P("d_obs_kp"), P("d_obs_desc"), O, P("d_R"), P("d_T"),
            P("d_n_cams"), Cs, P("d_xy"), P("d_desc"), P("d_n_kp"), Kp, P("d_cam_mask"), Hst("h_K"), width, height, B, _ref(params),
            P("d_found_point"), P("d_found_cam"), P("d_found_kp"), P("d_found_dist"), P("d_found_holder"), found_stride, P("d_n_found"), P("d_stats")]
    outs = {"d_" + k: ((B, found_stride), i32) for k in ("found_point", "found_cam", "found_kp", "found_dist", "found_holder")}
    outs.update(d_n_found=((B,), i32), d_stats=((B, 6), i32))
    return Call("vslam_fuse_project", argv, ins={name: d[key] for name, key in INS.items()}, outs=outs, hosts={"h_K": _K9(K)})
