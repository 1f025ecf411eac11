"""The Call (tests/entry_calls.Call) of vslam_graph_optimize, as tests/sim3_calls.py has them for include/vslam_sim3.h: the argument
list of the C prototype with every device tensor named as the header names it."""
import torch

from entry_calls import Call, P
from header_calls import _ref

i32, f64 = torch.int32, torch.float64

ENTRIES = ["vslam_graph_optimize"]


def optimize(d, params=None):
    """d: scale (B, S), R (B, S, 9), T (B, S, 3), fixed (B, S), n_nodes (B,), edge_ab (B, Es, 2), edge_scale (B, Es), edge_R (B, Es, 9),
    edge_T (B, Es, 3), edge_weight (B, Es, 3), n_edges (B,); params: capi.GraphParams or None"""
    B, S = d["scale"].shape
    Es = d["edge_scale"].shape[1]
    argv = [P("d_scale"), P("d_R"), P("d_T"), P("d_fixed"), P("d_n_nodes"), B, S, P("d_edge_ab"), P("d_edge_scale"), P("d_edge_R"), P("d_edge_T"),
            P("d_edge_weight"), P("d_n_edges"), Es, _ref(params), P("d_stats")]
    ins = {"d_" + k: d[k] for k in ("fixed", "n_nodes", "edge_ab", "edge_scale", "edge_R", "edge_T", "edge_weight", "n_edges")}
    return Call("vslam_graph_optimize", argv, ins=ins, inouts={"d_scale": d["scale"], "d_R": d["R"], "d_T": d["T"]},
                outs={"d_stats": ((B, 4), f64)})
