"""What the tests of vslam_graph_optimize share: the serial program (tests/native/graph_serial.cpp) built once with the sanitizers
and run over a list of items, the shapes and the hand cases, and each item's reference result computed once per process.  An item is
ref_graph.pack()'s dict; `prm` holds the vslam_graph_params fields it runs under.  SHAPES and the hand cases are consistent graphs
under unit weights (the minimum costs 0); LOOP_CASES are the weighted ones whose loops disagree, each under a fixed flow and some
run to convergence, with the checks both regimes share (hold_flow, hold_converged, same_under_scaled_weights)."""
import os
import struct
import subprocess

import numpy as np

import ref_graph as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# N, E, the seed, nodes held besides node 0 (ref_graph.consistent's fixed_every): a chain plus E - (N - 1) loops each.  One free node;
# 255 / 256 / 257 around the 256 lanes; 1025 = several strided passes.  The long chains are held every 32 nodes so that the conjugate
# gradient stays short; the seeds are ones under which neither iteration runs into its cap (test_ref_graph.py asserts that).
SHAPES = [(2, 1, 0, None), (3, 3, 0, None), (5, 6, 0, None), (64, 66, 0, None), (255, 255, 0, 32), (256, 257, 0, 32), (257, 260, 0, 32),
          (1025, 1028, 2, 32)]
SHAPE_PRM = dict(max_iterations=64, cg_iterations=2048, cg_tolerance=1e-8)


def build_serial(tmpdir):
    out = os.path.join(str(tmpdir), "graph_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "graph_serial.cpp")], check=True)
    return out


def run_serial(exe, tmpdir, items):
    src, dst = os.path.join(str(tmpdir), "graph_in.bin"), os.path.join(str(tmpdir), "graph_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(items)))
        for it in items:
            p = rg.params(**it.get("prm", {}))
            S, Es = len(it["scale"]), len(it["zs"])
            f.write(struct.pack("6i", S, Es, int(it["n_nodes"]), int(it["n_edges"]), p["max_iterations"], p["cg_iterations"]))
            f.write(struct.pack("d", p["cg_tolerance"]))
            for a, dt in ((it["scale"], np.float64), (it["R"], np.float64), (it["T"], np.float64), (it["fixed"], np.int32), (it["ab"], np.int32),
                          (it["zs"], np.float64), (it["zR"], np.float64), (it["zt"], np.float64), (it["zw"], np.float64)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
    subprocess.run([exe, src, dst], check=True)
    buf = open(dst, "rb").read()
    pos, out = 0, []

    def take(n, dt):
        nonlocal pos
        a = np.frombuffer(buf, dt, n, pos)
        pos += a.nbytes
        return a
    for it in items:
        S = len(it["scale"])
        out.append(dict(scale=take(S, np.float64), R=take(9 * S, np.float64).reshape(S, 9), T=take(3 * S, np.float64).reshape(S, 3),
                        stats=take(4, np.float64), cg=int(take(1, np.int32)[0])))
    assert pos == len(buf)
    return out


_REF = {}


def reference(it):
    """ref_graph.optimize on the item, once per process -> dict(scale, R, T, stats, info)"""
    key = id(it)
    if key not in _REF:
        s, R, T, stats, info = rg.optimize(*rg.args(it), **it.get("prm", {}))
        _REF[key] = (it, dict(scale=s, R=R, T=T, stats=stats, info=info))
    return _REF[key][1]


_SHAPES = {}


def shape_item(k, node_stride=None, edge_stride=None):
    """SHAPES[k] as an item (made once per process and stride)"""
    key = (k, node_stride, edge_stride)
    if key not in _SHAPES:
        N, E, seed, every = SHAPES[k]
        it, truth = rg.consistent(N, E - (N - 1), seed, node_stride, edge_stride, fixed_every=every)
        it["prm"] = dict(SHAPE_PRM)
        it["truth"] = truth
        _SHAPES[key] = it
    return _SHAPES[key]


# ------------------------------------------------------------------------------------------------ loops that disagree, weights that differ
# name -> the fixed-flow fields over ref_graph.FLOW.  Every item has per-edge, per-group weights from [0.25, 4] and a minimum with
# cost > 0.  cg_iterations is small enough that the conjugate gradient is cut far above its floor (test_ref_graph.py asserts
# rho' / rho_0 >= FLOW_RATIO at every exit): 10 on the short chains, 5 on the pieces of 32; 2 where the edges meet one hub, which
# block-Jacobi nearly solves.
LOOP_CASES = [("drift16", dict(max_iterations=3, cg_iterations=10)),     # drifting(16) and a loop 8 -> 1
              ("drift48", dict(max_iterations=3, cg_iterations=10)),     # drifting(48) and a loop 24 -> 1; ONE zero weight
              ("hub", dict(max_iterations=3, cg_iterations=2)),          # 8 nodes, 600 edges at free node 1: three fill chunks, multi-edges
              ("hub257", dict(max_iterations=2, cg_iterations=2)),       # 3 nodes, 257 edges: one edge in the second chunk
              ("star300", dict(max_iterations=2, cg_iterations=2)),      # hub 299, 600 + 100 edges, leaves without an edge: sums over inactive nodes
              ("capacity", dict(max_iterations=2, cg_iterations=5)),     # VSLAM_GRAPH_MAX_NODES x VSLAM_GRAPH_MAX_EDGES, every measurement moved
              ("both_caps", dict(max_iterations=1, cg_iterations=1))]    # drift16: one solve of one iteration
CONVERGED_CASES = ["drift16", "drift48", "hub"]
DRIFT_LOOPS = {"drift16": 16, "drift48": 48, "both_caps": 16}
ZERO_WEIGHT = ("drift48", (24, 1))   # w_t of the edge 24 -> 25: both nodes have other edges
# Factors that every weight of an item may take without a bit of the result changing.  EVEN powers of two: the preconditioner's
# Cholesky factor scales by the factor's square root, which is exact for 4 and 2^-4 and is not for 2^-3 (under 2^-3 the serial walk
# of drift16 ends some last places away, as it must).
WEIGHT_SCALES = (4.0, 2.0 ** -4)
_LOOPS = {}


def _loop_base(name):
    if name in DRIFT_LOOPS:
        N = DRIFT_LOOPS[name]
        it, truth = rg.weighted_drift(N, 0)
        if name == ZERO_WEIGHT[0]:
            it["zw"][ZERO_WEIGHT[1]] = 0.0
    elif name == "hub":
        it, truth = rg.star(8, 1, 600, 0, [0, 2, 3, 4, 5, 6, 7])
        it = rg.weighted(it, 8)
    elif name == "hub257":
        it, truth = rg.star(3, 1, 257, 0, [0, 2])
        it = rg.weighted(it, 3)
    elif name == "star300":
        it, truth = rg.star(300, 299, 700, 0, [i for i in range(299) if i % 7 != 3], ring=100)
        it = rg.weighted(it, 300)
    elif name == "capacity":
        it, truth = rg.consistent(rg.MAX_NODES, rg.MAX_EDGES - (rg.MAX_NODES - 1), 0, fixed_every=32)
        it = rg.weighted(rg.perturbed(it, 0), 4096)
    else:
        raise KeyError(name)
    it["truth"] = truth
    return it


def loop_item(name, regime="flow"):
    """a LOOP_CASES item under its fixed flow ("flow") or run to convergence ("converged"), made once per process; both regimes
    share the arrays"""
    if name not in _LOOPS:
        _LOOPS[name] = {"base": _loop_base(name)}
    if regime not in _LOOPS[name]:
        prm = dict(rg.FLOW, **dict(LOOP_CASES)[name]) if regime == "flow" else dict(rg.CONVERGED)
        _LOOPS[name][regime] = dict(_LOOPS[name]["base"], prm=prm, name=f"{name} {regime}")
    return _LOOPS[name][regime]


def scaled(it, factor):
    """the item with every weight multiplied by `factor`"""
    out = dict(it)
    out["zw"] = it["zw"] * factor
    return out


def hold_flow(name, got, it, against=None):
    """a fixed-flow result against the item's reference (and `against`): the integers exact -- usable edges, accepted steps ==
    max_iterations, the written set --, the nodes and statistics 1 .. 2 within 16 x DELTA_FLOW -> the distance"""
    ref = reference(it)
    assert ref["info"]["moved"], name
    assert got["stats"][0] == ref["stats"][0], (name, got["stats"][0], ref["stats"][0])
    assert got["stats"][3] == ref["stats"][3] == it["prm"]["max_iterations"], (name, got["stats"][3])
    w = written(got, it)
    assert np.array_equal(w, ref["info"]["written"]), (name, np.flatnonzero(w != ref["info"]["written"]))
    d = 0.0
    for other in (ref,) + ((against,) if against is not None else ()):
        d = max(d, rg.distance((got["scale"], got["R"], got["T"]), (other["scale"], other["R"], other["T"]), ref["info"]["written"]))
        d = max(d, float(np.abs(got["stats"][1:3] / other["stats"][1:3] - 1.0).max()))
    print(f"{name}: {d:.3e} (bound {16 * rg.DELTA_FLOW:.3e}), cost {got['stats'][1]:.6e} -> {got['stats'][2]:.6e}")
    assert d <= 16 * rg.DELTA_FLOW, (name, d)
    return d


def hold_converged(name, got, it, against=None):
    """a converged result against the item's reference (and `against`): usable edges and the written set exact, the final cost
    within 16 x CONVERGED_COST relative, the nodes within 16 x CONVERGED_NODES -> (the distance, the cost's relative difference)"""
    ref = reference(it)
    assert ref["info"]["moved"], name
    assert got["stats"][0] == ref["stats"][0], name
    w = written(got, it)
    assert np.array_equal(w, ref["info"]["written"]), (name, np.flatnonzero(w != ref["info"]["written"]))
    assert got["stats"][3] >= 1 and got["stats"][2] < got["stats"][1], name
    d = c = 0.0
    for other in (ref,) + ((against,) if against is not None else ()):
        d = max(d, rg.distance((got["scale"], got["R"], got["T"]), (other["scale"], other["R"], other["T"]), ref["info"]["written"]))
        c = max(c, abs(float(got["stats"][2] / other["stats"][2]) - 1.0), abs(float(got["stats"][1] / other["stats"][1]) - 1.0))
    print(f"{name}: nodes {d:.3e} (bound {16 * rg.CONVERGED_NODES:.3e}), cost {c:.3e} relative (bound {16 * rg.CONVERGED_COST:.3e}), "
          f"{int(got['stats'][3])} steps")
    assert d <= 16 * rg.CONVERGED_NODES and c <= 16 * rg.CONVERGED_COST, (name, d, c)
    return d, c


def same_under_scaled_weights(name, one, got, factor):
    """`got` ran the item of `one` with every weight times `factor`, a power of two"""
    for k in ("scale", "R", "T"):
        assert same_bits(one[k], got[k]), (name, factor, k)
    assert got["stats"][0] == one["stats"][0] and got["stats"][3] == one["stats"][3], (name, factor)
    assert same_bits(got["stats"][1:3], one["stats"][1:3] * factor), (name, factor, got["stats"].tolist(), one["stats"].tolist())


def drift_ratio(got, it):
    """(centre error after) / (centre error before) of a drift item"""
    return rg.centre_error(got["T"], it["truth"]) / rg.centre_error(it["T"], it["truth"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def written(got, it):
    """the nodes (rows below the stride) a result changed a bit of"""
    return np.array([not (same_bits(got["scale"][i], np.float64(it["scale"][i])) and same_bits(got["R"][i], it["R"][i])
                          and same_bits(got["T"][i], it["T"][i])) for i in range(len(it["scale"]))])


def hold(name, got, it, bound, against=None):
    """a result (the serial walk's or the device's) against the item's reference: stats[0] and the written set exact (every other
    node and the padding keep the caller's bits), the written nodes and statistics 1 .. 2 within `bound`"""
    ref = reference(it)
    assert got["stats"][0] == ref["stats"][0], name
    w = written(got, it)
    assert np.array_equal(w, ref["info"]["written"]), (name, np.flatnonzero(w != ref["info"]["written"]))
    if not ref["info"]["moved"]:
        assert np.isnan(got["stats"][1:]).all(), name
        return 0.0
    assert got["stats"][3] >= 1, name
    d = rg.distance((got["scale"], got["R"], got["T"]), (ref["scale"], ref["R"], ref["T"]), ref["info"]["written"])
    if against is not None:
        d = max(d, rg.distance((got["scale"], got["R"], got["T"]), (against["scale"], against["R"], against["T"]), ref["info"]["written"]))
    print(f"{name}: {d:.3e} (bound {bound:.3e})")
    assert d <= bound, (name, d)
    return d


def hand_cases():
    """name -> (item, moved expected, usable edges expected): every left-alone rule and every unusable-edge rule"""
    out = {}

    def base(**kw):
        it, _ = rg.consistent(5, 2, 7, node_stride=7, edge_stride=9)
        it = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in it.items()}
        it["prm"] = dict(SHAPE_PRM)
        it.update(kw)
        return it
    out["plain"] = (base(), True, 6)
    out["n_nodes_zero"] = (base(n_nodes=0), False, 0)
    out["n_nodes_past_stride"] = (base(n_nodes=8), False, 0)
    out["n_edges_negative"] = (base(n_edges=-1), False, 0)
    out["n_edges_past_stride"] = (base(n_edges=10), False, 0)
    for name, key, idx, val in (("nan_scale", "scale", 2, np.nan), ("zero_scale", "scale", 3, 0.0), ("negative_scale", "scale", 1, -1.0),
                                ("inf_R", "R", (4, 3), np.inf), ("nan_T", "T", (0, 1), np.nan)):
        it = base()
        it[key][idx] = val
        out[name] = (it, False, 6)
    it = base()
    it["fixed"][:] = 0
    out["no_fixed_node"] = (it, False, 6)
    it = base()
    it["fixed"][:5] = 1
    out["all_fixed"] = (it, False, 0)
    out["no_edges"] = (base(n_edges=0), False, 0)
    # cost exactly 0 under the start (identity rotations, unit scales, integer centres): the gradient is zero, p . q is not > 0
    nodes = [(1.0, np.eye(3), np.array([float(i), 0.0, 2.0 * i])) for i in range(4)]
    edges = [(i, i + 1, rg.relative(nodes[i], nodes[i + 1])) for i in range(3)] + [(3, 0, rg.relative(nodes[3], nodes[0]))]
    out["no_accepted_step"] = (dict(rg.pack(nodes, edges, [0], node_stride=6, edge_stride=5), prm=dict(SHAPE_PRM)), False, 4)
    # unusable edges: each rule on edge 4 or 5 (the two loops), the chain keeps the graph connected
    for name, key, idx, val in (("edge_a_negative", "ab", (4, 0), -1), ("edge_b_past_n", "ab", (5, 1), 5), ("edge_a_equals_b", "ab", (4, 1), None),
                                ("edge_nan_scale", "zs", 4, np.nan), ("edge_zero_scale", "zs", 5, 0.0), ("edge_inf_R", "zR", (4, 8), np.inf),
                                ("edge_nan_t", "zt", (5, 0), np.nan), ("edge_negative_weight", "zw", (4, 1), -1.0),
                                ("edge_nan_weight", "zw", (5, 2), np.nan)):
        it = base()
        it[key][idx] = it["ab"][4, 0] if val is None else val
        out[name] = (it, True, 5)
    it = base()
    it["fixed"][1] = 1   # edge 0 joins two fixed nodes
    out["edge_both_fixed"] = (it, True, 5)
    it = base()
    it["zw"][4] = 0.0    # a zero weight is usable
    out["edge_zero_weight"] = (it, True, 6)
    it = base()
    it["ab"][3] = (-1, -1)   # node 4 loses its chain edge; its loop edges may still hold it
    out["chain_cut"] = (it, True, 5)
    it = base(n_nodes=6)     # a free node without an edge: finite, not written
    it["scale"][5], it["R"][5], it["T"][5] = 1.5, np.eye(3).reshape(9) * 1.001, (1.0, 2.0, 3.0)
    out["isolated_free_node"] = (it, True, 6)
    return out
