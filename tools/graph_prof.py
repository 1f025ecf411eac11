#!/usr/bin/env python3
"""vslam_prof_* readings of vslam_graph_optimize (include/vslam_graph.h): `--items` graphs (default 256) of `--nodes` nodes (default
256) on a drifting circular track (tests/ref_graph.drifting, a seed per item) with 4 loop edges each.
  whole   the call under the default parameters: ms per call, and the statistics of item 0;
  cg      ms per conjugate-gradient iteration: the difference between two calls that take exactly 64 and 576 iterations (one outer
          iteration, a tolerance no residual reaches), divided by 512 -- every iteration is an edge pass, two node passes, two
          reductions and a node pass, for all items at once.
A number for the record, not a pass condition: nothing comparable ran before this call existed.

    python tools/graph_prof.py [--items 256] [--nodes 256] [--reps 5] [--out profiles/graph_prof.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_graph as rg
    from vslam_amd import Context
    ctx = Context(0)
    N = a.nodes
    extra = [(3 * N // 4, N // 4), (N // 2, 0), (N - 2, N // 3)]
    items = [rg.drifting(N, seed, extra)[0] for seed in range(a.items)]
    keys = ("scale", "R", "T", "fixed", "n_nodes", "ab", "zs", "zR", "zt", "zw", "n_edges")
    host = {k: np.stack([np.asarray(it[k]) for it in items]) for k in keys}
    host["n_nodes"], host["n_edges"] = host["n_nodes"].astype(np.int32), host["n_edges"].astype(np.int32)
    fixed = {k: torch.from_numpy(np.ascontiguousarray(host[k])).cuda() for k in keys[3:]}

    def timed(**prm):
        def call():
            io = [torch.from_numpy(np.ascontiguousarray(host[k])).cuda() for k in keys[:3]]
            return ctx.graph_optimize(*io, *(fixed[k] for k in keys[3:]), **prm)[3]
        ctx.prof_enable(False)
        call()                                                   # warm-up: the arena at this size
        ctx.synchronize()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            stats = call()
        ctx.synchronize()
        ms, cnt = ctx.prof_report()["graph_optimize_kernel"]
        ctx.prof_enable(False)
        return ms / max(cnt, 1), stats.cpu().numpy()
    whole, stats = timed()
    short, _ = timed(max_iterations=1, cg_iterations=64, cg_tolerance=1e-300)
    long, _ = timed(max_iterations=1, cg_iterations=576, cg_tolerance=1e-300)
    result = dict(device=torch.cuda.get_device_name(0), items=a.items, nodes=N, edges=int(host["n_edges"][0]), reps=a.reps,
                  ms_per_call=round(whole, 3), ms_per_cg_iteration=round((long - short) / 512.0, 6),
                  ms_64_iterations=round(short, 3), ms_576_iterations=round(long, 3),
                  item0=dict(usable_edges=int(stats[0, 0]), cost_start=float(stats[0, 1]), cost_result=float(stats[0, 2]), accepted=int(stats[0, 3])),
                  moved=int((~np.isnan(stats[:, 3])).sum()))
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
