#!/usr/bin/env python3
"""Where ransac_count_kernel abandons its hypotheses: a histogram of `matches seen at the exit` on the bench's data, for the
walk behind the head and (VSLAM_RANSAC_COUNT_FROM_ZERO) the walk from ranked match 0.  Experiments build only: with
VSLAM_RANSAC_COUNT_EXIT_PAYLOAD the NaN in hyp_sum of an abandoned hypothesis carries the count.  The walk behind the head is
taken twice, without ransac_prune (VSLAM_RANSAC_NO_PRUNE) and with it: "pruned" = ruled out before the count kernel with the
prune kernel and not without it.
    python tools/count_exit_hist.py [C3] [hard|easy]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vslam_amd import Context, capi, shard, synth  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "C3"
kind = sys.argv[2] if len(sys.argv) > 2 else "hard"
w, h, K, H, P = bench.WORKLOADS[wl]
P = min(P, 64)
dev = torch.device("cuda:0")
ca, sa = synth.keypoint_rotation()
seeds = torch.from_numpy(shard.pair_seeds(0x5EED0002, 0, P).view(np.int32)).to(dev)
bgr = (synth.frames_torch_hard if kind == "hard" else synth.frames_torch)(0x5EED0002, P, w, h, dev)
ctx = Context(0, lib=capi.load_library(capi.EXP_LIB_PATH))
fe = ctx.frontend_pairs(bgr, P, K, ca, sa, None, seeds, H, 10.0)
ctx.synchronize()
xy, desc, n = fe["xy"], fe["desc"], fe["n"]
# pair p = frames p, P + p: the stage's own inputs again, through the stage entry points
pairs, m = ctx.match_knn2_ratio(desc[:P].contiguous(), n[:P].contiguous(), desc[P:].contiguous(), n[P:].contiguous())
sets = ctx.ransac_sets(seeds, m, H)
os.environ["VSLAM_RANSAC_COUNT_EXIT_PAYLOAD"] = "1"
base_early = None   # never walked by the count kernel without the prune kernel
for walk in ("behind the head, no prune", "behind the head", "from zero"):
    os.environ.pop("VSLAM_RANSAC_NO_PRUNE", None)
    if walk == "behind the head, no prune":
        os.environ["VSLAM_RANSAC_NO_PRUNE"] = "1"
    if walk == "from zero":
        os.environ["VSLAM_RANSAC_COUNT_FROM_ZERO"] = "1"
    out = ctx.ransac_fundamental(xy[:P].contiguous(), xy[P:].contiguous(), pairs, m, sets, 10.0)
    ctx.synchronize()
    same = bool((out["best"].cpu().numpy()[:, :2] == fe["best"].cpu().numpy()[:, :2]).all())
    cnt = out["hyp_count"].cpu().numpy()
    pay = out["hyp_sum"].cpu().numpy().view(np.uint32) & 0x3FFFFF
    mm = m.cpu().numpy()
    gone = cnt < 0
    tot = cnt.size
    print(f"{wl} {kind}, {walk}: {P} pairs, m mean {mm.mean():.0f}, winner counts mean {out['best'].cpu().numpy()[:, 1].mean():.0f}, "
          f"stage outputs equal the front end's: {same}")
    # never walked by the count kernel: the payload is all ones, or none at all where a whole workgroup had nobody left
    early = gone & ((pay == 0x3FFFFF) | (pay == 0))
    if base_early is None:
        base_early = early
    pruned = early & ~base_early
    screen = gone & (pay == 0x3FFFFF) & ~pruned
    print(f"  counted in full {100 * (~gone).sum() / tot:.2f} %   ruled out by the screen {100 * screen.sum() / tot:.2f} %"
          f"   pruned {100 * pruned.sum() / tot:.2f} %")
    vals, c = np.unique(pay[gone & ~pruned & (pay != 0x3FFFFF)], return_counts=True)
    rest = 0.0
    for v, k in zip(vals, c):
        if 100 * k / tot >= 0.5 and v % 128 == 0:
            print(f"  abandoned after {v:5d} matches seen {100 * k / tot:6.2f} %")
        else:
            rest += 100 * k / tot
    print(f"  abandoned at the partial last block or at a rarer point {rest:.2f} %")
ctx.close()
