#!/usr/bin/env python3
"""vslam_prof_* readings of the pose without a prior (include/vslam_pnp.h), ONE reading each (one process, a warm-up call, then the
mean per launch over `--reps` calls):
  pnp     pnp_solve_kernel, pnp_count_kernel, pnp_select_kernel and the polish (resect_poses_kernel) at `--items` items of
          `--corr` correspondences, `--hypotheses` hypotheses, half of the keypoints replaced by random pixels
          (tests/ref_pnp.planted, one scene broadcast to every item with a seed of its own);
  match   match_propose_kernel and corr_resolve_kernel at `--items` items of `--points` points with 1 to 3 observations against
          `--keypoints` keypoints (tests/pnp_cases.match_case).
No target time is set; the numbers are a record to measure later work against.

    python tools/pnp_prof.py [--items 256] [--corr 2000] [--hypotheses 128] [--points 4000] [--keypoints 2000] [--reps 10] [--out profiles/pnp_prof.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pnp_cases as pc
    import ref_pnp as rp
    from vslam_amd import Context
    ctx = Context(0)
    B = a.items

    def dev(v):
        return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (B,) + np.shape(v)))).cuda()

    def timed(call, prefixes):
        ctx.prof_enable(False)
        out = call()                                             # warm-up: the arena at this size
        ctx.synchronize()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            call()
        ctx.synchronize()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        return out, {k: dict(ms_per_launch=round(ms / max(cnt, 1), 5), launches=cnt) for k, (ms, cnt) in rep.items() if k.startswith(prefixes)}
    result = dict(device=torch.cuda.get_device_name(0), readings="one reading each: one process, mean per launch over reps calls")
    sc = rp.planted(a.corr, 0.5, 7)
    d = dict(points=dev(sc["points"]), xy=dev(sc["xy"]), n=dev(np.int32(a.corr)), seeds=torch.arange(1, B + 1, dtype=torch.int32).cuda(),
             R=dev(np.zeros(9)), T=dev(np.zeros(3)))
    out = {}

    def pnp():
        out.update(ctx.pnp_ransac(d["points"], d["xy"], d["n"], sc["K"], d["seeds"], d["R"], d["T"], polish={}, out=out or None, want_stats=True,
                                  hypotheses=a.hypotheses))
        return out
    o, kern = timed(pnp, ("pnp_", "resect_poses"))
    found = int((o["winner"] >= 0).sum())
    exact = int((o["inlier"].bool().cpu() == torch.from_numpy(sc["planted"])[None, :]).all(1).sum())
    result["pnp"] = dict(items=B, correspondences=a.corr, hypotheses=a.hypotheses, outliers=0.5, found=found, planted_set_exact=exact, kernels=kern)
    c = pc.match_case(4242, a.points, (1, 3), a.keypoints)
    m = dict(points=dev(c["points"]), n_points=dev(np.int32(a.points)), offsets=dev(c["offsets"]), obs_desc=dev(c["obs_desc"]), xy=dev(c["xy"]),
             desc=dev(c["desc"]), n_kp=dev(np.int32(a.keypoints)))
    mout = {}

    def match():
        mout.update(ctx.match_points(m["points"], m["n_points"], m["offsets"], m["obs_desc"], m["xy"], m["desc"], m["n_kp"], out=mout or None))
        return mout
    o, kern = timed(match, ("match_propose", "corr_resolve"))
    result["match"] = dict(items=B, points=a.points, observations="1-3", keypoints=a.keypoints, stats=o["stats"][0].cpu().numpy().tolist(), kernels=kern)
    ctx.close()
    print("PNP_PROF " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--corr", type=int, default=2000)
    ap.add_argument("--hypotheses", type=int, default=128)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for k in ("items", "corr", "hypotheses", "points", "keypoints", "reps")
                                                                    for x in ("--" + k, str(getattr(a, k)))]
    txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout   # a fresh process that opens the device
    line = [l for l in txt.splitlines() if l.startswith("PNP_PROF ")][-1][len("PNP_PROF "):]
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
