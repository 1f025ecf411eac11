#!/usr/bin/env python3
"""One vslam_prof_* reading of the window adjustment (include/vslam_adjust.h): adjust_windows_kernel at `--tracks` items of
`--cams` cameras and `--points` points, every item the exact problem of tests/ref_adjust.py (seed 1, each point seen by a camera
with probability 0.75, 20 % planted outliers, the free cameras and the points perturbed).  The call is repeated `--reps` times
from the same start; the library's per-kernel event timing is read once at the end and the mean per launch is printed as one
JSON line (and written to --out).

    python tools/adjust_prof.py [--tracks 256] [--cams 8] [--points 2000] [--reps 20] [--out profiles/adjust_prof.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_adjust as ra  # noqa: E402
from vslam_amd import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pr = ra.problem(1, a.cams, a.points, seen=0.75, outliers=0.2)
    B = a.tracks

    def rep(v, dt):
        v = np.ascontiguousarray(v, dt)
        return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (B,) + v.shape))).cuda()
    start = dict(R=rep(pr["R"], np.float64), T=rep(pr["T"], np.float64), X=rep(pr["X"], np.float64))
    off, cam, xy = rep(pr["off"], np.int32), rep(pr["cam"], np.int32), rep(pr["xy"], np.float32)
    nc, n = torch.full((B,), a.cams, dtype=torch.int32).cuda(), torch.full((B,), a.points, dtype=torch.int32).cuda()
    ctx = Context(0)

    def once():
        R, T, X = (start[k].clone() for k in ("R", "T", "X"))
        return ctx.adjust_windows(R, T, nc, X, n, off, cam, xy, ra.kmat())
    st = once()[3]                                               # warm-up: the arena
    ctx.synchronize()
    st = st.cpu().numpy()[0]
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(a.reps):
        once()
    ctx.synchronize()
    report = ctx.prof_report()
    ctx.prof_enable(False)
    out = dict(tracks=B, cams=a.cams, points=a.points, observations=int(len(pr["cam"])), reps=a.reps, participants=int(st[0]),
               accepted_steps=int(st[3]), mean_rho_start=round(float(st[1]), 4), mean_rho_result=float(f"{st[2]:.4g}"),
               device=torch.cuda.get_device_name(0),
               mean_ms_per_launch={k: round(ms / max(cnt, 1), 4) for k, (ms, cnt) in report.items() if k.startswith("adjust_")},
               launches={k: cnt for k, (ms, cnt) in report.items() if k.startswith("adjust_")})
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
