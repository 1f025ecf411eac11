#!/usr/bin/env python3
"""One vslam_prof_* reading of the resecting world step (include/vslam_resect.h): world_step_kernel and world_resect_kernel at
`--tracks` tracks of `--points` keypoints, every track the exact scene of tests/ref_resect.py (seed 1, 20 % planted outliers)
with the second pair's R turned by 1 degree and t by 8.  Frame 1 has no carry (the resection returns at once) and is not timed; frame 2
resects over about 0.8 * points links.  The two frames are repeated `--reps` times from a reset; the library's per-kernel event
timing of frame 2 is read once at the end and the mean per launch is printed as one JSON line (and written to --out).

    python tools/resect_prof.py [--tracks 256] [--points 2000] [--reps 20] [--out profiles/resect_prof.json]
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
import ref_resect as rr  # noqa: E402
from vslam_amd import Context, capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sc = rr.scene_inputs(1, points=a.points, frames=3, outliers=0.2)
    T, kp = a.tracks, a.points
    batches = []
    for p in sc["pairs"]:
        n = len(p["matches"])
        m = np.zeros((kp, 2), np.int32); X = np.zeros((kp, 4), np.float32)
        m[:n], X[:n] = p["matches"], p["X"]
        one = dict(matches=m, best=np.array([0, n, 0, n], np.int32), X=X, R=p["R"], t=p["t"], n_last=np.array(kp, np.int32),
                   n_cur=np.array(kp, np.int32), xy=p["xy_cur"])
        batches.append({k: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (T,) + np.shape(v)))).cuda() for k, v in one.items()})
    ctx = Context(0)
    world = capi.World(ctx, T, 3, kp)
    world.set_resection()

    def two_frames(timed):
        world.reset()
        for f, b in enumerate(batches):
            ctx.prof_enable(timed and f == 1)                    # only frame 2, the one that resects, is timed
            world.step(b["matches"], b["best"], b["X"], b["R"], b["t"], b["n_last"], b["n_cur"], xy_cur=b["xy"], K=rr.kmat())
    two_frames(False)                                            # warm-up: attributes, allocations
    ctx.synchronize()
    st = world.view()["resect_stats"][0, 2]
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(a.reps):
        two_frames(True)
    ctx.synchronize()
    rep = ctx.prof_report()
    ctx.prof_enable(False)
    out = dict(tracks=T, points=kp, reps=a.reps, participants=int(st[0]), accepted_steps=int(st[3]),
               device=torch.cuda.get_device_name(0),
               mean_ms_per_launch={k: round(ms / max(cnt, 1), 5) for k, (ms, cnt) in rep.items() if k.startswith("world_")},
               launches={k: cnt for k, (ms, cnt) in rep.items() if k.startswith("world_")})
    world.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
