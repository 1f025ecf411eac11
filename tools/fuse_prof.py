#!/usr/bin/env python3
"""vslam_prof_* readings of the fusion and the cull (include/vslam_fuse.h): fuse_points_kernel and cull_points_kernel at `--items`
items of `--points` points each (4000 and 16000 by default).  The fusion's items are the duplicate structure the map has: chains of
1 to 5 points in which every point shares one (frame, keypoint) with the next, two observations per point, over `--frames` frames
of `--keypoints` keypoints; the cull's items are tests/ref_fuse.random_cull_item's.  Per shape: a warm-up call, then `--reps`
timed calls; the library's per-kernel event timing is read once and the mean per launch reported.  The whole measurement is
repeated in `--processes` fresh processes (children of this one, which never opens the device itself) and the spread over them
is reported beside the mean.  The fill of the cell table in front of the fusion (frames x keypoints x 4 bytes per item) is a
memset the profiler does not bracket: it is not in these figures.  Measured against nothing: the feature is new.

    python tools/fuse_prof.py [--items 64] [--frames 8] [--keypoints 2000] [--points 4000 16000] [--reps 20] [--processes 3] [--out profiles/fuse_prof.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("fuse_points", "cull_points")


def chains(seed, n, frames, keypoints):
    """n points in chains of 1 to 5: point j of a chain observes (f + j, k_j) and (f + j + 1, k_{j + 1}), every (frame, keypoint)
    used by one chain only; the points of a chain are scattered over the index range, as pairs of different steps are in the map"""
    import numpy as np
    rng = np.random.default_rng(seed)
    cam, kp = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    free = [list(rng.permutation(keypoints)) for _ in range(frames)]
    order = rng.permutation(n)
    i = 0
    while i < n:
        m = min(int(rng.integers(1, 6)), n - i, frames - 1)
        f = int(rng.integers(0, frames - m))
        ks = [free[f + j].pop() if free[f + j] else int(rng.integers(0, keypoints)) for j in range(m + 1)]
        for j in range(m):
            cam[order[i + j]], kp[order[i + j]] = (f + j, f + j + 1), (ks[j], ks[j + 1])
        i += m
    return np.arange(0, 2 * n + 1, 2, dtype=np.int32), cam.reshape(-1), kp.reshape(-1)


def child(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_fuse as rf
    from vslam_amd import Context
    ctx = Context(0)
    B = a.items
    result = {}

    def dev(v):
        return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (B,) + np.shape(v)))).cuda()

    def timed(call):
        ctx.prof_enable(False)
        out = call(None)                                         # warm-up: the arena at this size
        ctx.synchronize()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            call(out)
        ctx.synchronize()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        return out, {k: ms / cnt for k, (ms, cnt) in rep.items() if k.startswith(KERNELS) and cnt > 0}
    for n in a.points:
        off, cam, kp = chains(4242, n, a.frames, a.keypoints)
        d = dict(n=dev(np.int32(n)), off=dev(off), cam=dev(cam), kp=dev(kp))
        out, ms = timed(lambda o: ctx.fuse_points(d["n"], d["off"], d["cam"], d["kp"], a.frames, a.keypoints, out=o))
        readings = dict(fuse=dict(stats=out["stats"][0].cpu().numpy().tolist(), mean_ms_per_launch=ms))
        c = rf.random_cull_item(77, n, a.frames, kp_stride=a.keypoints)
        e = {k: dev(np.asarray(c[k])) for k in ("points", "offsets", "cam", "kp", "R", "T", "xy")}
        e.update(n=dev(np.int32(n)), n_cams=dev(np.int32(a.frames)))
        out, ms = timed(lambda o: ctx.cull_points(e["points"], e["n"], e["offsets"], e["cam"], e["kp"], e["R"], e["T"], e["n_cams"], e["xy"], c["K"], out=o))
        readings["cull"] = dict(stats=out["stats"][0].cpu().numpy().tolist(), mean_ms_per_launch=ms)
        result[str(n)] = readings
    result["device"] = torch.cuda.get_device_name(0)
    ctx.close()
    print("FUSE_PROF " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--points", type=int, nargs="+", default=[4000, 16000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.processes):                                 # fresh processes, one at a time
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--items", str(a.items), "--frames", str(a.frames), "--keypoints",
               str(a.keypoints), "--reps", str(a.reps), "--points"] + [str(p) for p in a.points]
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
        runs.append(json.loads([l for l in txt.splitlines() if l.startswith("FUSE_PROF ")][-1][len("FUSE_PROF "):]))
    out = dict(items=a.items, frames=a.frames, keypoints=a.keypoints, reps=a.reps, processes=a.processes, device=runs[0]["device"], shapes={})
    for p in a.points:
        shape = {}
        for name, first in runs[0][str(p)].items():
            entry = dict(stats=first["stats"], ms_per_launch={})
            for kern in first["mean_ms_per_launch"]:
                vals = [r[str(p)][name]["mean_ms_per_launch"][kern] for r in runs]
                entry["ms_per_launch"][kern] = dict(mean=round(sum(vals) / len(vals), 5), min=round(min(vals), 5), max=round(max(vals), 5))
            shape[name] = entry
        out["shapes"][str(p)] = shape
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
