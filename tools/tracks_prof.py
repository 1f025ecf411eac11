#!/usr/bin/env python3
"""vslam_prof_* readings of the track triangulation (include/vslam_tracks.h) beside the cull (include/vslam_fuse.h):
triangulate_tracks_kernel and cull_points_kernel on the SAME items in the same process, `--items` items (64 and 256 by default) of
`--points` points each (4000 and 16000), `--frames` cameras, rows of 1 .. frames observations (tests/ref_tracks.random_track_item
with finite input rows, so that the cull takes the same points).  Per shape: a warm-up call of each, then `--reps` rounds that
alternate the two calls; the library's per-kernel event timing is read once and the mean per launch reported with the ratio
triangulate / cull.  The whole measurement is repeated in `--processes` fresh processes (children of this one, which never opens
the device itself) and the spread over them is reported beside the mean.  The kernel walks a row once per pass -- iterations + 4 of
them at most, where the cull walks it once -- so the ratio to expect is of that order, less what early ends and refusals save.

    python tools/tracks_prof.py [--items 64 256] [--frames 6] [--points 4000 16000] [--reps 20] [--processes 3] [--out profiles/tracks_prof.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("triangulate_tracks", "cull_points")


def child(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_tracks as rt
    from vslam_amd import Context
    ctx = Context(0)
    result = {}
    for n in a.points:
        c = rt.random_track_item(77, n, a.frames)
        nan = ~np.isfinite(c["points"][:, :3]).all(1)
        c["points"][nan, :3] = c["truth"][nan]
        for B in a.items:
            def dev(v):
                return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (B,) + np.shape(v)))).cuda()
            e = {k: dev(np.asarray(c[k])) for k in ("points", "offsets", "cam", "kp", "R", "T", "xy")}
            e.update(n=dev(np.int32(n)), n_cams=dev(np.int32(a.frames)))
            args = (e["points"], e["n"], e["offsets"], e["cam"], e["kp"], e["R"], e["T"], e["n_cams"], e["xy"], c["K"])
            ctx.prof_enable(False)
            tri, cul = ctx.triangulate_tracks(*args), ctx.cull_points(*args)      # warm-up
            ctx.synchronize()
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(a.reps):                                  # alternating: both meet the same machine
                ctx.triangulate_tracks(*args, out=tri)
                ctx.cull_points(*args, out=cul)
            ctx.synchronize()
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            ms = {k: t / cnt for k, (t, cnt) in rep.items() if k.startswith(KERNELS) and cnt > 0}
            result[f"{B}x{n}"] = dict(track_stats=tri["stats"][0].cpu().numpy().tolist(), cull_stats=cul["stats"][0].cpu().numpy().tolist(),
                                      observations=int(c["offsets"][n]), mean_ms_per_launch=ms)
    result["device"] = torch.cuda.get_device_name(0)
    ctx.close()
    print("TRACKS_PROF " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--frames", type=int, default=6)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--frames", str(a.frames), "--reps", str(a.reps), "--items"] + [
            str(i) for i in a.items] + ["--points"] + [str(p) for p in a.points]
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
        runs.append(json.loads([l for l in txt.splitlines() if l.startswith("TRACKS_PROF ")][-1][len("TRACKS_PROF "):]))
    out = dict(frames=a.frames, reps=a.reps, processes=a.processes, device=runs[0]["device"], shapes={})
    for shape, first in runs[0].items():
        if shape == "device":
            continue
        entry = dict(track_stats=first["track_stats"], cull_stats=first["cull_stats"], observations=first["observations"], ms_per_launch={})
        for kern in first["mean_ms_per_launch"]:
            vals = [r[shape]["mean_ms_per_launch"][kern] for r in runs]
            entry["ms_per_launch"][kern] = dict(mean=round(sum(vals) / len(vals), 5), min=round(min(vals), 5), max=round(max(vals), 5))
        ratios = [r[shape]["mean_ms_per_launch"]["triangulate_tracks_kernel"] / r[shape]["mean_ms_per_launch"]["cull_points_kernel"] for r in runs]
        entry["ratio_triangulate_over_cull"] = dict(mean=round(sum(ratios) / len(ratios), 2), min=round(min(ratios), 2), max=round(max(ratios), 2))
        out["shapes"][shape] = entry
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
