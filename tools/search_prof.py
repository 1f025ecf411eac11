#!/usr/bin/env python3
"""vslam_prof_* readings of the search by projection (include/vslam_search.h): search_propose_kernel and corr_resolve_kernel at
`--items` items of `--keypoints` keypoints in a 1280 x 720 frame, `--points` points per item (4000 and 16000 by default) with 1 to
5 observations each, radius 8, from a pose a few pixels off (tests/search_cases.random_case's construction: keypoints scattered
on the projections, descriptors from a pool so that ties, ratio rejections and contests occur).  Per shape: a warm-up call, then
`--reps` timed calls; the library's per-kernel event timing is read once and the mean per launch reported.  The whole
measurement is repeated in `--processes` fresh processes (children of this one, which never opens the device itself) and the
spread over them is reported beside the mean.

Two more readings per shape say where search_propose_kernel's time goes:
  no_candidates    the same call at radius 2^-7 px: no keypoint passes the disc test, so what is left is the grid's construction in
                   every workgroup, the projections and the walk over the cells.
  one_observation  the same points with one observation each: the descriptor loads per candidate fall to a fifth .. a third.
For scale only, assoc_candidates_kernel (vslam_associate_map_points: f32 projection, k-d walk in visit order, first acceptable
hits) on the same points and keypoints at the same radius.  The two do different work: no ratio of them is a speed-up.

    python tools/search_prof.py [--items 256] [--keypoints 2000] [--points 4000 16000] [--reps 20] [--processes 3] [--out profiles/search_prof.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, RADIUS = 1280, 720, 8.0
KERNELS = ("search_propose", "corr_resolve")


def child(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import search_cases as sc
    from vslam_amd import Context
    ctx = Context(0)
    B = a.items
    result = {}
    for n_points in a.points:
        c = sc.random_case(4242, n_points, a.keypoints, W, H, RADIUS, max_obs=5)
        c["xy"] = np.nan_to_num(c["xy"], nan=5.0)                # the k-d build of the scale reading takes finite keypoints only
        ang = 0.004                                              # a few pixels off: 0.004 rad about z, 2 .. 5 px of translation
        c["R"] = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]).reshape(9)
        c["T"] = np.array([0.01, -0.008, 0.0])
        one_obs = np.arange(n_points + 1, dtype=np.int32)       # the first observation of every point that has one
        first = np.minimum(c["offsets"][:-1], len(c["obs_desc"]) - 1)

        def dev(v):
            return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (B,) + np.shape(v)))).cuda()
        d = dict(points=dev(c["points"]), n_points=dev(np.int32(n_points)), offsets=dev(c["offsets"]), obs_desc=dev(c["obs_desc"]),
                 R=dev(c["R"]), T=dev(c["T"]), xy=dev(c["xy"]), desc=dev(c["desc"]), n_kp=dev(np.int32(a.keypoints)))
        d1 = dict(d, offsets=dev(one_obs), obs_desc=dev(c["obs_desc"][first]))
        out = None

        def search(dd, radius):
            nonlocal out
            out = ctx.search_projection(dd["points"], dd["n_points"], dd["offsets"], dd["obs_desc"], dd["R"], dd["T"], c["K"], W, H, dd["xy"],
                                        dd["desc"], dd["n_kp"], out=out, radius_px=radius)
            return out
        readings = {}
        for name, dd, radius in (("search", d, RADIUS), ("no_candidates", d, 2.0 ** -7), ("one_observation", d1, RADIUS)):
            ctx.prof_enable(False)
            search(dd, radius)                                   # warm-up: the arena at this size
            ctx.synchronize()
            stats = out["stats"][0].cpu().numpy().tolist()
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(a.reps):
                search(dd, radius)
            ctx.synchronize()
            rep = ctx.prof_report()
            readings[name] = dict(stats=stats, mean_ms_per_launch={k: ms / max(cnt, 1) for k, (ms, cnt) in rep.items() if k.startswith(KERNELS)},
                                  launches={k: cnt for k, (ms, cnt) in rep.items() if k.startswith(KERNELS)})
        # for scale: the reference-exact association's candidate kernel on the same points and keypoints
        ctx.prof_enable(False)
        nodes = ctx.kdtree_build(d["xy"], d["n_kp"])
        Km = np.asarray(c["K"], np.float64)
        c2 = (Km @ np.concatenate([c["R"].reshape(3, 3), c["T"].reshape(3, 1)], 1)).astype(np.float32).reshape(12)
        ids = torch.full((B, a.keypoints), -1, dtype=torch.int32).cuda()
        args = (d["points"], d["n_points"], dev(c2), W, H, nodes, d["xy"], d["desc"], d["n_kp"], d["offsets"], d["obs_desc"])
        ctx.associate(*args, ids.clone(), radius=RADIUS)
        ctx.synchronize()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            ctx.associate(*args, ids.clone(), radius=RADIUS)
        ctx.synchronize()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        readings["assoc_for_scale"] = dict(mean_ms_per_launch={k: ms / max(cnt, 1) for k, (ms, cnt) in rep.items() if k.startswith("assoc_")},
                                           launches={k: cnt for k, (ms, cnt) in rep.items() if k.startswith("assoc_")})
        result[str(n_points)] = readings
    result["device"] = torch.cuda.get_device_name(0)
    ctx.close()
    print("SEARCH_PROF " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--items", str(a.items), "--keypoints", str(a.keypoints), "--reps",
               str(a.reps), "--points"] + [str(p) for p in a.points]
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
        runs.append(json.loads([l for l in txt.splitlines() if l.startswith("SEARCH_PROF ")][-1][len("SEARCH_PROF "):]))
    out = dict(items=a.items, keypoints=a.keypoints, width=W, height=H, radius_px=RADIUS, reps=a.reps, processes=a.processes,
               device=runs[0]["device"], shapes={})
    for p in a.points:
        shape = {}
        for name, first in runs[0][str(p)].items():
            entry = {k: v for k, v in first.items() if k not in ("mean_ms_per_launch",)}
            entry["ms_per_launch"] = {}
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
