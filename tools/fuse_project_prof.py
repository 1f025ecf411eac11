#!/usr/bin/env python3
"""vslam_prof_* readings of the geometric fusing (include/vslam_fuse_project.h) beside the only way to get the same pairs without
it: one vslam_search_projection call per camera on the same points.  Two shapes by default: 64 items of 4000 points x 16 cameras and
16 items of 16000 points x 64 cameras, 2000 keypoint slots per camera; the items are tests/ref_fuse_project.random_item's (every
feature three times in the item, one to three observations per point).  Per shape: a warm-up call, then `--reps` timed calls; the
library's per-kernel event timing is read once and the mean per launch reported, summed over the kernels of a call (four for
vslam_fuse_project; two for each of the C searches, whose sum over the cameras is reported).  The whole measurement is repeated in
`--processes` fresh processes (children of this one, which never opens the device itself) and the spread over them is reported beside
the mean.  The fills in front of the kernels are memsets the profiler does not bracket: they are in neither figure.  The per-camera
searches try every (point, camera) pair, the seen ones too -- they have no skip rule --, so their pairs are n x C.

    python tools/fuse_project_prof.py [--shapes 64x4000x16 16x16000x64] [--keypoints 2000] [--reps 10] [--processes 3] [--out profiles/fuse_project_prof.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = "fuse_project_"
THEIRS = ("search_propose", "corr_resolve")


def child(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_fuse_project as rfp
    from vslam_amd import Context
    ctx = Context(0)
    result = {}

    def timed(call, prefixes):
        ctx.prof_enable(False)
        out = call(None)                                         # warm-up: the arena at this size
        ctx.synchronize()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            out = call(out)
        ctx.synchronize()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        return out, {k: ms / a.reps for k, (ms, cnt) in rep.items() if k.startswith(prefixes) and cnt > 0}
    for shape in a.shapes:
        B, n, C = (int(v) for v in shape.split("x"))
        c = rfp.random_item(4242, n, C, kp_stride=a.keypoints)

        def dev(v):
            return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (B,) + np.shape(v)))).cuda()
        d = {k: dev(np.asarray(c[k])) for k in ("points", "offsets", "cam", "kp", "obs_desc", "R", "T", "xy", "desc", "n_kp")}
        d.update(n=dev(np.int32(n)), n_cams=dev(np.int32(C)))
        out, ms = timed(lambda o: ctx.fuse_project(d["points"], d["n"], d["offsets"], d["cam"], d["kp"], d["obs_desc"], d["R"], d["T"], d["n_cams"],
                                                   d["xy"], d["desc"], d["n_kp"], c["K"], c["width"], c["height"], found_stride=n, out=o), OURS)
        stats = out["stats"][0].cpu().numpy().tolist()
        per_cam = [{k: d[k][:, cam].contiguous() for k in ("R", "T", "xy", "desc", "n_kp")} for cam in range(C)]

        def searches(o):
            o = o or [None] * C
            return [ctx.search_projection(d["points"], d["n"], d["offsets"], d["obs_desc"], e["R"], e["T"], c["K"], c["width"], c["height"], e["xy"],
                                          e["desc"], e["n_kp"], out=o[cam]) for cam, e in enumerate(per_cam)]
        _, base = timed(searches, THEIRS)
        result[shape] = dict(stats=stats, tried=stats[0], ms_per_call=ms, search_ms_per_c_calls=base, search_pairs=n * C)
        del d, per_cam, out
        torch.cuda.empty_cache()
    result["device"] = torch.cuda.get_device_name(0)
    ctx.close()
    print("FUSE_PROJECT_PROF " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64x4000x16", "16x16000x64"], help="items x points x cameras")
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.processes):                                 # fresh processes, one at a time
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--keypoints", str(a.keypoints), "--reps", str(a.reps), "--shapes"] + a.shapes
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
        runs.append(json.loads([l for l in txt.splitlines() if l.startswith("FUSE_PROJECT_PROF ")][-1][len("FUSE_PROJECT_PROF "):]))
    out = dict(keypoints=a.keypoints, reps=a.reps, processes=a.processes, device=runs[0]["device"], shapes={})
    for s in a.shapes:
        items = int(s.split("x")[0])
        first = runs[0][s]
        entry = dict(stats_per_item=first["stats"], tried_pairs_per_call=items * first["tried"], search_pairs_per_c_calls=items * first["search_pairs"])
        for key in ("ms_per_call", "search_ms_per_c_calls"):
            per_kernel = {}
            for kern in first[key]:
                vals = [r[s][key][kern] for r in runs]
                per_kernel[kern] = dict(mean=round(sum(vals) / len(vals), 5), min=round(min(vals), 5), max=round(max(vals), 5))
            totals = [sum(r[s][key].values()) for r in runs]
            entry[key] = dict(kernels=per_kernel, total=dict(mean=round(sum(totals) / len(totals), 5), min=round(min(totals), 5), max=round(max(totals), 5)))
        entry["ns_per_tried_pair"] = round(1e6 * entry["ms_per_call"]["total"]["mean"] / max(entry["tried_pairs_per_call"], 1), 4)
        entry["search_ns_per_pair"] = round(1e6 * entry["search_ms_per_c_calls"]["total"]["mean"] / entry["search_pairs_per_c_calls"], 4)
        out["shapes"][s] = entry
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
