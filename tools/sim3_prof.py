#!/usr/bin/env python3
"""vslam_prof_* readings of the similarity between two views (include/vslam_sim3.h) and, in the same visit, of the pose without a
prior (include/vslam_pnp.h) at the same sizes.  `--readings` readings (default 3), each a fresh process: a warm-up call, then the
mean per launch over `--reps` calls.
  sim3    sim3_solve_kernel, sim3_count_kernel, sim3_select_kernel and sim3_refine_kernel at `--items` items of `--corr`
          correspondences, `--hypotheses` hypotheses, half of the pairs planted outliers (tests/ref_sim3.planted, one scene broadcast
          to every item with a seed of its own);
  pnp     pnp_solve_kernel, pnp_count_kernel, pnp_select_kernel and the polish at the same sizes (tests/ref_pnp.planted).
The count's time is reported per (model x correspondence x direction) -- a hypothesis has one model, counted in two directions
-- against pnp's per (pose slot x correspondence): four pose slots per hypothesis, whether they hold a pose or not.  A number for
the record, not a pass condition.

    python tools/sim3_prof.py [--items 256] [--corr 2000] [--hypotheses 128] [--reps 10] [--readings 3] [--out profiles/sim3_prof.json]
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
    import ref_pnp as rp
    import ref_sim3 as r3
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
    result = dict(device=torch.cuda.get_device_name(0))
    seeds = torch.arange(1, B + 1, dtype=torch.int32).cuda()
    sc = r3.planted(a.corr, 0.5, 7)
    d = dict(A=dev(sc["A"]), xa=dev(sc["xa"]), B=dev(sc["B"]), xb=dev(sc["xb"]), n=dev(np.int32(a.corr)))
    out = {}

    def sim3():
        s, R, T = dev(np.float64(1.0)), dev(np.zeros(9)), dev(np.zeros(3))
        out.update(ctx.sim3_ransac(d["A"], d["xa"], d["B"], d["xb"], d["n"], sc["K"], seeds, s, R, T, polish={}, out=out or None,
                                   want_counts=True, hypotheses=a.hypotheses))
        return out
    o, kern = timed(sim3, ("sim3_",))
    models = int((o["counts"] >= 0).sum()) // B
    result["sim3"] = dict(items=B, correspondences=a.corr, hypotheses=a.hypotheses, outliers=0.5, found=int((o["winner"] >= 0).sum()),
                          planted_set_exact=int((o["inlier"].bool().cpu() == torch.from_numpy(sc["planted"])[None, :]).all(1).sum()),
                          models_kept_per_item=models, kernels=kern)
    ps_count = kern["sim3_count_kernel"]["ms_per_launch"] * 1e9 / (B * a.hypotheses * a.corr * 2)
    sp = rp.planted(a.corr, 0.5, 7)
    p = dict(points=dev(sp["points"]), xy=dev(sp["xy"]), n=dev(np.int32(a.corr)), R=dev(np.zeros(9)), T=dev(np.zeros(3)))
    pout = {}

    def pnp():
        pout.update(ctx.pnp_ransac(p["points"], p["xy"], p["n"], sp["K"], seeds, p["R"], p["T"], polish={}, out=pout or None, want_counts=True,
                                   hypotheses=a.hypotheses))
        return pout
    o, kern = timed(pnp, ("pnp_", "resect_poses"))
    result["pnp"] = dict(items=B, correspondences=a.corr, hypotheses=a.hypotheses, outliers=0.5, found=int((o["winner"] >= 0).sum()),
                         poses_per_item=int((o["counts"] >= 0).sum()) // B, kernels=kern)
    ps_pnp = kern["pnp_count_kernel"]["ms_per_launch"] * 1e9 / (B * a.hypotheses * 4 * a.corr)
    result["count_ps"] = dict(sim3_per_model_correspondence_direction=round(ps_count, 3), pnp_per_pose_slot_correspondence=round(ps_pnp, 3))
    ctx.close()
    print("SIM3_PROF " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--corr", type=int, default=2000)
    ap.add_argument("--hypotheses", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--readings", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for k in ("items", "corr", "hypotheses", "reps")
                                                                    for x in ("--" + k, str(getattr(a, k)))]
    readings = []
    for _ in range(a.readings):   # a fresh process that opens the device, one after the other; a failure ends the visit
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
        readings.append(json.loads([l for l in txt.splitlines() if l.startswith("SIM3_PROF ")][-1][len("SIM3_PROF "):]))
    line = json.dumps(dict(readings_taken=len(readings), readings=readings))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
