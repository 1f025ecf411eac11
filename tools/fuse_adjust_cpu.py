#!/usr/bin/env python3
"""What fusing buys the window adjustment, measured on the CPU reference (tests/ref_adjust.py), no GPU: the largest camera-centre
error after the adjustment with the map's two-view duplicates as they are, and with the same observations merged by
tests/ref_fuse.fuse_item.  One line per seed of ref_adjust.EXACT_SEEDS; DESIGN.md 5k carries the reading.

    python tools/fuse_adjust_cpu.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import ref_adjust as ra
import ref_fuse as rf
# A ref_adjust.problem scene (6 cameras, 120 points seen by every camera, 0.5 px keypoint noise, cameras 2.. turned 1 degree and
# shifted 0.02, points moved 0.05) in the map's shape: every physical point is five two-view map points, (c, c + 1) for c = 0 .. 4, each with
# its own perturbed start -- and the same observations after vslam_fuse_points' rule: one point, six observations, the survivor's start.
for seed in ra.EXACT_SEEDS:
    pr = ra.problem(seed, cams=6, points=120, seen=1.0, noise_px=0.5)
    rng = np.random.default_rng(100 + seed)
    P = 120
    off_u, cam_u, kp_u, xy_u, X_u = [0], [], [], [], []
    for i in range(P):
        o0 = pr["off"][i]
        for c in range(5):
            cam_u += [c, c + 1]; kp_u += [i, i]
            xy_u += [pr["xy"][o0 + c], pr["xy"][o0 + c + 1]]
            X_u.append(pr["X_true"][i] + 0.05 * rng.normal(size=3))
            off_u.append(len(cam_u))
    off_u, cam_u, kp_u = np.array(off_u, np.int32), np.array(cam_u, np.int32), np.array(kp_u, np.int32)
    xy_u, X_u = np.array(xy_u, np.float32), np.array(X_u)
    t0 = time.time()
    out_u = ra.adjust(pr["R"], pr["T"], X_u, off_u, cam_u, xy_u, ra.kmat(), n_fixed=2)
    r = rf.fuse_item(len(X_u), off_u, cam_u, kp_u, 6, P)
    surv = np.flatnonzero(r["fuse_to"] == np.arange(len(X_u)))
    X_f = X_u.copy(); X_f[r["fuse_to"] != np.arange(len(X_u))] = np.nan
    out_f = ra.adjust(pr["R"], pr["T"], X_f, r["out_offsets"], r["out_cam"], xy_u[r["out_src"]], ra.kmat(), n_fixed=2)
    eu = np.abs(ra.centres(out_u[0], out_u[1]) - pr["centres_true"]).max()
    ef = np.abs(ra.centres(out_f[0], out_f[1]) - pr["centres_true"]).max()
    e0 = np.abs(ra.centres(pr["R"], pr["T"]) - pr["centres_true"]).max()
    print(f"seed {seed}: start {e0:.4f}; unfused ({len(X_u)} points x 2 obs) {eu:.5f} stats {np.round(out_u[3], 3).tolist()}; fused ({len(surv)} points x 6 obs) {ef:.5f} stats {np.round(out_f[3], 3).tolist()}  [{time.time() - t0:.1f} s]", flush=True)
