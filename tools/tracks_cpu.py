#!/usr/bin/env python3
"""How accurate triangulating a track from all its observations is, read on the CPU reference (tests/ref_tracks.py), no GPU.  The device
is held to that reference bit for bit, so these readings are the device's.  Per seed of ref_adjust.EXACT_SEEDS, 6 true cameras and
120 points seen by every camera:
  (a) exact projections rounded to f32: every point's status and the worst |X - X_true|;
  (b) 0.5 px of keypoint noise: the median |X - X_true| of the six-view rows and of the two-view rows (c, c + 1) of
      tools/fuse_adjust_cpu.py's construction, both by the same rule.
DESIGN.md 5l carries the reading; tests/test_ref_tracks.py asserts it.

    python tools/tracks_cpu.py
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import ref_adjust as ra
import ref_tracks as rt

for seed in ra.EXACT_SEEDS:
    st, d = rt.distances(rt.from_problem(ra.problem(seed, **ra.EXACT_SHAPE, noise_px=0)))
    pr = ra.problem(seed, **ra.EXACT_SHAPE, noise_px=0.5)
    st6, d6 = rt.distances(rt.from_problem(pr))
    st2, d2 = rt.distances(rt.from_problem(pr, two_view=True))
    print(f"seed {seed}: (a) OK {int((st == rt.OK).sum())} of {len(st)}, worst |X - X_true| {np.nanmax(d):.3e}; "
          f"(b) six views: OK {int((st6 == rt.OK).sum())} of {len(st6)}, median {np.nanmedian(d6):.5f}; "
          f"two views: OK {int((st2 == rt.OK).sum())} of {len(st2)}, refined {int(np.isfinite(d2).sum())}, median {np.nanmedian(d2):.5f}", flush=True)
