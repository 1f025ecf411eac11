#!/usr/bin/env python3
"""The reference's whole loop (src/vslam.cpp:53-270) for several short videos at once, resident on the device: every frame
extracted once, consecutive frames matched as one batch, then one map step per frame -- pose accumulation, propagation of
map_point_ids, association, triangulation, reprojection filter, new map points with their colours -- all tracks in lockstep
(vslam_track_sequences).  Only the numbers printed here leave the device.

    python examples/track_sequences.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vslam_amd import Context, capi, synth  # noqa: E402


def main():
    tracks, frames, width, height, max_corners, hyp = 4, 8, 640, 480, 1000, 512
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    cos_a, sin_a = synth.keypoint_rotation()
    K = np.array([[525.0, 0, width // 2], [0, 525.0, height // 2], [0, 0, 1]], np.float32)   # src/vslam.cpp:32
    bgr = synth.sequences_torch(7, tracks, frames, width, height, dev)
    seeds = torch.arange(tracks * (frames - 1), dtype=torch.int32, device=dev).reshape(tracks, frames - 1).contiguous()
    pmap = capi.PointMap(ctx, tracks, frames, max_corners, map_capacity=frames * max_corners, obs_capacity=4 * frames * max_corners)
    ctx.track_sequences(pmap, bgr, max_corners, cos_a, sin_a, None, seeds, hyp, 10.0, K)
    ctx.synchronize()                                    # VSLAM_ERR_CAPACITY here if a map had been too small
    v = pmap.view()
    off, _, _ = pmap.observations()
    off = off.cpu().numpy()
    for t in range(tracks):
        n = int(v["sizes"][t])
        longest = int(np.diff(off[t, :n + 1]).max()) if n else 0
        p = v["pose"][t, frames - 1].reshape(4, 4)
        print(f"track {t}: {n} map points, {int(v['n_obs'][t])} observations (longest list {longest}), "
              f"{int((v['map_point_ids'][t, frames - 1] >= 0).sum())} keypoints of the last frame tied to the map, "
              f"pose translation [{p[0, 3]:+.3f} {p[1, 3]:+.3f} {p[2, 3]:+.3f}]")
    pmap.close()
    ctx.close()


if __name__ == "__main__":
    main()
