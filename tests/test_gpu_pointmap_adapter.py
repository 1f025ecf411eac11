"""include/vslam/PointMap.h, the reference's PointMap surface over a one-track device map: tests/native/pointmap_demo.cpp runs
the reference's loop through it (extract_features, match_features, vslam::map_step per frame), and what sync_to_host() leaves
in the struct's vectors is held to tests/ref_map.py, bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_map
from vslam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pointmap_adapter_sync_to_host_matches_model(oracle, tmp_path):
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path / "pointmap_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "pointmap_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    w, h, maxc, hyp, frames = 320, 240, 400, 256, 5
    bgr = synth.sequences_numpy(2, 1, frames, w, h)[0]
    seeds = (np.arange(frames - 1, dtype=np.uint32) * 7919 + 5).astype(np.uint32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("5i", w, h, maxc, hyp, frames))
        f.write(seeds.tobytes())
        f.write(bgr.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    off = 0

    def take(dtype, n):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=n, offset=off)
        off += a.nbytes
        return a

    K = np.array([[525, 0, w // 2], [0, 525, h // 2], [0, 0, 1]], np.float32)
    ca, sa = synth.keypoint_rotation()
    m = ref_map.run_track(oracle, bgr, seeds, K, maxc, ca, sa, synth.brief_pattern(), hyp, 10.0)
    assert m.stats["association_claims"] >= 1 and m.stats["propagation_pushes"] >= 1 and m.size > 50
    size = int(take(np.int32, 1)[0])
    assert size == m.size
    pts = take(np.float32, 4 * size).reshape(size, 4)
    assert np.array_equal(pts.view(np.uint32), m.points[:size].view(np.uint32))
    assert np.array_equal(take(np.uint8, 3 * size).reshape(size, 3), np.array(m.colors, np.uint8).reshape(-1, 3))
    for i in range(size):
        k = int(take(np.int32, 1)[0])
        obs = take(np.int32, 2 * k).reshape(k, 2)
        assert list(obs[:, 0]) == m.frame_ids[i] and list(obs[:, 1]) == m.frame_point_ids[i], i
    for f in range(frames):
        fr = m.frames[f]
        n = int(take(np.int32, 1)[0])
        assert n == len(fr.points)
        assert np.array_equal(take(np.int32, n), fr.map_point_ids[:n]), f
        assert np.array_equal(take(np.float32, 16).view(np.uint32), fr.R_t.reshape(16).view(np.uint32)), f
        assert np.array_equal(take(np.float32, 16).view(np.uint32), fr.pose.reshape(16).view(np.uint32)), f
    dist = take(np.int32, size)
    assert [int(d) for d in dist] == [m.orb_distance(i, m.frames[-1], 0) for i in range(size)]
    assert int(take(np.int32, 1)[0]) == 1          # add_reprojection_inliers on the host-side members
    assert off == len(buf)
