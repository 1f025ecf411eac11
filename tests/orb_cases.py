"""Inputs for the grid ORB/FAST tests (tests/test_oracle_orb*.py, test_gpu_orb_grid.py): scene builders, the directed
scenes that land on the extractor's boundaries, and FAST-9/16 by brute force.

`python tests/orb_cases.py` reruns the seeded search behind COUNT_SCENES."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def fast_bruteforce(img, t):
    """FAST-9/16 from its definition: 9 contiguous circle pixels all darker than v - t or all brighter
    than v + t; score = largest t' for which that still holds; strict 3x3 non-max suppression."""
    h, w = img.shape
    g = img.astype(np.int32)
    score = np.zeros((h, w), np.int32)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            d = np.array([g[y, x] - g[y + dy, x + dx] for dx, dy in CIRCLE])
            best = -10 ** 9
            for s in range(16):
                arc = d[[(s + j) % 16 for j in range(9)]]
                best = max(best, arc.min(), (-arc).min())
            if best > t:
                score[y, x] = best - 1
    out = []
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            s = score[y, x]
            if s > 0:
                nb = score[y - 1:y + 2, x - 1:x + 2].copy()
                nb[1, 1] = -1
                if (s > nb).all():
                    out.append((x, y, s))
    return np.array(out, np.float32).reshape(-1, 3)


def photos():
    d = np.load(os.path.join(HERE, "golden", "real_v1.npz"))
    return [d["crop%d" % i] for i in range(4)]


def checker(w, h, p, lo=20, hi=200):
    yy, xx = np.mgrid[0:h, 0:w]
    c = np.where(((yy // p) + (xx // p)) % 2 == 1, hi, lo).astype(np.uint8)
    return np.repeat(c[:, :, None], 3, 2)


def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def blocks(seed, w, h):
    rng = np.random.default_rng(seed)
    g = rng.integers(100, 140, (h, w, 3), dtype=np.uint8)
    for _ in range(max(1, w * h // 300)):
        x, y = rng.integers(0, w), rng.integers(0, h)
        g[y:y + rng.integers(2, 20), x:x + rng.integers(2, 20)] = rng.integers(0, 256, 3)
    return g


def dots(n, side=448, seed=0):
    """n isolated one-pixel dots (spacing 4) of random contrast on a flat frame: each is exactly one FAST corner at both
    thresholds, so level 0's FAST list inside the border holds exactly n entries."""
    rng = np.random.default_rng(seed + n)
    g = np.full((side, side), 100, np.uint8)
    pos = np.arange(32, side - 32, 4)
    yy, xx = np.meshgrid(pos, pos, indexing="ij")
    yy, xx = yy.reshape(-1)[:n], xx.reshape(-1)[:n]
    assert len(yy) == n
    c = rng.integers(22, 100, n) * np.where(rng.random(n) < 0.5, 1, -1)
    g[yy, xx] = (100 + c).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, 2)


def scene(w, h, seed, band):
    """A synthetic frame; band = p puts a checkerboard of period p across rows [h/2 - 30, h/2 + 30), whose identical
    corners tie Harris responses at a cut."""
    from vslam_amd import synth
    bgr = synth.frames_numpy(seed, 1, w, h)[0].copy()
    if band:
        y0 = h // 2 - 30
        yy, xx = np.mgrid[0:60, 0:w]
        bgr[y0:y0 + 60] = (((yy // band + xx // band) % 2) * 150 + 50).astype(np.uint8)[:, :, None]
    return bgr


# one-cell frames whose threshold-20 count, after its own ties, is 499 (falls back to threshold 5), 500 and 501 (kept):
# (w, h, seed, band) as search_count_scene() finds them
COUNT_SCENES = {499: (380, 280, 1, 0), 500: (380, 280, 3, 0), 501: (360, 300, 1, 6)}


def count_scene(target):
    return scene(*COUNT_SCENES[target])


def search_count_scene(oracle, target, sizes=((380, 280), (360, 300)), seeds=range(1, 25), bands=(0, 6, 9, 12)):
    """The first (w, h, seed, band) in this order whose threshold-20 count is decided and equals target."""
    import ref_orb
    for band in bands:
        for w, h in sizes:
            for seed in seeds:
                gray = oracle.bgr2gray(ref_orb.outline(scene(w, h, seed, band), 1, 1))
                if ref_orb.detect(oracle.orb_pyramid(gray), 20)["count_range"] == (target, target):
                    return w, h, seed, band
    return None


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    from oracle_lib import Oracle
    o = Oracle()
    for t in sorted(COUNT_SCENES):
        print(t, search_count_scene(o, t))
