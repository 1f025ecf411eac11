"""Inputs shared by the CPU and the GPU tests of the RANSAC stage (numpy only), so that both sides see the same points."""
import numpy as np

from vslam_amd import synth


def batch(seed0, sizes, K, W, H):
    """len(sizes) items of synth.two_view_points (65 % inliers) with K points each; item b uses sizes[b] of them, a sorted
    random subset, as matches i <-> i.  Returns xy1, xy2 (B, K, 2), pairs (B, K, 2), m (B)."""
    B = len(sizes)
    xy1 = np.zeros((B, K, 2), np.float32); xy2 = np.zeros((B, K, 2), np.float32)
    pairs = np.zeros((B, K, 2), np.int32); m = np.zeros(B, np.int32)
    for b, n in enumerate(sizes):
        p1, p2, _ = synth.two_view_points(seed0 + b, K, W, H, inlier_frac=0.65)
        xy1[b], xy2[b] = p1, p2
        rng = np.random.default_rng(seed0 * 7 + b)
        q = np.sort(rng.permutation(K)[:n])
        pairs[b, :n, 0] = q
        pairs[b, :n, 1] = q                       # correspondence i <-> i, as two_view_points builds it
        m[b] = n
    return xy1, xy2, pairs, m
