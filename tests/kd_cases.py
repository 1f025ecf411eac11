"""Inputs and an oracle-free checker for the k-d tree tests.

* adversary(n): the frozen key sequence of tests/native/introselect_adversary.cpp (McIlroy's adversary run against the
  project's own median selection), read from tests/golden/introselect_adversary.npz.  tests/test_kd_cases.py regenerates the
  sequences on the CPU and proves that each takes the selection's depth-limit fallback.
* planted_orders(n): the x orders the host check of introselect.h uses, as point sets whose point i is the i-th element: the
  root split (depth 0, on x, ids loaded 0..n-1 in order) sees exactly the planted order.
* check_tree(nodes, xy): the definition of a k-d tree in the reference's pre-order layout, without the oracle.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADVERSARY_FIXTURE = os.path.join(ROOT, "tests", "golden", "introselect_adversary.npz")
# both sides of the lane / wave threshold (48) and of the 64-lane chunk of the ballot scans, and two sizes with several
# wave-path levels
ORDER_SIZES = (40, 47, 48, 49, 63, 64, 65, 127, 128, 129, 300, 2000)
ORDER_NAMES = ("adversary", "sorted", "reversed", "organ-pipe", "all-equal-x", "four-values", "all-equal-xy")


def header_constant(name):
    text = open(os.path.join(ROOT, "include", "vslam_amd.h")).read()
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", text, re.M)
    assert m, f"{name} is not defined in include/vslam_amd.h"
    return int(m.group(1))


VSLAM_MAX_KP = header_constant("VSLAM_MAX_KP")
# the largest kp_stride vslam_kdtree_build takes; the rule is restated in tests/test_kd_cases.py
KDTREE_MAX_KP = header_constant("VSLAM_KDTREE_MAX_KP")
ADVERSARY_SIZES = ORDER_SIZES + (KDTREE_MAX_KP,)

_adv = {}


def adversary(n):
    """float32 [n], distinct integers 0..n-1: nth_element(0, n/2, n) over them ends in heap_select."""
    if not _adv:
        with np.load(ADVERSARY_FIXTURE) as z:
            _adv.update({int(k[1:]): z[k] for k in z.files})
    return _adv[n].astype(np.float32)


def planted_orders(n):
    """[(name, xy float32 [n, 2])] in ORDER_NAMES' order."""
    i = np.arange(n)
    rng = np.random.default_rng(9000 + n)
    xs = [adversary(n), i, n - i, np.where(i < n // 2, i, n - i), np.full(n, 7), rng.integers(0, 4, n), np.full(n, 5)]
    out = []
    for name, x in zip(ORDER_NAMES, xs):
        y = np.full(n, 5) if name == "all-equal-xy" else rng.integers(0, 720, n)
        out.append((name, np.stack([x, y], 1).astype(np.float32)))
    return out


def check_tree(nodes, xy):
    """None if nodes[:n] is a k-d tree of xy [n, 2] in pre-order -- a permutation of 0..n-1 where the subtree of len nodes at
    position p has its root at p, len/2 nodes on the left (from p + 1) and len - len/2 - 1 on the right, and at depth d every
    left key on axis d & 1 is <= the root's key <= every right key -- else a string that says what is wrong."""
    nodes = np.asarray(nodes)
    n = len(xy)
    if nodes.shape != (n,):
        return f"{nodes.shape} nodes for {n} points"
    if not np.array_equal(np.sort(nodes), np.arange(n)):
        return "nodes are not a permutation of 0..n-1"
    keys = (np.asarray(xy, np.float32)[nodes, 0], np.asarray(xy, np.float32)[nodes, 1])   # in pre-order position
    stack = [(0, n, 0)]
    while stack:
        pos, ln, depth = stack.pop()
        if ln <= 1:
            continue
        k = keys[depth & 1]
        nl = ln // 2
        nr = ln - nl - 1
        if k[pos + 1:pos + 1 + nl].max() > k[pos]:
            return f"depth {depth}, position {pos}: a left key above the node's"
        if nr > 0 and k[pos + 1 + nl:pos + ln].min() < k[pos]:
            return f"depth {depth}, position {pos}: a right key below the node's"
        stack.append((pos + 1, nl, depth + 1))
        stack.append((pos + 1 + nl, nr, depth + 1))
    return None
