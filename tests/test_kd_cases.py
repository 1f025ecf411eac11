"""The k-d tree tests' own tools, checked on the CPU: the adversarial sequences do what the GPU tests plant them for, the
tree checker rejects wrong trees, and the build limit the header states is the one the launcher's rule gives."""
import os
import sys

import numpy as np

import kd_cases

sys.path.insert(0, os.path.join(kd_cases.ROOT, "tests", "golden"))
import make_adversary  # noqa: E402


def test_adversary_sequences_take_the_fallback_and_match_the_fixture(native_bin):
    """Regenerated with the project's own introselect.h, every sequence equals the committed one; replayed as plain floats it
    sends the MEDIAN selection -- all the build ever asks for -- through heap_select at least once, at every size the GPU
    tests use on either side of the lane / wave threshold, and leaves std::nth_element's permutation."""
    exe = native_bin("introselect_adversary", link_oracle=False)
    got = make_adversary.generate(exe, kd_cases.ADVERSARY_SIZES)
    assert sorted(got) == sorted(kd_cases.ADVERSARY_SIZES)
    for n, (heap_calls, same_as_std, keys) in got.items():
        assert heap_calls >= 1, f"n = {n}: the depth limit was not reached"
        assert same_as_std == 1, n
        assert np.array_equal(np.sort(keys), np.arange(n)), n
        assert np.array_equal(kd_cases.adversary(n), keys.astype(np.float32)), f"n = {n}: fixture differs"


def test_tree_checker_accepts_the_oracles_trees_and_rejects_planted_errors(oracle):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 64, 301):
        xy = rng.integers(0, 40, (n, 2)).astype(np.float32)          # many ties
        nodes = oracle.kdtree_build_frame(xy)
        assert kd_cases.check_tree(nodes, xy) is None, n
    for name, xy in kd_cases.planted_orders(129):
        assert kd_cases.check_tree(oracle.kdtree_build_frame(xy), xy) is None, name
    n = 301
    xy = np.stack([rng.permutation(n), rng.permutation(n)], 1).astype(np.float32)   # distinct keys: any exchange shows
    nodes = oracle.kdtree_build_frame(xy)
    nl = n // 2
    bad = nodes.copy()                                   # two nodes exchanged across the root's split
    bad[[1 + 3, 1 + nl + 5]] = bad[[1 + nl + 5, 1 + 3]]
    assert "depth 0" in kd_cases.check_tree(bad, xy)
    bad = nodes.copy()                                   # across a split two levels down (inside the left-left subtree)
    sub = nl // 2
    bad[[2 + 1, 2 + 1 + sub // 2 + 1]] = bad[[2 + 1 + sub // 2 + 1, 2 + 1]]
    assert "depth 2" in kd_cases.check_tree(bad, xy)
    bad = nodes.copy()                                   # the root exchanged with its left child
    bad[[0, 1]] = bad[[1, 0]]
    assert kd_cases.check_tree(bad, xy) is not None
    bad = nodes.copy()                                   # a duplicated index
    bad[17] = bad[200]
    assert "permutation" in kd_cases.check_tree(bad, xy)
    assert kd_cases.check_tree(nodes[:-1], xy) is not None
    assert kd_cases.check_tree(nodes, xy) is None


def test_header_states_the_build_limit_of_the_launchers_rule():
    """vs_launch_kdtree_build (kdtree.hip): 8 bytes of coordinates and three 16-bit words per slot and 4 bytes more, rounded
    up to 16, must not exceed 160 KB less 512 bytes.  The largest kp_stride that passes is what the header promises."""
    def lds(k):
        return (k * 8 + k * 2 * 3 + 4 + 15) & ~15
    cap = 160 * 1024 - 512
    k = kd_cases.KDTREE_MAX_KP
    assert lds(k) <= cap < lds(k + 1)
    assert k == 11666 and k < kd_cases.VSLAM_MAX_KP
    src = open(os.path.join(kd_cases.ROOT, "vslam_amd", "csrc", "kdtree.hip")).read()
    assert "(size_t)kp_stride * 8 + (size_t)kp_stride * 2 * 3 + 4 + 15) & ~(size_t)15" in src   # the rule restated above
    assert "VS_REQUIRE(ctx, lds <= 160 * 1024 - 512, VSLAM_ERR_CAPACITY);" in src
