"""What the geometric fusing's kernels compile (vslam_amd/csrc/fuse_project_math.h: who takes part, which pairs are tried, the packed
proposal; search_math.h: visibility, the disc, the choice, the keys, the grid; fuse_math.h: valid entries, a sound CSR) built for the
host as a stand-alone program with -fsanitize=address,undefined and walked serially (tests/native/fuse_project_serial.cpp: cameras and
points from the last to the first, keys and holders in ordered maps, the found pairs sorted at the end), held bit for bit to
tests/ref_fuse_project.py -- which has no grid -- on every hand case and on the random items up to n = 257.  Nothing sanitized is loaded
into Python."""
import numpy as np
import pytest

import fuse_project_cases as fpc
import ref_fuse_project as rfp

KEYS = rfp.OUTS + ("n_found", "stats")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return fpc.build_serial(tmp_path_factory.mktemp("serial"))


def _walk(exe, tmp_path, named):
    got = fpc.run_serial(exe, tmp_path, list(named.values()))
    for (name, c), g in zip(named.items(), got):
        ref = rfp.reference(c)
        for k in KEYS:
            assert np.array_equal(g[k], ref[k]), (name, k, g[k], ref[k])
    return got


def test_hand_cases_on_the_serial_walk(exe, tmp_path):
    cases = fpc.hand_cases()
    got = _walk(exe, tmp_path, cases)
    for (name, c), g in zip(cases.items(), got):
        assert fpc.found_of(g) == c["expect"], name
        if c["expect_stats"] is not None:
            assert np.array_equal(g["stats"], c["expect_stats"]), name


def test_random_items_on_the_serial_walk(exe, tmp_path):
    cases = {name: c for name, c in fpc.random_cases().items() if c["n"] <= 257}
    assert len(cases) >= 5
    got = _walk(exe, tmp_path, cases)
    assert sum(g["stats"][4] > 0 for g in got) >= 4
    short = {name: dict(c, found_stride=max(int(g["stats"][3]) - 1, 1)) for (name, c), g in zip(cases.items(), got)}
    _walk(exe, tmp_path, short)
