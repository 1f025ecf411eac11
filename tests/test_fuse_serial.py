"""What the fusion and cull kernels compile (vslam_amd/csrc/fuse_math.h: which entries and offsets count, the per-observation test of
the cull, a point's verdict) built for the host as a stand-alone program with -fsanitize=address,undefined and walked serially
(tests/native/fuse_serial.cpp: the fusion by a sort over (cam, kp, row) and a union-find, no cell table and no rounds; the cull's points
in descending order), held bit for bit to tests/ref_fuse.py on the hand cases and on random items."""
import numpy as np
import pytest

import fuse_cases as fc
import ref_fuse as rf


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return fc.build_serial(tmp_path_factory.mktemp("serial"))


def _walk(exe, tmp_path, named):
    got = fc.run_serial(exe, tmp_path, list(named.values()))
    for (name, c), g in zip(named.items(), got):
        if "cam_stride" in c:
            ref, keys = fc.fuse_reference(c), rf.FUSE_OUTS
        else:
            ref, keys = fc.cull_reference(c), rf.CULL_OUTS
        for k in keys:
            assert np.array_equal(g[k], ref[k]), (name, k, g[k], ref[k])
    return got


def test_hand_cases_on_the_serial_walk(exe, tmp_path):
    cases = dict(fc.fuse_hand_cases(), cull=fc.cull_hand_case())
    got = _walk(exe, tmp_path, cases)
    for (name, c), g in zip(cases.items(), got):
        assert np.array_equal(g["keep" if name == "cull" else "fuse_to"], c["expect"]), name
    assert np.array_equal(got[-1]["counts"], cases["cull"]["expect_counts"])


def test_random_fusions_on_the_serial_walk(exe, tmp_path):
    cases = {f"n{n}s{s}": rf.random_fuse_item(77 * n + s, n, kp_stride=max(16, n // 2), S=n + 3) for n in (1, 2, 40, 257, 513, 1200) for s in (0, 1)}
    cases["chain"] = dict(n=300, offsets=np.arange(0, 602, 2, dtype=np.int32), cam=np.zeros(600, np.int32),
                          kp=np.stack([np.arange(300, 0, -1), np.arange(299, -1, -1)], 1).reshape(-1).astype(np.int32), cam_stride=1, kp_stride=301, mask=None)
    got = _walk(exe, tmp_path, cases)
    assert (got[-1]["fuse_to"] == 0).all() and got[-1]["stats"].tolist() == [300, 1, 299, 301]
    assert all(g["stats"][2] > 0 for (name, _), g in zip(cases.items(), got) if not name.startswith(("n1s", "n2s")))


def test_random_culls_on_the_serial_walk(exe, tmp_path):
    cases = {f"n{n}c{c}": rf.random_cull_item(5 * n + c, n, c, S=n + 4) for n, c in ((40, 6), (257, 6), (600, 64))}
    cases["params"] = dict(rf.random_cull_item(3, 300, 6), params=dict(inlier_px=3.0, min_good=1, mature_good=4, mature_age=1, good10=8))
    got = _walk(exe, tmp_path, cases)
    for g in got:
        assert g["stats"][1] > 0 and g["stats"][2] > 0 and (g["keep"] == -1).any()
