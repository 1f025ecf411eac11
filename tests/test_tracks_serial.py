"""What the track kernel compiles (vslam_amd/csrc/tracks_math.h: the inverse of K, which observations count, rays and centres, the
parallax test, the linear start, the refinement and a point's verdict) built for the host as a stand-alone program with
-fsanitize=address,undefined and walked serially (tests/native/tracks_serial.cpp, the points in descending order), held bit for bit to
tests/ref_tracks.py on the hand cases and on random items."""
import numpy as np
import pytest

import ref_tracks as rt
import tracks_cases as tc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return tc.build_serial(tmp_path_factory.mktemp("serial"))


def _walk(exe, tmp_path, named):
    got = tc.run_serial(exe, tmp_path, list(named.values()))
    for (name, c), g in zip(named.items(), got):
        assert g is not None, name
        tc.same_bits(g, tc.reference(c), name)
    return got


def test_hand_cases_on_the_serial_walk(exe, tmp_path):
    cases = tc.hand_cases()
    got = _walk(exe, tmp_path, cases)
    for name, g in zip(cases, got):
        tc.check_hand(name, g)


def test_random_items_on_the_serial_walk(exe, tmp_path):
    cases = {f"n{n}c{c}": rt.random_track_item(7 * n + c, n, c, S=n + 3) for n, c in ((1, 2), (40, 6), (257, 6), (600, 64))}
    cases["linear_start"] = dict(rt.random_track_item(5, 300, 6), params=dict(iterations=0))
    cases["params"] = dict(rt.random_track_item(6, 300, 6), params=dict(cos_parallax_max=0.99999, huber_px=1.0, inlier_px=2.0, iterations=3, min_good=3, good10=8))
    cases["cam_stride"] = rt.random_track_item(9, 6, 200, rows=(200, 200), cam_stride=203, junk=0.02)
    got = _walk(exe, tmp_path, cases)
    seen = set()
    for (name, c), g in zip(cases.items(), got):
        seen |= set(g["status"].tolist())
        if not name.startswith("n1c"):
            ok = g["status"] == rt.OK
            assert ok.any() and (g["out_points"].view(np.uint32) != c["points"].view(np.uint32)).any(1)[ok].any(), name
    assert {-1, 0, 1, 2, 4, 5, 6} <= seen, sorted(seen)


def test_refused_parameters_and_K_on_the_serial_walk(exe, tmp_path):
    c = tc.hand_item()
    Ks = np.array(c["K"])
    Ks[2] = Ks[0]
    cases = [dict(c, params=dict(min_good=1)), dict(c, params=dict(cos_parallax_max=-1.0)), dict(c, params=dict(iterations=65)), dict(c, K=Ks),
             dict(c, K=np.zeros((3, 3), np.float32)), c]
    got = tc.run_serial(exe, tmp_path, cases)
    assert [g is None for g in got] == [True] * 5 + [False]
