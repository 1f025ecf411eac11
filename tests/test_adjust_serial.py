"""The arithmetic the adjustment kernel compiles (vslam_amd/csrc/adjust_math.h: an observation's blocks, a point's damped solve, the
entries of the reduced system and its Cholesky solve, the candidate, the rounds) built for the host as a stand-alone program with
-fsanitize=address,undefined and walked serially (tests/native/adjust_serial.cpp), against tests/ref_adjust.py.

Both run the header's rounds in float64 from the same inputs and differ in the order of their sums over the points (left to right
here, pairwise in numpy), in the inner sums of the reduced solve (numpy dot products there) and in the library sine.
DELTA_ORDER is the largest disagreement measured between the two over the comparison cases (R entries absolute, T and X relative
to max(1, max|.|)); the test holds every case to it, holds it under BOUND = 1e-6, the issue's ceiling for either delta, and
checks that it is no more than 4 x what the cases give (a bound far above what is measured would hide a regression).
The accepted-step counts are compared on the runs every decision of which is at least ref_adjust.DECIDED_MARGIN from a tie; the
participants of the last round are compared on all of them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_adjust as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-6
# measured per case (this file's test prints them)
DELTA_ORDER_CASES = {"c2n8": 2.74e-11, "c3n9": 5.90e-10, "c4n40": 1.07e-14, "c8n257": 4.39e-15, "c8n2000": 5.87e-15,
                     "decided_c4n40": 5.65e-15, "decided_c8n257": 2.38e-13, "decided_c8n2000": 1.28e-14}
DELTA_ORDER = 6.0e-10   # the largest of them (c3n9), rounded up
_seen = {}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(str(tmp_path_factory.mktemp("serial") / "adjust_serial"))


def build_exe(out):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "adjust_serial.cpp")], check=True)
    return out


def run(exe, path, R, T, X, off, cam, xy, p, C=None, N=None, pt_stride=None, obs_stride=None):
    """-> moved, stats (4,), R, T, X of the serial walk; C / N: the counts claimed (default: the arrays')"""
    cs, ps, os_ = len(R), max(pt_stride or len(X), 1), max(obs_stride or len(cam), 1)
    Xp = np.zeros((ps, 3)); Xp[:len(X)] = X
    offp = np.zeros(ps + 1, np.int32); offp[:len(off)] = off
    camp = np.zeros(os_, np.int32); camp[:len(cam)] = cam
    xyp = np.zeros((os_, 2), np.float32); xyp[:len(xy)] = xy
    with open(path, "wb") as f:
        f.write(struct.pack("10i", cs, ps, os_, len(R) if C is None else C, len(X) if N is None else N, p["max_iterations"], p["rounds"],
                            p["min_obs"], p["n_fixed"], 0))
        f.write(struct.pack("dd", p["huber_px"], p["gate_px"]))
        f.write(ra.kmat().astype(np.float64).tobytes())
        for a, dt in ((R, np.float64), (T, np.float64), (Xp, np.float64), (offp, np.int32), (camp, np.int32), (xyp, np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    out = subprocess.run([exe, path], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    v = [np.array(l.split(), float) for l in out[1:5]]
    return int(out[0]), v[0], v[1].reshape(cs, 9), v[2].reshape(cs, 3), v[3].reshape(ps, 3)[:len(X)]


def deltas(got, ref):
    """entry-wise disagreement: R absolute, T and X relative to max(1, max|.|)"""
    (R, T, X), (Rr, Tr, Xr) = got, ref
    return max(float(np.abs(R - Rr).max()), float(np.abs(T - Tr).max() / max(1.0, np.abs(Tr).max())),
               float(np.abs(X - Xr).max() / max(1.0, np.abs(Xr).max())) if len(Xr) else 0.0)


@pytest.mark.parametrize("name", list(ra.comparison_cases()))
def test_serial_walk_of_the_kernel_arithmetic(exe, tmp_path, name):
    pr, p = ra.cases()[name]
    Rr, Tr, Xr, sr, info = ra.comparison_results()[name]
    moved, st, Rs, Ts, Xs = run(exe, str(tmp_path / "in.bin"), pr["R"], pr["T"], pr["X"], pr["off"], pr["cam"], pr["xy"], p)
    d = deltas((Rs, Ts, Xs), (Rr, Tr, Xr))
    print(f"{name}: accepted {st[3]} / {sr[3]}, margin {info['margin']:.1e}, gate margin {info['gate_margin']:.1e}, delta {d:.1e}")
    assert moved == 1 and info["moved"]
    assert info["gate_margin"] >= ra.DECIDED_MARGIN and st[0] == sr[0]
    if name.startswith("decided"):
        assert info["margin"] >= ra.DECIDED_MARGIN
    if info["margin"] >= ra.DECIDED_MARGIN:
        assert st[3] == sr[3]
    _seen[name] = d
    assert d <= DELTA_ORDER < BOUND
    assert abs(st[1] - sr[1]) <= 1e-9 * sr[1] and abs(st[2] - sr[2]) <= 1e-6 * sr[2]
    fixed = ~info["free"]
    assert np.array_equal(Rs[fixed], pr["R"][fixed]) and np.array_equal(Ts[fixed], pr["T"][fixed]), "a held camera keeps its bits"


def test_delta_order_is_what_the_cases_give():
    assert set(_seen) == set(DELTA_ORDER_CASES), "runs behind the parametrised test"
    assert max(_seen.values()) >= 0.25 * DELTA_ORDER


def test_left_alone_keeps_the_bits(exe, tmp_path):
    pr, p = ra.cases()["c4n40"]
    a = [pr[k] for k in ("R", "T", "X", "off", "cam", "xy")]

    def alone(got, count=None):
        moved, st, Rs, Ts, Xs = got
        assert moved == 0 and np.isnan(st[1:]).all() and (count is None or st[0] == count)
        assert np.array_equal(Rs, a[0]) and np.array_equal(Ts, a[1])
        return Xs
    path = str(tmp_path / "in.bin")
    assert np.array_equal(alone(run(exe, path, *a, p, N=0), 0), a[2])                                  # no points
    assert np.array_equal(alone(run(exe, path, *a, p, N=41), 0), a[2])                                 # N beyond the stride
    assert np.array_equal(alone(run(exe, path, *a, p, C=9), 0), a[2])                                  # C beyond the stride
    off = a[3].copy(); off[5] = off[4] - 1
    assert np.array_equal(alone(run(exe, path, a[0], a[1], a[2], off, a[4], a[5], p), 0), a[2])        # decreasing offsets
    Rn = a[0].copy(); Rn[1, 4] = np.nan
    moved, st, Rs, Ts, Xs = run(exe, path, Rn, a[1], a[2], a[3], a[4], a[5], p)                       # a NaN in a held camera
    assert moved == 0 and st[0] == 0 and np.array_equal(Rs, Rn, equal_nan=True) and np.array_equal(Xs, a[2])
    once = np.arange(len(a[2]) + 1, dtype=np.int32)                                                    # every point seen once
    assert np.array_equal(alone(run(exe, path, a[0], a[1], a[2], once, a[4], a[5], p), 0), a[2])
    assert np.array_equal(alone(run(exe, path, *a, dict(p, n_fixed=4))), a[2])                         # no camera left free
    assert np.array_equal(alone(run(exe, path, *a, dict(p, min_obs=1000))), a[2])                      # every free camera below min_obs


def test_a_camera_below_min_obs_is_held_while_the_others_move(exe, tmp_path):
    pr, p = ra.cases()["c4n40"]
    keep = np.ones(len(pr["cam"]), bool)
    keep[np.nonzero(pr["cam"] == 3)[0][5:]] = False           # camera 3 keeps 5 observations
    pid = np.repeat(np.arange(len(pr["X"])), np.diff(pr["off"]))[keep]
    off = np.concatenate([[0], np.cumsum(np.bincount(pid, minlength=len(pr["X"])))]).astype(np.int32)
    a = (pr["R"], pr["T"], pr["X"], off, pr["cam"][keep], pr["xy"][keep])
    moved, st, Rs, Ts, Xs = run(exe, str(tmp_path / "in.bin"), *a, p)
    Rr, Tr, Xr, sr, info = ra.adjust(*a, ra.kmat(), **p)
    assert moved == 1 and info["moved"] and info["free"].tolist() == [False, False, True, False]
    assert np.array_equal(Rs[3], pr["R"][3]) and np.array_equal(Ts[3], pr["T"][3]) and not np.array_equal(Rs[2], pr["R"][2])
    assert st[0] == sr[0] and deltas((Rs, Ts, Xs), (Rr, Tr, Xr)) <= BOUND
