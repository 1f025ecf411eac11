"""The arithmetic the adjustment kernel compiles (vslam_amd/csrc/adjust_math.h: an observation's blocks, a point's damped solve, the
entries of the reduced system and its Cholesky solve, the candidate, the rounds) built for the host as a stand-alone program with
-fsanitize=address,undefined and walked serially (tests/native/adjust_serial.cpp), against tests/ref_adjust.py.

Both run the header's rounds in float64 from the same inputs and differ in the order of their sums over the points (left to right
here, pairwise in numpy), in the inner sums of the reduced solve (numpy dot products there) and in the library sine.
DELTA_ORDER is the largest disagreement measured between the two over the comparison cases (R entries absolute, T and X relative
to max(1, max|.|)); the test holds every case to it, holds it under BOUND = 1e-6, the issue's ceiling for either delta, and
checks that it is no more than 4 x what the cases give (a bound far above what is measured would hide a regression).
The accepted-step counts are compared on the runs every decision of which is at least ref_adjust.DECIDED_MARGIN from a tie; the
participants of the last round are compared on all of them.

ref_adjust.rule_cases() -- ragged CSRs (unusable observations, one-camera and empty rows, a camera seen twice), cameras free in
one round and held in the next, a later round without a free camera, seven and five slots, four rounds, one step -- run through
the same program under the same DELTA_ORDER without entering it (they are not in _seen); their measured deltas, 1.7e-15 ..
6.2e-13, are in the table above test_rule_cases_on_the_serial_walk."""
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


def run(exe, path, R, T, X, off, cam, xy, p, C=None, N=None, pt_stride=None, obs_stride=None, K=None):
    """-> moved, stats (4,), R, T, X of the serial walk; C / N: the counts claimed (default: the arrays'); X from its bits"""
    cs, ps, os_ = len(R), max(pt_stride or len(X), 1), max(obs_stride or len(cam), 1)
    Xp = np.zeros((ps, 3)); Xp[:len(X)] = X
    offp = np.zeros(ps + 1, np.int32); offp[:len(off)] = off
    camp = np.zeros(os_, np.int32); camp[:len(cam)] = cam
    xyp = np.zeros((os_, 2), np.float32); xyp[:len(xy)] = xy
    with open(path, "wb") as f:
        f.write(struct.pack("10i", cs, ps, os_, len(R) if C is None else C, len(X) if N is None else N, p["max_iterations"], p["rounds"],
                            p["min_obs"], p["n_fixed"], 0))
        f.write(struct.pack("dd", p["huber_px"], p["gate_px"]))
        f.write((ra.kmat() if K is None else np.asarray(K)).astype(np.float64).tobytes())
        for a, dt in ((R, np.float64), (T, np.float64), (Xp, np.float64), (offp, np.int32), (camp, np.int32), (xyp, np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    out = subprocess.run([exe, path], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    v = [np.array(l.split(), float) for l in out[1:4]]
    Xs = np.array([int(h, 16) for h in out[5].split()], np.uint64).view(np.float64)
    return int(out[0]), v[0], v[1].reshape(cs, 9), v[2].reshape(cs, 3), Xs.reshape(ps, 3)[:len(X)]


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


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def deltas_finite(got, ref, X_in):
    """deltas() over the points whose input is finite; the others (ref_adjust.ragged's nan_X) are held to the input's bits"""
    odd = ~np.isfinite(X_in).all(1)
    assert np.array_equal(bits(got[2][odd]), bits(X_in[odd])) and np.array_equal(bits(ref[2][odd]), bits(X_in[odd])), "a NaN's bits are kept"
    return deltas((got[0], got[1], got[2][~odd]), (ref[0], ref[1], ref[2][~odd]))


def hold_rule_pattern(name, p, info):
    """what the rule case is there for, asserted on the reference's record of its rounds (free_rounds, n_rounds): the free cameras of
    every round that ran, and that each min_obs separates the counts it is meant to separate"""
    fr, nr = info["free_rounds"], info["n_rounds"]
    if name.startswith("ragged"):
        ra.hold_kinds(ra.rule_cases()[name][0], ra.rule_kinds()[name], info)
        return
    assert ra.free_sets(info) == ra.rule_pattern(name)
    for f, n in zip(fr, nr):
        assert np.array_equal(f, (np.arange(len(n)) >= p["n_fixed"]) & (n >= p["min_obs"]))
    if name in ra.RULE_NO_FREE:
        assert len(fr) == 1 < p["rounds"] and (nr[0][p["n_fixed"]:] >= p["min_obs"]).all()
    if name == "free_then_held_c4":
        assert fr[0][3] and not fr[1][3] and not fr[2][3] and nr[1][3] < p["min_obs"] <= nr[0][3] and fr[2][2]
    if name == "held_then_free_c8":     # slots 6 -> 5 -> 6: the cameras behind 5 are renumbered twice
        assert fr[0][5] and not fr[1][5] and fr[2][5] and nr[1][5] < p["min_obs"] <= nr[2][5] and fr[1][6] and fr[1][7]
    if name == "free_then_held_c8":
        assert fr[0][5] and not fr[1][5] and not fr[2][5] and max(nr[1][5], nr[2][5]) < p["min_obs"] <= nr[0][5]
    if name == "seven_slots":
        assert all(f.sum() == 7 for f in fr) and p["n_fixed"] == 1
    if name == "five_slots":
        assert all(f.sum() == 5 for f in fr) and p["n_fixed"] == 3
    if name == "rounds4":
        assert len(fr) == p["rounds"] == 4
    if name == "one_step":
        assert len(fr) == p["rounds"] == p["max_iterations"] == 1


# measured per rule case: the serial walk against the reference (this file's test prints them); none enters DELTA_ORDER
#   case                   delta    participants  accepted  margin   gate margin
#   ragged_c4n40           1.2e-14       85          36     5.3e-13  8.5e-02     (the default schedule: decided is not asserted)
#   ragged_c8n257          3.3e-15     1257          31     6.6e-15  1.9e-02     (undecided: the count is not compared)
#   ragged_decided_c4n40   1.0e-14       93           4     1.2e-02  8.7e-02
#   ragged_decided_c8n257  6.0e-13     1299           4     5.5e-03  6.9e-03
#   free_then_held_c4      5.5e-15      108           6     1.3e-04  2.1e-03
#   no_free_round1_c4      2.9e-14      137           2     9.7e-03  no gate ran
#   held_then_free_c8      5.6e-13     1333           6     5.4e-03  7.8e-04
#   free_then_held_c8      4.8e-13     1333           6     4.1e-03  7.8e-04
#   no_free_round1_c8      2.2e-14     1677           2     5.4e-03  no gate ran
#   seven_slots            5.2e-14     1326           4     5.7e-03  1.4e-03
#   five_slots             6.2e-13     1322           4     4.8e-03  4.7e-03
#   rounds4                4.8e-13     1333           8     4.1e-04  7.8e-04
#   one_step               1.7e-15     1677           1     9.2e-02  no gate ran
UNDECIDED_RULE_CASES = ("ragged_c4n40", "ragged_c8n257")   # the default schedule: the accepted-step count is not compared


@pytest.mark.parametrize("name", list(ra.rule_cases()))
def test_rule_cases_on_the_serial_walk(exe, tmp_path, name):
    pr, p = ra.rule_cases()[name]
    Rr, Tr, Xr, sr, info = ra.rule_results()[name]
    hold_rule_pattern(name, p, info)
    moved, st, Rs, Ts, Xs = run(exe, str(tmp_path / "in.bin"), pr["R"], pr["T"], pr["X"], pr["off"], pr["cam"], pr["xy"], p)
    d = deltas_finite((Rs, Ts, Xs), (Rr, Tr, Xr), pr["X"])
    print(f"{name}: participants {st[0]:.0f}, accepted {st[3]:.0f} / {sr[3]:.0f}, margin {info['margin']:.1e}, gate margin "
          f"{info['gate_margin']:.1e}, delta {d:.1e}")
    assert moved == 1 and info["moved"]
    assert info["gate_margin"] >= ra.DECIDED_MARGIN and st[0] == sr[0]
    if name not in UNDECIDED_RULE_CASES:
        assert info["margin"] >= ra.DECIDED_MARGIN
    if info["margin"] >= ra.DECIDED_MARGIN:
        assert st[3] == sr[3]
    assert d <= DELTA_ORDER
    assert abs(st[1] - sr[1]) <= 1e-9 * sr[1] and abs(st[2] - sr[2]) <= 1e-6 * sr[2]
    free = info["free"]
    assert np.array_equal(bits(Rs[~free]), bits(pr["R"][~free])) and np.array_equal(bits(Ts[~free]), bits(pr["T"][~free])), "never free: its bits"
    for c in np.nonzero(free)[0]:   # free in some round, round 0 alone included: written, and not with its input
        assert not np.array_equal(Rs[c], pr["R"][c]) and not np.array_equal(Ts[c], pr["T"][c]), c
    last = np.zeros(len(Xr), bool)
    last[np.repeat(np.arange(len(Xr)), np.diff(pr["off"]))[info["part"]]] = True
    assert np.array_equal(bits(Xs[~last]), bits(pr["X"][~last])), "a point outside the last round keeps its input"
    assert not np.array_equal(Xs[last], pr["X"][last]) and ((~last).any() or len(info["free_rounds"]) == 1)
    if name in ra.RULE_NO_FREE:     # round 0's result and participants stand
        one = ra.run(pr, **dict(p, rounds=1))
        assert np.array_equal(bits(one[2]), bits(Xr)) and np.array_equal(one[3], sr) and np.array_equal(one[4]["part"], info["part"])


def test_unused_observations_in_front_change_nothing(exe, tmp_path):
    """offsets[0] > 0: the observations in front of the first row belong to no point"""
    pr, p = ra.rule_cases()["ragged_decided_c4n40"]
    a = [pr[k] for k in ("R", "T", "X", "off", "cam", "xy")]
    rng = np.random.default_rng(5)
    b = a[:3] + [a[3] + 7, np.concatenate([rng.integers(0, 4, 7).astype(np.int32), a[4]]),
                 np.concatenate([rng.uniform(0, 400, (7, 2)).astype(np.float32), a[5]])]
    path = str(tmp_path / "in.bin")
    one, two = run(exe, path, *a, p), run(exe, path, *b, p)
    ref = ra.adjust(*b, ra.kmat(), **p)
    assert one[0] == two[0] == 1 and ref[4]["moved"] and not ref[4]["part"][:7].any()
    for x, y in zip(one[1:], two[1:]):
        assert np.array_equal(bits(x), bits(y))
    for x, y in zip(ref[:4], ra.rule_results()["ragged_decided_c4n40"][:4]):
        assert np.array_equal(bits(x), bits(y))


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
    for bad in (np.nan, np.inf):                                                                       # a non-finite entry of K
        Kb = ra.kmat().copy(); Kb[1, 2] = bad
        assert np.array_equal(alone(run(exe, path, *a, p, K=Kb), 0), a[2])
    off = a[3].copy(); off[-1] = len(a[4]) + 1
    assert np.array_equal(alone(run(exe, path, a[0], a[1], a[2], off, a[4], a[5], p), 0), a[2])        # offsets[N] > obs_stride
    off = a[3].copy(); off[0] = -1
    assert np.array_equal(alone(run(exe, path, a[0], a[1], a[2], off, a[4], a[5], p), 0), a[2])        # offsets[0] < 0
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
