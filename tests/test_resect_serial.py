"""The arithmetic the resection kernels compile (vslam_amd/csrc/resect_math.h: a correspondence's Jacobian, weight and
contributions, the damped 6 x 6 solve, the candidate, the rounds) built for the host as a stand-alone program with
-fsanitize=address,undefined and walked serially (tests/native/resect_serial.cpp), against tests/ref_resect.py.

Both run the header's rounds in float64 from the same inputs and differ in the order of their sums (left to right here, pairwise
in numpy) and in the library sine.  The sums' rounding is about sqrt(n) 2^-53 and the 6 x 6 system's condition is below 1e5 on
these inputs, so the unknowns agree to about 1e-10 of their scale; that is the bound (measured: 2e-15 in R, 6e-15 in T).
The accepted-step counts are compared on the runs every decision of which is at least ref_resect.DECIDED_MARGIN from a tie; the
participants of the last round are compared on all of them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_resect as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-10


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("serial") / "resect_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "resect_serial.cpp")], check=True)
    return out


def run(exe, path, P, x, R, T, p):
    with open(path, "wb") as f:
        f.write(struct.pack("iiii", len(P), p["max_iterations"], p["rounds"], p["min_links"]))
        f.write(struct.pack("dd", p["huber_px"], p["gate_px"]))
        for a in (rr.kmat(), R, T, P, np.asarray(x, np.float32)):
            f.write(np.ascontiguousarray(np.asarray(a).astype(np.float64)).tobytes())
    out = subprocess.run([exe, path], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return int(out[0]), np.array(out[1].split(), float), np.array(out[2].split(), float), np.array(out[3].split(), float)


@pytest.mark.parametrize("name", ["n8", "n40", "n257", "n2000", "decided_n40", "decided_n257", "decided_n2000"])
def test_serial_walk_of_the_kernel_arithmetic(exe, tmp_path, name):
    P, x, R, T, p = rr.comparison_cases()[name]
    Rr, Tr, sr, info = rr.comparison_results()[name]
    moved, st, Rs, Ts = run(exe, str(tmp_path / "in.bin"), P, x, R, T, p)
    dR, dT = np.abs(Rs - Rr).max(), np.abs(Ts - Tr).max() / max(1.0, np.abs(Tr).max())
    print(f"{name}: accepted {st[3]} / {sr[3]}, margin {info['margin']:.1e}, gate margin {info['gate_margin']:.1e}, dR {dR:.1e}, dT {dT:.1e}")
    assert moved == 1 and info["moved"]
    assert info["gate_margin"] >= rr.DECIDED_MARGIN and st[0] == sr[0]
    if name.startswith("decided"):
        assert info["margin"] >= rr.DECIDED_MARGIN
    if info["margin"] >= rr.DECIDED_MARGIN:
        assert st[3] == sr[3]
    assert dR <= BOUND and dT <= BOUND
    assert abs(st[1] - sr[1]) <= 1e-10 * sr[1] and abs(st[2] - sr[2]) <= 1e-9 * sr[2]


def test_left_alone_keeps_the_bits(exe, tmp_path):
    P, x, R, T, p = rr.comparison_cases()["n40"]
    moved, st, Rs, Ts = run(exe, str(tmp_path / "in.bin"), P[:7], x[:7], R, T, p)
    assert moved == 0 and st[0] == 7 and np.isnan(st[1:]).all()
    assert np.array_equal(Rs, R) and np.array_equal(Ts, T)
    Pn = P.copy(); Pn[3, 1] = np.nan
    moved, st, Rs, Ts = run(exe, str(tmp_path / "in.bin"), Pn, x, R, T, p)
    assert moved == 0 and np.array_equal(Rs, R) and np.array_equal(Ts, T)
