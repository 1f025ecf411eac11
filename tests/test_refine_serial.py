"""The arithmetic the refine kernel compiles (vslam_amd/csrc/refine_math.h: a point's blocks, the reduced solve, the tangent
basis, the rotation update) built for the host and walked serially (tests/native/refine_serial.cpp), against tests/ref_refine.py.

Both run the header's iteration in float64 from the same start and differ in the order of their sums and in the linear solves
(Cholesky here, LU in numpy).  The sums' rounding is about sqrt(n) 2^-53 (4e-15 at n = 1023) and the reduced system's condition is
at most 1 / 4.6e-5 = 2e4 on these inputs (tests/test_ref_refine.py), so the unknowns agree to about 1e-10 of their scale; that is
the bound.  Measured: 3e-16 in R, 5e-15 in t, 2e-14 relative in the points.  The accepted-step counts are equal because every
decision of these reference runs is at least ref_refine.DECIDED_MARGIN from a tie."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_refine as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-10


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("serial") / "refine_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-o", out, os.path.join(ROOT, "tests", "native", "refine_serial.cpp")],
                   check=True)
    return out


@pytest.mark.parametrize("name", ["K64_n8", "K64_n63", "K1024_n257", "K1024_n1023"])
def test_serial_walk_of_the_kernel_arithmetic(exe, tmp_path, name):
    info = rr.comparison_results()[name][4]
    part = info["part"]
    n = int(part.sum())
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", n))
        for a in (rr.KMAT.astype(np.float64), info["R_start"], info["t_start"], np.c_[info["o1"][part], info["o2"][part]], info["X_start"]):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    out = subprocess.run([exe, fin, str(rr.MAX_ITERATIONS)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    accepted, obj = out[0].split()
    R = np.array(out[1].split(), float).reshape(3, 3); t = np.array(out[2].split(), float); X = np.array(out[3].split(), float).reshape(n, 3)
    dR, dt = np.abs(R - info["R64"]).max(), np.abs(t - info["t64"]).max()
    dX = np.abs(X - info["X64"]).max() / np.abs(info["X64"]).max()
    print(f"{name}: accepted {accepted} / {info['stats'][3]}, dR {dR:.1e}, dt {dt:.1e}, dX {dX:.1e}")
    assert int(accepted) == info["stats"][3]
    assert abs(float(obj) - info["objective"][-1]) <= 1e-10 * info["objective"][-1]
    assert dR <= BOUND and dt <= BOUND and dX <= BOUND
