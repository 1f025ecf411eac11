"""The refinement the refine kernel compiles (vslam_amd/csrc/refine_math.h: ba_run -- participation, the left-alone rules, the
start, the iteration, the rounding and the statistics -- over a point's blocks, the reduced solve, the tangent basis, the rotation
update) built for the host as a stand-alone program with -fsanitize=address,undefined and walked serially
(tests/native/refine_serial.cpp), against tests/ref_refine.py.

Both run the header's iteration in float64 from the same inputs and differ in the order of their sums and in the linear solves
(Cholesky here, LU in numpy).  The sums' rounding is about sqrt(n) 2^-53 (4e-15 at n = 1023) and the reduced system's condition is
at most 1 / 4.6e-5 = 2e4 on these inputs (tests/test_ref_refine.py), so the unknowns agree to about 1e-10 of their scale; that is
the bound.  Measured: 3e-16 in R, 5e-15 in t, 2e-14 relative in the points.  The accepted-step counts are equal because every
decision of these reference runs is at least ref_refine.DECIDED_MARGIN from a tie.  The participants are counted exactly
(stats[0]); their mean error under the inputs (stats[1]) is one sum of n terms in two orders, held to 1e-9 of itself."""
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
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "refine_serial.cpp")], check=True)
    return out


def run(exe, path, info, keep=None, winner=0):
    """-> the driver's lines for the comparison case behind `info`, or for its correspondences `keep` alone"""
    keep = np.arange(len(info["part"])) if keep is None else keep
    with open(path, "wb") as f:
        f.write(struct.pack("iiii", len(keep), winner, rr.MAX_ITERATIONS, 0))
        f.write(struct.pack("d", rr.GATE_SQ))
        for a in (rr.KMAT, info["R_in"], info["t_in"], np.c_[info["o1"], info["o2"]][keep], info["X_in"][keep]):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    return subprocess.run([exe, path], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()


def inputs(name):
    """the comparison case's info with the refinement's own inputs beside it: R, t and the points as the device is handed them"""
    c = next(c for c in rr.comparison_cases() if c[0] == name)
    info = dict(rr.comparison_results()[name][4])
    n = len(info["part"])
    info.update(R_in=c[5], t_in=c[6], X_in=c[7][:n, :3])
    return info


@pytest.mark.parametrize("name", ["K64_n8", "K64_n63", "K1024_n257", "K1024_n1023"])
def test_serial_walk_of_the_kernel_arithmetic(exe, tmp_path, name):
    info = inputs(name)
    n = int(info["part"].sum())
    out = run(exe, str(tmp_path / "in.bin"), info)
    moved, stats = int(out[0]), np.array(out[1].split(), float)
    accepted, obj = out[2].split()
    R = np.array(out[3].split(), float).reshape(3, 3); t = np.array(out[4].split(), float); X = np.array(out[5].split(), float).reshape(n, 3)
    dR, dt = np.abs(R - info["R64"]).max(), np.abs(t - info["t64"]).max()
    dX = np.abs(X - info["X64"]).max() / np.abs(info["X64"]).max()
    print(f"{name}: accepted {accepted} / {info['stats'][3]}, dR {dR:.1e}, dt {dt:.1e}, dX {dX:.1e}, stats {stats} / {info['stats']}")
    assert moved == 1 and not info["left_alone"]
    assert int(accepted) == info["stats"][3] == stats[3]
    assert abs(float(obj) - info["objective"][-1]) <= 1e-10 * info["objective"][-1]
    assert dR <= BOUND and dt <= BOUND and dX <= BOUND
    assert stats[0] == info["stats"][0]
    assert abs(stats[1] - info["stats"][1]) <= 1e-9 * info["stats"][1]


def test_seven_participants_are_left_alone(exe, tmp_path):
    info = inputs("K64_n8")
    keep = np.nonzero(info["part"])[0][:7]
    assert len(keep) == 7
    out = run(exe, str(tmp_path / "in.bin"), info, keep)
    stats = np.array(out[1].split(), float)
    assert int(out[0]) == 0 and stats[0] == 7 and np.isnan(stats[1:]).all()
