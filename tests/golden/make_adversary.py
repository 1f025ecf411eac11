"""Writes tests/golden/introselect_adversary.npz: the frozen key sequences of tests/native/introselect_adversary.cpp for the
sizes the k-d tree tests use (tests/kd_cases.py: ADVERSARY_SIZES), array "n<size>" = uint16 [size].
usage: python tests/golden/make_adversary.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kd_cases  # noqa: E402


def generate(exe, sizes):
    """{n: (heap_select calls of the replay, replay == std::nth_element, keys int64 [n])}"""
    out = {}
    for line in subprocess.run([exe] + [str(n) for n in sizes], check=True, capture_output=True, text=True).stdout.splitlines():
        f = np.array(line.split(), dtype=np.int64)
        assert len(f) == 3 + f[0]
        out[int(f[0])] = (int(f[1]), int(f[2]), f[3:])
    return out


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "introselect_adversary")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(kd_cases.ROOT, "tests", "native", "introselect_adversary.cpp")],
                       check=True)
        got = generate(exe, kd_cases.ADVERSARY_SIZES)
    np.savez_compressed(kd_cases.ADVERSARY_FIXTURE, **{f"n{n}": keys.astype(np.uint16) for n, (_, _, keys) in got.items()})
    print({n: calls for n, (calls, _, _) in got.items()})
