"""The world frame's scale selection on the host.  tests/native/world_select_check.cpp compiles vslam_amd/csrc/world_select.h,
the header the kernel compiles (key formation, rank choice, one radix pass), runs it serially under AddressSanitizer and
UBSan, and is held here to tests/ref_world.py: the same links, the same q bit for bit, the same square root."""
import os
import struct
import subprocess

import numpy as np

import ref_world as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    rng = np.random.default_rng(11)
    out = []
    for n in (1, 2, 7, 8, 9, 64, 255, 256, 257, 1000, 8160):
        carry = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3)
        X = rng.normal(size=(n, 3))
        out.append((carry, X))
    # ties: few distinct ratios; keys that differ only in the lowest byte; an even count whose two medians differ
    carry = np.zeros((100, 3)); carry[:, 2] = rng.integers(1, 4, 100); X = np.tile([0.0, 0, 1], (100, 1))
    out.append((carry, X))
    carry = np.zeros((300, 3)); carry[:, 2] = np.sqrt(1.0 + np.arange(300) * 2.0 ** -52); X = np.tile([0.0, 0, 1], (300, 1))
    out.append((carry[rng.permutation(300)], X))
    # ratios that are not finite do not vote: an overflowed square, |X|^2 = 0 (0 / 0 and c / 0), a NaN
    carry = rng.normal(size=(12, 3)); X = rng.normal(size=(12, 3))
    carry[0] = [1e200, 0, 0]; X[1] = [0, 0, 0]; carry[2] = [0, 0, 0]; X[2] = [0, 0, 0]; carry[3, 1] = np.nan; X[4] = [1e-200, 0, 0]
    out.append((carry, X))
    out.append((np.zeros((0, 3)), np.zeros((0, 3))))
    # the whole exponent range in one case
    carry = np.zeros((2000, 3)); carry[:, 0] = 2.0 ** rng.uniform(-500, 500, 2000); X = np.tile([1.0, 0, 0], (2000, 1))
    out.append((carry, X))
    return out


def test_host_selection_matches_the_reference_under_sanitizers(tmp_path):
    exe = str(tmp_path / "world_select_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "world_select_check.cpp")], check=True)
    cases = _cases()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for carry, X in cases:
            f.write(struct.pack("i", len(carry)))
            f.write(np.ascontiguousarray(np.concatenate([carry, X], 1), np.float64).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    assert len(buf) == 20 * len(cases)
    seen_links = []
    for i, (carry, X) in enumerate(cases):
        links, q, s = struct.unpack_from("<idd", buf, 20 * i)
        with np.errstate(all="ignore"):
            qs = [rw.norm2(c) / rw.norm2(x) for c, x in zip(carry, X)]
        qs = [v for v in qs if np.isfinite(v)]
        assert links == len(qs), i
        seen_links.append(links)
        if not qs:
            assert np.isnan(q)
            continue
        want = rw.lower_median(qs)
        assert np.float64(q).view(np.uint64) == want.view(np.uint64), i
        assert np.float64(s).view(np.uint64) == np.sqrt(want).view(np.uint64), i
    assert seen_links[-3] == 12 - 5 and 0 in seen_links and 8160 in seen_links
