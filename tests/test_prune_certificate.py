"""The one-sided certificate of ransac_prune.hip on the host.  tests/native/prune_cert_check.cpp compiles
vslam_amd/csrc/ransac_prune_cert.h, the header the kernel compiles, and applies it to float32 values of n and a0 formed in three
accumulation orders (forward, reverse, pairwise), each with and without fma.  Held here to the oracle (oracle.residual, the
reference's own floats) and to tests/ref64.py: no (hypothesis, match) is ever a certified miss while the oracle calls it an
inlier -- on the inputs of tests/test_gpu_ransac_headstart.py, on hypotheses scaled far down and up, on a zero first row and
NaN, and on matches placed within 1e-6 relative of n^2 = thr a0^2, where the certificate has to stay silent or be right."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref64
from test_gpu_ransac_headstart import first_exit_inputs, plateau_inputs, uncertified_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("forward", "forward fma", "reverse", "reverse fma", "pairwise", "pairwise fma")


@pytest.fixture(scope="module")
def cert_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prune_cert") / "prune_cert_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "native", "prune_cert_check.cpp")], check=True)
    return exe


def certify(exe, tmp_path, cases):
    """cases: [(thr, F (H, 9), xy (M, 4))] -> [uint8 (H, M)]: bit v set where form v certified a miss."""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for thr, F, xy in cases:
            f.write(struct.pack("fii", thr, len(F), len(xy)))
            f.write(np.ascontiguousarray(F, np.float32).tobytes())
            f.write(np.ascontiguousarray(xy, np.float32).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    buf = np.frombuffer(open(fout, "rb").read(), np.uint8)
    out, at = [], 0
    for _, F, xy in cases:
        out.append(buf[at:at + len(F) * len(xy)].reshape(len(F), len(xy)))
        at += len(F) * len(xy)
    assert at == len(buf)
    return out


def matched(xy1, xy2, pairs):
    """(M, 4): x1, y1, x2, y2 of every match."""
    return np.concatenate([xy1[pairs[:, 0]], xy2[pairs[:, 1]]], 1).astype(np.float32)


def oracle_inliers(oracle, xy, F, thr):
    """(H, M) bool: the reference's own decision e <= thr for every hypothesis and match."""
    ident = np.stack([np.arange(len(xy)), np.arange(len(xy))], 1).astype(np.int32)
    p1, p2 = np.ascontiguousarray(xy[:, 0:2]), np.ascontiguousarray(xy[:, 2:4])
    with np.errstate(all="ignore"):
        return np.stack([np.asarray(oracle.residual(p1, p2, ident, f, thr)[0]).astype(bool) for f in F])


def assert_sound(oracle, cert, xy, F, thr, tag):
    inl = oracle_inliers(oracle, xy, F, thr)
    for v, name in enumerate(FORMS):
        bad = ((cert >> v) & 1).astype(bool) & inl
        assert not bad.any(), (tag, name, np.argwhere(bad)[:4])
    # tests/ref64.py: what float64 decides an inlier beyond any f32 error is never certified either
    ident = np.stack([np.arange(len(xy)), np.arange(len(xy))], 1)
    with np.errstate(all="ignore"):
        r = ref64.residuals(F, xy[:, 0:2], xy[:, 2:4], ident, thr, keep=list(range(len(F))))
    sure = np.asarray(r["decided"], bool) & np.asarray(r["inlier"], bool)
    assert not ((cert != 0) & sure).any(), tag
    return inl


def test_first_exit_premise_and_soundness(oracle, cert_exe, tmp_path):
    """The hard data (55 % inliers, exact): the oracle alone puts D = m - maximum + 1 inside (256, 384]; the certificate, over
    a fourth of the hypotheses, never marks an inlier, and marks most of what is not one."""
    for exact in (True, False):
        xy1, xy2, pairs, m, sets, thr = first_exit_inputs(oracle, exact)
        cases, keep = [], []
        for b in range(len(m)):
            n = int(m[b])
            ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
            if exact:
                D = n - int(ref["count"]) + 1
                assert 256 < D <= 384, (n, D)
            F = ref["hypF"][::4]
            cases.append((thr, F, matched(xy1[b], xy2[b], pairs[b, :n])))
        certs = certify(cert_exe, tmp_path, cases)
        for b, (cert, (_, F, xy)) in enumerate(zip(certs, cases)):
            inl = assert_sound(oracle, cert, xy, F, thr, ("first exit", exact, b))
            share = (cert == 63)[~inl].mean()
            print("first exit (exact %s) m = %d: %.1f %% of the oracle's misses certified in all six forms" % (exact, len(xy), 100 * share))
            assert share > 0.5, (exact, b, share)


def test_plateau_and_uncertified_inputs(oracle, cert_exe, tmp_path):
    xy1, xy2, pairs, m, sets, thr = plateau_inputs(oracle)
    cases = []
    for b in range(len(m)):
        n = int(m[b])
        ref = oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], thr)
        cases.append((thr, ref["hypF"][::4], matched(xy1[b], xy2[b], pairs[b, :n])))
    xy1, xy2, pairs, m, sets, hypF = uncertified_inputs(oracle)     # scaled by 1e-18, all NaN, zero first row
    for b in range(len(m)):
        for t in (10.0, 3e6, 1e-7):
            cases.append((t, hypF[b], matched(xy1[b], xy2[b], pairs[b, :int(m[b])])))
    certs = certify(cert_exe, tmp_path, cases)
    for i, (cert, (t, F, xy)) in enumerate(zip(certs, cases)):
        assert_sound(oracle, cert, xy, F, t, ("plateau / uncertified", i))
        nan_rows = np.isnan(F).any(axis=1)
        assert not cert[nan_rows].any(), i                      # a NaN hypothesis certifies nothing
        if not (2.0 ** -20 <= t <= 2.0 ** 20):
            assert not cert.any(), (i, t)                       # a threshold outside the stated range: nothing at all


@pytest.mark.parametrize("scale", [1e-18, 1e-30, 1e18, 1.0])
def test_scaled_hypotheses_and_the_edge_of_the_band(oracle, cert_exe, tmp_path, scale):
    """Hypotheses scaled far down (a0^2 underflows, then n^2 as well) and far up (beyond |f| <= 2^10: nothing may be certified),
    with a zero first row and a NaN among them; and, per hypothesis, matches whose y2 is solved so that n = +-sqrt(thr) a0 (1 + d)
    with d spread over +-1e-6: on the edge of what the certificate may decide."""
    xy1, xy2, pairs, m, sets, thr = first_exit_inputs(oracle, True)
    n = int(m[0])
    ref = oracle.find_fundamental(xy1[0], xy2[0], pairs[0, :n], sets[0], thr)
    rng = np.random.default_rng(81)
    F = ref["hypF"][rng.choice(len(ref["hypF"]), 24, replace=False)].copy()
    F[0] = ref["hypF"][int(ref["winner"])]
    xy = matched(xy1[0], xy2[0], pairs[0, :n])[:256]
    # matches on the edge: for hypothesis h and an (x1, y1) of the data, y2 from n = x2 a0 + y2 a1 + a2 = +-sqrt(thr) a0 (1 + d)
    # in float64 with x2 = 0.5.  Rounding y2 to float32 moves n by up to 2^-24 |y2 a1|, far more than 1e-6 of sqrt(thr) |a0| at
    # pixel scale; so x2 is solved again for the rounded y2 and rounded in turn: it stays near 0.5, where a float32 step moves
    # n by less than 2^-24 |a0|, 2e-8 of the target.  Eight per hypothesis, d spread over +-1e-6, both signs of n.
    edge, edge_h = [], []
    s = np.sqrt(np.float64(np.float32(thr)))
    for h in range(len(F)):
        f = F[h].astype(np.float64)
        kept = 0
        for j in range(len(xy)):
            if kept == 8:
                break
            x1, y1 = xy[(7 * h + j) % len(xy), 0:2].astype(np.float64)
            a0 = f[0] * x1 + f[1] * y1 + f[2]; a1 = f[3] * x1 + f[4] * y1 + f[5]; a2 = f[6] * x1 + f[7] * y1 + f[8]
            target = (1.0 if kept % 2 else -1.0) * s * a0 * (1.0 + (kept - 3.5) / 3.5 * 1e-6)
            with np.errstate(all="ignore"):
                y2 = np.float64(np.float32((target - 0.5 * a0 - a2) / a1))
                x2 = np.float64(np.float32((target - y2 * a1 - a2) / a0))
            if np.isfinite(y2) and np.isfinite(x2) and abs(y2) < 2.0 ** 20 and 0.25 <= x2 <= 1.0:
                edge.append([x1, y1, x2, y2])
                edge_h.append(h)
                kept += 1
    n_data = len(xy)
    xy = np.concatenate([xy, np.array(edge, np.float32).reshape(-1, 4)])
    # The edge matches are where they were aimed: |n| / (sqrt(thr) |a0|) of each under its own hypothesis, in float64 from the
    # float32 coordinates, is 1 within the 1e-6 asked for plus the 2e-8 that rounding x2 may add.
    assert len(edge) >= 100, len(edge)
    for (x1, y1, x2, y2), h in zip(xy[n_data:].astype(np.float64), edge_h):
        f = F[h].astype(np.float64)
        a0 = f[0] * x1 + f[1] * y1 + f[2]; a1 = f[3] * x1 + f[4] * y1 + f[5]; a2 = f[6] * x1 + f[7] * y1 + f[8]
        ratio = abs(x2 * a0 + y2 * a1 + a2) / (s * abs(a0))
        assert abs(ratio - 1.0) <= 1.03e-6, (h, ratio)
    with np.errstate(all="ignore"):
        Fs = (F.astype(np.float64) * scale).astype(np.float32)
    Fs[1, 0:3] = 0
    Fs[2, 4] = np.float32("nan")
    cert, = certify(cert_exe, tmp_path, [(thr, Fs, xy)])
    inl = assert_sound(oracle, cert, xy, Fs, thr, ("scaled", scale))
    assert not cert[2].any()
    if scale == 1e18:
        assert not cert[np.abs(Fs).max(axis=1) > 1024].any()     # outside |f| <= 2^10: never pruned
    print("scale %g: %d of %d evaluations certified in some form, %d oracle inliers" % (scale, (cert != 0).sum(), cert.size, inl.sum()))
    if scale == 1.0:
        # under its own hypothesis an edge match is an outlier of the oracle unless a1^2 + t0^2 + t1^2 vanish (e >= q, q at thr):
        # the certificate must stay silent on nearly all of them (c is tens of u wide, the matches lie within 1e-6 = 17 u), and
        # may speak about the far-away data
        own = cert[edge_h, n_data + np.arange(len(edge_h))]
        print("edge matches certified under their own hypothesis: %d of %d; oracle inliers among them: %d"
              % ((own != 0).sum(), len(own), inl[edge_h, n_data + np.arange(len(edge_h))].sum()))
        own_inl = inl[edge_h, n_data + np.arange(len(edge_h))]
        assert own_inl.any() and not own_inl.all()      # the oracle decides them both ways: they do straddle its threshold
        edited = np.isin(edge_h, (1, 2))                # rows 1 and 2 were edited after the matches were placed
        assert not (own[~edited] != 0).any()            # c is 18 u of the terms' sum wide: within 1e-6 nothing is certified
        assert (cert[:, :n_data] != 0).any()
