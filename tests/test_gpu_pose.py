"""extract_Rt / camera matrix / triangulate on the device vs the oracle (bit-exact), fed by a real
RANSAC result so the chain F -> (R, t) -> c2 -> 3-D points is the one src/vslam.cpp:77-186 runs; every device
output is also held to the float64 references of tests/ref64.py and, where the motion is known, to the truth."""
import numpy as np
import pytest
import torch

import ref64
from test_oracle_pose import _K, _rot, expected_Rt, true_F
from vslam_amd import synth

pytestmark = pytest.mark.gpu
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_pose_chain_bit_exact(ctx, oracle):
    B, K, Hy, thr = 5, 400, 128, 10.0
    w, h, f = 1280, 720, 525.0
    Kmat = np.array([[f, 0, w // 2], [0, f, h // 2], [0, 0, 1]], np.float32)       # src/vslam.cpp:32
    xy1 = np.zeros((B, K, 2), np.float32); xy2 = np.zeros((B, K, 2), np.float32)
    pairs = np.zeros((B, K, 2), np.int32); m = np.zeros(B, np.int32)
    sizes = [400, 120, 9, 300, 5]
    for b, n in enumerate(sizes):
        xy1[b], xy2[b], _ = synth.two_view_points(900 + b, K, w, h, inlier_frac=0.75)
        pairs[b, :n] = np.stack([np.arange(n), np.arange(n)], 1)
        m[b] = n
    sets = np.stack([oracle.ransac_sets(30 + b, max(n, 8), Hy) if n >= 8 else np.zeros((Hy, 8), np.int32) for b, n in enumerate(sizes)])
    t = lambda a: torch.from_numpy(a).cuda()
    out = ctx.ransac_fundamental(t(xy1), t(xy2), t(pairs), t(m), t(sets), thr)
    R, tv, c2 = ctx.extract_Rt(out["F"], out["best"], Kmat)
    pts = ctx.triangulate(t(xy1), t(xy2), out["matches"], out["best"], Kmat, c2)
    ids = np.full((B, K), -1, np.int32)
    ids[:, ::7] = 3                                   # some matches are skipped through the match-indexed id test
    ridx, rn, rerr = ctx.reprojection_filter(pts, t(xy1), t(xy2), out["matches"], out["best"], Kmat, c2, t(ids), 4.0)
    ctx.synchronize()
    ridx, rn, rerr = ridx.cpu().numpy(), rn.cpu().numpy(), rerr.cpu().numpy()
    Fh, best, matches = out["F"].cpu().numpy(), out["best"].cpu().numpy(), out["matches"].cpu().numpy()
    R, tv, c2, pts = R.cpu().numpy(), tv.cpu().numpy(), c2.cpu().numpy(), pts.cpu().numpy()
    c1 = np.c_[Kmat, np.zeros(3, np.float32)]
    held = 0
    for b, n in enumerate(sizes):
        if best[b, 0] < 0:
            assert not R[b].any()                      # nothing accepted: outputs untouched
            continue
        Rr, tr = oracle.extract_Rt(Fh[b], Kmat)
        assert np.array_equal(bits(R[b]), bits(Rr.reshape(9))), b
        assert np.array_equal(bits(tv[b]), bits(tr)), b
        c2r = oracle.camera_matrix(Kmat, Rr, tr)
        assert np.array_equal(bits(c2[b]), bits(c2r.reshape(12))), b
        k = best[b, 3]
        mm = matches[b, :k]
        ref = oracle.triangulate(xy1[b][mm[:, 0]], xy2[b][mm[:, 1]], c1, c2r)
        assert np.array_equal(bits(pts[b, :k]), bits(ref)), b
        kept, err = oracle.reprojection_filter(ref, xy1[b][mm[:, 0]], xy2[b][mm[:, 1]], c1, c2r, ids[b, :k], 4.0)
        assert rn[b] == len(kept) and np.array_equal(ridx[b, :rn[b]], kept), b
        assert rerr[b] == err, b
        st = ref64.hold_pose(Fh[b], Kmat, R[b], tv[b], c2[b], xy1[b][mm[:, 0]], xy2[b][mm[:, 1]], pts[b, :k], ids[b, :k],
                             ridx[b, :rn[b]], rerr[b])
        held += st["points"]
        # and it is a rotation with unit translation
        assert abs(np.linalg.det(Rr.astype(np.float64)) - 1) < 1e-4 and abs(np.linalg.norm(tr) - 1) < 1e-5
    assert held > 300, "the triangulated points should be held to the float64 DLT"


def test_extract_Rt_degenerate_inputs(ctx, oracle):
    """Rank-deficient / zero / huge F matrices drive the SVD's zero-singular-value branch."""
    Kmat = np.array([[525, 0, 640], [0, 525, 360], [0, 0, 1]], np.float32)
    Fs = np.zeros((6, 9), np.float32)
    Fs[1] = np.eye(3, dtype=np.float32).reshape(9)
    Fs[2, 0] = 1.0
    Fs[3] = np.arange(9, dtype=np.float32) * 1e-6
    Fs[4] = np.array([0, -1e-7, 3e-5, 1e-7, 0, -2e-4, -3e-5, 2e-4, 0], np.float32)     # skew-symmetric: pure translation
    Fs[5] = np.random.default_rng(0).normal(size=9).astype(np.float32) * 1e4
    R, tv, c2 = ctx.extract_Rt(torch.from_numpy(Fs).cuda(), None, Kmat)
    R, tv = R.cpu().numpy(), tv.cpu().numpy()
    for b in range(6):
        Rr, tr = oracle.extract_Rt(Fs[b], Kmat)
        assert np.array_equal(bits(R[b]), bits(Rr.reshape(9))), b
        assert np.array_equal(bits(tv[b]), bits(tr)), b
        ref64.hold_pose(Fs[b], Kmat, R[b], tv[b], c2.cpu().numpy()[b])


def test_pose_recovers_known_motion(ctx):
    """Exact F of known motions on the device: small and large rotations (past 120 degrees the twisted candidate is the one
    the trace rule keeps), t_z ~ 0 (t up to sign), F scaled by 1e-30 .. 1e30.  R and t / |t| hold to ref64 and to the truth;
    then points projected exactly through that motion triangulate back to X / |t|."""
    K = _K()
    Kd = K.astype(np.float64)
    rng = np.random.default_rng(3)
    cases = []
    for ang in (0.5, 5, 20, 60, 100, 130, 150, 170):   # the motion drawn so that exactly one candidate has trace >= 0
        while True:
            R, t = _rot(rng.normal(size=3), np.deg2rad(ang)), rng.normal(size=3) * rng.uniform(0.1, 10)
            th = t / np.linalg.norm(t)
            tr, trw = np.trace(R), np.trace((2 * np.outer(th, th) - np.eye(3)) @ R)
            if (tr >= 0) != (trw >= 0) and min(abs(tr), abs(trw)) > 0.05:
                break
        cases.append((R, t, 1.0))
    assert sum(np.trace(R) < 0 for R, _, _ in cases) >= 3, "the twisted candidate should be exercised"
    for sc in (1e-30, 1e-12, 1e12, 1e30):
        cases.append((_rot([1, 2, 0.5], 0.2), np.array([0.3, -0.2, 0.9]), sc))
    cases.append((_rot([0.2, 1, -0.3], 0.05), np.array([0.8, -0.6, 1e-9]), 1.0))
    Fs = np.stack([true_F(K, R, t, sc).reshape(9) for R, t, sc in cases])
    R, tv, c2 = ctx.extract_Rt(torch.from_numpy(Fs).cuda(), None, K)
    ctx.synchronize()
    R, tv, c2 = R.cpu().numpy(), tv.cpu().numpy(), c2.cpu().numpy()
    c1 = np.c_[Kd, np.zeros(3)].astype(np.float32)
    for b, (Rt, tt, _) in enumerate(cases):
        st = ref64.hold_pose(Fs[b], K, R[b], tv[b], c2[b])
        assert st["rt"], b
        r = ref64.extract_Rt(Fs[b], K)
        Rx, tx = expected_Rt(Rt, tt)
        assert np.abs(R[b].reshape(3, 3) - Rx).max() <= 2 * r["tol"], b
        if r["t_sign"]:
            assert np.abs(tv[b] - tx).max() <= 2 * r["tol"], b
        else:
            assert min(np.abs(tv[b] - tx).max(), np.abs(tv[b] + tx).max()) <= 2 * r["tol"], b
        if b >= 8 or np.trace(Rt) < 0:                  # the twisted pose is not the motion the points were projected with
            continue
        # triangulate points projected exactly through the true motion with the device's own c2: X / |t| comes back
        X = np.c_[rng.uniform(-2, 2, (64, 2)), rng.uniform(3, 20, 64)]
        pr = lambda c: (lambda p: p[:, :2] / p[:, 2:])(np.c_[X, np.ones(64)] @ np.asarray(c, float).T)
        p1, p2 = pr(c1).astype(np.float32), pr(Kd @ np.c_[Rt, tt]).astype(np.float32)
        pts = ctx.triangulate_points(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), c1, c2[b].reshape(3, 4))
        ctx.synchronize()
        pts = pts.cpu().numpy()
        tri = ref64.triangulate(p1, p2, c1, c2[b])
        assert (ref64.homogeneous_error(pts, tri) <= tri["tol"]).all(), b
        Xs = np.c_[X * np.sign(tv[b] @ tt) / np.linalg.norm(tt), np.ones(64)]   # t_z >= 0 turns the scene round when t_z < 0
        Xs /= np.linalg.norm(Xs, axis=1, keepdims=True)
        u = np.c_[pts[:, :3], np.ones(64)].astype(np.float64)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        assert (np.linalg.norm(u - Xs, axis=1) <= (1 + tri["cond"]) * (ref64.C_X * ref64.EPS + 2 * r["tol"])).all(), b
