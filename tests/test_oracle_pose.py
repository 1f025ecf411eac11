"""The oracle's pose stages (oracle/vso_pose.cpp: extract_Rt, the camera matrix, triangulate, the reprojection filter) held to
the float64 restatements of tests/ref64.py and to ground truth, within bounds computed from each case's conditioning (the
constants are stated in ref64).  The GPU tests hold the device to the oracle bit for bit; these hold the oracle to the
definition."""
import numpy as np
import pytest

import ref64


def _rot(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * k @ k


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _K(f=525.0, w=1280, h=720):
    return np.array([[f, 0, w // 2], [0, f, h // 2], [0, 0, 1]], np.float32)


def true_F(K, R, t, scale=1.0):
    """F of x2^T F x1 = 0 for X2 = R X1 + t: K^-T [t]x R K^-1 (what E = K^T F K undoes)."""
    Ki = np.linalg.inv(np.asarray(K, float))
    return (Ki.T @ _skew(t) @ R @ Ki * scale).astype(np.float32)


def expected_Rt(R, t):
    """Ground truth of extract_Rt on an exact F: t / |t| with t_z >= 0, and whichever of R and the twisted candidate
    (2 t t^T - I) R the trace rule keeps (the one with trace >= 0)."""
    th = t / np.linalg.norm(t)
    twisted = (2 * np.outer(th, th) - np.eye(3)) @ R
    return (R if np.trace(R) >= 0 else twisted), th * (1 if th[2] >= 0 else -1)


def _check_rt(oracle, F, K, R_true=None, t_true=None):
    """Hold oracle.extract_Rt(F, K) to ref64 (decided parts only) and, given the truth, ref64 to the truth.  Returns the
    largest error / bound ratio and the ref64 dict."""
    Ro, to = oracle.extract_Rt(F, K)
    r = ref64.extract_Rt(F, K)
    er, et = ref64.rt_errors(r, Ro, to)
    worst = max(er or 0.0, et or 0.0) / r["tol"]
    assert worst <= 1.0, (F.tolist(), er, et, r["tol"])
    if R_true is not None:
        Rx, tx = expected_Rt(R_true, t_true)
        assert r["rot_decided"] and r["t_sign"], (r["traces"], r["t"])
        assert np.abs(r["R_expected"] - Rx).max() <= r["tol"], "ref64 misses the true rotation"
        assert np.abs(r["t"] - tx).max() <= r["tol"], "ref64 misses the true translation"
        assert np.abs(Ro - Rx).max() <= 2 * r["tol"] and np.abs(to - tx).max() <= 2 * r["tol"], (Ro, Rx, to, tx)
    return worst, r


def test_extract_Rt_recovers_true_motion(oracle):
    """1500 exact fundamental matrices K^-T [t]x R K^-1 (rotations up to 30 degrees, F scaled by 10^-6 .. 10^6, rounded to
    f32): the oracle returns R and t / |t| (t_z >= 0) within C_RT * 2^-23 * (1 + s1 / (s2 - s3))."""
    rng = np.random.default_rng(20261016)
    worst = 0.0
    for _ in range(1500):
        K = _K(float(rng.choice([300.0, 525.0, 1000.0])))
        R = _rot(rng.normal(size=3), np.deg2rad(rng.uniform(0, 30)))
        t = rng.normal(size=3)
        F = true_F(K, R, t, 10.0 ** rng.uniform(-6, 6))
        w, _ = _check_rt(oracle, F, K, R, t)
        worst = max(worst, w)
    assert worst > 0.001, "the bound should not be vacuous"


def test_extract_Rt_twisted_candidate_above_120_degrees(oracle):
    """Past 120 degrees trace(R) < 0 and the trace rule keeps the twisted candidate (2 t t^T - I) R instead of R."""
    rng = np.random.default_rng(7)
    K = _K()
    twisted = 0
    for ang in (125, 140, 160, 175):
        for _ in range(20):
            R = _rot(rng.normal(size=3), np.deg2rad(ang))
            t = rng.normal(size=3)
            th = t / np.linalg.norm(t)
            tw = (2 * np.outer(th, th) - np.eye(3)) @ R
            if min(abs(np.trace(tw)), abs(np.trace(R))) < 0.05 or (np.trace(tw) >= 0) == (np.trace(R) >= 0):
                continue                                   # only scenes where exactly one candidate has trace >= 0
            _check_rt(oracle, true_F(K, R, t), K, R, t)
            twisted += 1
    assert twisted >= 30


def test_extract_Rt_translation_in_the_image_plane(oracle):
    """t_z ~ 0: the sign rule of src/helpers.cpp:31 is a coin flip and ref64 says so; R and t up to sign still hold."""
    K = _K()
    for tz in (0.0, 1e-9, -1e-9):
        for ang in (0.0, 3.0, 20.0):
            R = _rot([0.2, 1.0, -0.3], np.deg2rad(ang))
            t = np.array([0.8, -0.6, tz])
            F = true_F(K, R, t)
            _, r = _check_rt(oracle, F, K)
            assert r["rot_decided"] and r["t_separated"] and not r["t_sign"]
            Ro, to = oracle.extract_Rt(F, K)
            assert np.abs(Ro - R).max() <= 2 * r["tol"]
            assert min(np.abs(to - t).max(), np.abs(to + t).max()) <= 2 * r["tol"]


def test_extract_Rt_pure_rotation_and_scale_extremes(oracle):
    """t = 0 gives F = 0: nothing is decided, and the oracle still returns a rotation and a unit vector.  Exact F at scales
    10^-30 .. 10^30 (E stays within f32) are recovered like any other."""
    K = _K()
    r = ref64.extract_Rt(np.zeros((3, 3), np.float32), K)
    assert not (r["rot_decided"] or r["t_separated"])
    Ro, to = oracle.extract_Rt(np.zeros((3, 3), np.float32), K)
    assert abs(np.linalg.det(Ro.astype(float)) - 1) < 1e-5 and abs(np.linalg.norm(to) - 1) < 1e-6
    R = _rot([1.0, 2.0, 0.5], np.deg2rad(12))
    t = np.array([0.3, -0.2, 0.9])
    for scale in (1e-30, 1e-20, 1e-8, 1e8, 1e20, 1e30):
        _check_rt(oracle, true_F(K, R, t, scale), K, R, t)


def test_extract_Rt_on_any_F(oracle):
    """Generic, rank-1, zero-row, skew-symmetric and zero F over 10^-8 .. 10^8 (the shapes tests/fuzz_pose.py feeds the
    device): every part ref64 decides holds; the undecided ones (rank < 2, exact zero rows) are counted."""
    rng = np.random.default_rng(11)
    decided = total = 0
    for i in range(1200):
        K = _K(float(rng.choice([300.0, 525.0, 1000.0])))
        kind = i % 6
        if kind == 0:
            M = rng.normal(size=(3, 3))
        elif kind == 1:
            M = np.linalg.inv(K.astype(float)).T @ _skew(rng.normal(size=3)) @ _rot(rng.normal(size=3), rng.uniform(0, np.pi)) \
                @ np.linalg.inv(K.astype(float))
        elif kind == 2:
            M = np.outer(rng.normal(size=3), rng.normal(size=3))
        elif kind == 3:
            M = rng.normal(size=(3, 3)); M[i % 3] = 0
        elif kind == 4:
            M = _skew(rng.normal(size=3))
        else:
            M = np.zeros((3, 3))
        _, r = _check_rt(oracle, (M * 10.0 ** rng.uniform(-8, 8)).astype(np.float32), K)
        total += 1
        decided += r["rot_decided"]
    assert decided > total // 3, (decided, total)


def test_extract_Rt_trace_rule_on_the_svd_labels(oracle):
    """Where both candidates' traces have the same sign, which one src/helpers.cpp:29 keeps depends on the SVD's labels,
    not on E.  Restate :13-29 in float64 on the oracle SVD's own factors of E and check the candidate it keeps.  K = I, so
    E = F exactly and the SVD sees the matrix extract_Rt decomposes."""
    rng = np.random.default_rng(5)
    K = np.eye(3, dtype=np.float32)
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    seen = 0
    for _ in range(400):
        F = rng.normal(size=(3, 3)).astype(np.float32)
        _, U, Vt = oracle.svd(F)
        U, Vt = U.astype(np.float64), Vt.astype(np.float64)
        R1 = U @ W @ Vt; R1 = -R1 if np.linalg.det(R1) < 0 else R1
        R2 = U @ W.T @ Vt; R2 = -R2 if np.linalg.det(R2) < 0 else R2
        tr1, tr2 = np.trace(R1), np.trace(R2)
        if (tr1 >= 0) != (tr2 >= 0) or min(abs(tr1), abs(tr2)) < 0.05 or np.abs(R1 - R2).max() < 0.1:
            continue
        Ro, _ = oracle.extract_Rt(F, K)
        want = R2 if tr1 < 0 else R1
        assert np.abs(Ro - want).max() < 1e-3, (tr1, tr2)
        seen += 1
    assert seen > 50


def test_camera_matrix(oracle):
    rng = np.random.default_rng(3)
    for _ in range(200):
        K = _K(float(rng.choice([300.0, 525.0, 1000.0])), int(rng.choice([320, 1280])), int(rng.choice([240, 720])))
        R = _rot(rng.normal(size=3), rng.uniform(0, np.pi)).astype(np.float32)
        t = (rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
        c2, tol = ref64.camera_matrix(K, R, t)
        assert (np.abs(oracle.camera_matrix(K, R, t) - c2) <= tol).all()


# ------------------------------------------------------------------------------------------------------- triangulate
def _project(c, X):
    p = np.c_[X, np.ones(len(X))] @ np.asarray(c, float).T
    return p[:, :2] / p[:, 2:]


def test_triangulate_exact_projections(oracle):
    """Exact projections into three camera pairs: the oracle is within C_X * 2^-23 * (1 + s1 / (s3 - s4)) of the float64 DLT
    (as unit homogeneous vectors), and the DLT recovers the true X."""
    rng = np.random.default_rng(2)
    K = _K().astype(float)
    c1 = np.c_[K, np.zeros(3)].astype(np.float32)
    worst = 0.0
    for R, t in ((_rot([0, 1, 0], 0.05), [1.0, 0, 0]), (_rot([1, 2, 3], 0.3), [0.2, -0.5, 0.8]), (np.eye(3), [0, 0, 1.0])):
        c2 = (K @ np.c_[R, t]).astype(np.float32)
        X = np.c_[rng.uniform(-3, 3, (500, 2)), rng.uniform(2, 40, 500)]
        p1 = _project(c1, X).astype(np.float32)
        p2 = _project(c2, X).astype(np.float32)
        r = ref64.triangulate(p1, p2, c1, c2)
        assert not r["at_inf"].any()
        e = ref64.homogeneous_error(oracle.triangulate(p1, p2, c1, c2), r)
        assert (e <= r["tol"]).all(), (e / r["tol"]).max()
        worst = max(worst, float((e / r["tol"]).max()))
        v = np.c_[X, np.ones(len(X))]
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        assert (np.linalg.norm(v - r["v"], axis=1) <= r["tol"]).all(), "the float64 DLT misses the true point"
    assert worst > 1e-3


def test_pose_chain_recovers_scaled_points(oracle):
    """F from a known motion -> extract_Rt -> camera matrix -> triangulate, all in the oracle: the points come back as X / |t|
    (extract_Rt returns a unit translation), within the conditioning bound widened by the pose error carried into c2."""
    rng = np.random.default_rng(4)
    K = _K()
    Kd = K.astype(float)
    c1 = np.c_[Kd, np.zeros(3)].astype(np.float32)
    for _ in range(20):
        R = _rot(rng.normal(size=3), np.deg2rad(rng.uniform(2, 20)))
        t = rng.normal(size=3); t[2] = abs(t[2]) + 0.1
        t *= rng.uniform(0.1, 10)
        X = np.c_[rng.uniform(-2, 2, (60, 2)), rng.uniform(3, 20, 60)]
        p1 = _project(c1, X).astype(np.float32)
        p2 = _project(Kd @ np.c_[R, t], X).astype(np.float32)
        F = true_F(K, R, t)
        Ro, to = oracle.extract_Rt(F, K)
        rt = ref64.extract_Rt(F, K)
        c2 = oracle.camera_matrix(K, Ro, to)
        pts = oracle.triangulate(p1, p2, c1, c2)
        r = ref64.triangulate(p1, p2, c1, c2)
        Xs = np.c_[X / np.linalg.norm(t), np.ones(len(X))]
        Xs /= np.linalg.norm(Xs, axis=1, keepdims=True)
        # the pose error moves c2 by ~tol_Rt relative, which a point's DLT amplifies by its own (1 + s1 / (s3 - s4))
        bound = (1 + r["cond"]) * (ref64.C_X * ref64.EPS + 2 * rt["tol"])
        u = np.c_[pts[:, :3], np.ones(len(pts))].astype(float)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        e = np.linalg.norm(u - Xs, axis=1)
        assert (e <= bound).all(), (e / bound).max()


def test_triangulate_degenerate_pairs(oracle):
    """The pairs tests/fuzz_pose.py feeds the device: perturbed, coincident (p2 = p1), half at the principal point, 50x
    outside the image, rounded to integers.  Every point not at infinity holds to the float64 DLT."""
    rng = np.random.default_rng(9)
    held = 0
    for case in range(60):
        K = _K(float(rng.choice([300.0, 525.0, 1000.0]))).astype(float)
        R2, t2 = _rot(rng.normal(size=3), np.deg2rad(rng.uniform(0, 3))), rng.normal(size=3) * 0.2
        c1 = np.c_[K, np.zeros(3)].astype(np.float32)
        c2 = (K @ np.c_[R2, t2]).astype(np.float32)
        n = int(rng.choice([1, 7, 65, 300]))
        X = np.c_[rng.uniform(-2, 2, (n, 2)), rng.uniform(2, 12, n)]
        p1, p2 = _project(c1, X), _project(c2, X)
        mode = case % 5
        if mode == 1:
            p2 = p2 + rng.normal(0, 3.0, p2.shape)
        elif mode == 2:
            p2 = p1.copy()
        elif mode == 3:
            p1[: n // 2] = [K[0, 2], K[1, 2]]
        elif mode == 4:
            p1 = p1 * 50
        p1 = (np.rint(p1) if case % 2 else p1).astype(np.float32)
        p2 = (np.rint(p2) if case % 3 else p2).astype(np.float32)
        r = ref64.triangulate(p1, p2, c1, c2)
        e = ref64.homogeneous_error(oracle.triangulate(p1, p2, c1, c2), r)
        ok = ~r["at_inf"] & (r["tol"] < 1e-2)
        assert (e[ok] <= r["tol"][ok]).all(), (case, (e[ok] / r["tol"][ok]).max())
        held += int(ok.sum())
    assert held > 2000


# ------------------------------------------------------------------------------------------------ reprojection filter
def _filter_scene(rng, n, depth_one):
    """c1 = [K | 0], c2 = K [I | t] with t along x so both views see the same depth.  Rows in `depth_one` sit at depth
    exactly 1 (h = 1: dividing changes nothing); the others at depth 3..9, where an undivided row lands pixels away."""
    K = _K(500.0, 640, 480).astype(float)
    c1 = np.c_[K, np.zeros(3)].astype(np.float32)
    c2 = (K @ np.c_[np.eye(3), [0.25, 0, 0]]).astype(np.float32)
    z = np.where(depth_one, 1.0, rng.uniform(3, 9, n))
    X = np.c_[rng.uniform(-0.3, 0.3, (n, 2)) * z[:, None], z]
    p1 = _project(c1, X) + rng.uniform(-1.2, 1.2, (n, 2))
    p2 = _project(c2, X) + rng.uniform(-1.2, 1.2, (n, 2))
    far = rng.random(n) < 0.15
    p2[far] += rng.choice([-4.0, 4.0], (int(far.sum()), 2))
    pts = np.c_[X, np.ones(n)].astype(np.float32)
    return pts, p1.astype(np.float32), p2.astype(np.float32), c1, c2


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 65, 300])
def test_reprojection_filter(oracle, n):
    """Kept set and error sum of the oracle against ref64's restatement, at sizes around the ceil(N/3) de-homogenise quirk, with
    map point ids < 0, = 0 (not skipped: the test is > 0) and > 0 at the match index.  Depth-1 rows pass whether divided or
    not; deeper rows pass only among the first ceil(N/3), so the quirk shapes the kept set, and the scene is asserted free of
    borderline decisions."""
    rng = np.random.default_rng(100 + n)
    depth_one = rng.random(n) < 0.4
    pts, p1, p2, c1, c2 = _filter_scene(rng, n, depth_one)
    ids = rng.choice(np.array([-1, -1, 0, 0, 3, 12], np.int32), n)
    r = ref64.reprojection_filter(pts, p1, p2, c1, c2, ids, 4.0)
    assert r["slack"] > 1, "the scene has a borderline decision"
    kept, err = oracle.reprojection_filter(pts, p1, p2, c1, c2, ids, 4.0)
    assert np.array_equal(kept, r["kept"]), (kept, r["kept"])
    assert abs(err - r["err"]) <= r["err_tol"]
    if n >= 7:
        # what the quirk does here: an undivided deep row never passes, a depth-1 row can
        undivided = ~r["divided"]
        assert not np.isin(np.nonzero(undivided & ~depth_one)[0], r["kept"]).any()
        assert np.isin(np.nonzero(undivided & depth_one)[0], r["kept"]).any()
        assert (ids[r["kept"]] == 0).any(), "an id of 0 must not skip the match"


def test_reprojection_filter_ties_are_kept(oracle):
    """re == thresholdSq exactly (all arithmetic exact: integer pixels, h = 1): `re1 > thresholdSq` rejects only above."""
    c = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    pts = np.array([[10, 20, 1, 1], [30, 40, 1, 1], [50, 60, 1, 1], [70, 80, 1, 1]], np.float32)
    p1 = pts[:, :2] + np.array([[2, 0], [0, -2], [1, 1], [2, 1]], np.float32)   # re1 = 4, 4, 2, 5
    p2 = pts[:, :2] + np.array([[0, 2], [0, 0], [-2, 0], [0, 0]], np.float32)   # re2 = 4, 0, 4, 0
    ids = np.full(4, -1, np.int32)
    r = ref64.reprojection_filter(pts, p1, p2, c, c, ids, 4.0)
    assert list(r["kept"]) == [0, 1, 2] and r["err"] == 18.0
    kept, err = oracle.reprojection_filter(pts, p1, p2, c, c, ids, 4.0)
    assert list(kept) == [0, 1, 2] and err == 18.0
