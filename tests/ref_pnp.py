"""vslam_pnp_ransac (include/vslam_pnp.h) restated in numpy float64, written from the header's text -- not from the device code.

The sampler is the header's, in integers.  The minimal solver is this file's own: the quartic is formed by numpy polynomial
arithmetic as the resultant of the two law-of-cosines quadratics, its roots are numpy.roots' (companion-matrix eigenvalues),
and the pose of a root is the least-squares absolute orientation by SVD about the centroid -- where pnp_math.h has Ferrari's
closed form and two orthonormal frames.  So the order of a hypothesis' solutions differs between the two (winner // 4 is
comparable, winner % 4 is not), and an unpolished pose differs by what two formulations of P3P on f32-rounded pixels differ by:
DELTA_PNP.  The count, the key and the choice are the header's; the polish is ref_resect.resect.

Measured here (tests/test_ref_pnp.py re-measures and compares), K = (525, 525, 320, 240), 640 x 480, depths 2 .. 9, keypoints
rounded to f32, outliers uniform random pixels, seeds 0 .. 19 of every configuration of CONFIGS: the winner's inlier set equals
the planted set on every seed; no planted outlier within 2 inlier_px of its true projection.
  unpolished pose against the truth: at most RAW_WORST (R entries and T entries, T in scene units of 2 .. 9), RAW_BOUND = 4 x;
  polished: error / (2^-23 max|P|) at most POLISH_WORST_RATIO; POLISH_BOUND = 4 x that, rounded up (include/vslam_resect.h's
  own rule);
  0.5 px of keypoint noise: the polished camera centre within NOISE_BOUND = 4 x the worst seen of the truth, in units of
  0.5 px x 9 (the largest depth) / 525 (the focal length) / sqrt(inliers).  The winner itself is not comparable under noise: equally good sets differ.
"""
import numpy as np

import ref_resect as rr

f64 = np.float64
DEFAULTS = dict(hypotheses=128, min_inliers=8, inlier_px=2.0)
DRAWS = 16
ROT_TOL = 1e-9
WIDTH, HEIGHT = 640, 480
CONFIGS = [(12, 0.5, 64, 6), (40, 0.5, 64, 8), (1025, 0.5, 64, 8), (200, 0.5, 128, 8), (200, 0.7, 256, 8)]   # n, outlier share, hypotheses, min_inliers (12 x 0.5 plants 6)
SEEDS = list(range(20))
RAW_WORST = 1.9e-5          # measured (n = 40 seed 7): three f32-rounded pixels fix the pose
RAW_BOUND = 7.6e-5          # 4 x
POLISH_WORST_RATIO = 0.32   # measured (n = 12, where six points carry the pose)
POLISH_BOUND = 1.3
NOISE_WORST_RATIO = 2.96    # measured, n = 200 at 50 %, seeds 0 .. 19
NOISE_BOUND = 12.0
DELTA_PNP = 6.1e-9          # 4 x 1.51e-9: this file against pnp_math.h on the same f32-rounded pixels (tests/test_pnp_serial.py)
M32 = 0xFFFFFFFF


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ------------------------------------------------------------------------------------------------ the sampler
def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def sample(seed, h, n):
    """three distinct indices below n, or None after DRAWS draws"""
    if n < 1:
        return None
    base = mix((seed & M32) ^ ((0x9E3779B9 * (h + 1)) & M32))
    got = []
    for c in range(DRAWS):
        i = (mix((base + c) & M32) * n) >> 32
        if i not in got:
            got.append(i)
            if len(got) == 3:
                return got
    return None


# ------------------------------------------------------------------------------------------------ the minimal solver
def bearings(K, x):
    m = np.linalg.solve(K.reshape(3, 3), np.concatenate([x, np.ones((len(x), 1))], 1).T).T
    return m / np.linalg.norm(m, axis=1, keepdims=True)


def orientation(P, Y, plant=None):
    """least-squares R, T with Y = R P + T (Kabsch about the centroid)"""
    pc, yc = P.mean(0), Y.mean(0)
    U, S, Vt = np.linalg.svd((Y - yc).T @ (P - pc))
    if S[1] < 1e-12 * max(S[0], 1e-300):
        return None   # collinear
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    T = (Y[1] - R @ P[0]) if plant == "t_wrong_point" else (yc - R @ pc)
    return R.reshape(9), T


def p3p(P, f, plant=None):
    """P (3, 3) points, f (3, 3) unit bearings -> [(R (9,), T (3,))], at most 4"""
    with np.errstate(all="ignore"):
        A2, B2, C2 = np.sum((P[1] - P[2]) ** 2), np.sum((P[0] - P[2]) ** 2), np.sum((P[0] - P[1]) ** 2)
        if not (A2 > 0 and B2 > 0 and C2 > 0):
            return []
        ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
        A, C = A2 / B2, C2 / B2
        w = np.array([1.0, -2.0 * cb, 1.0])                      # v^2 - 2 cb v + 1 = |P0 - P2|^2 / s0^2
        p0 = np.polysub(np.array([1.0, 0.0, 0.0]), A * w)        # u^2 + p1 u + p0: (s1, s2) against |P1 - P2|
        p1 = np.array([-2.0 * ca, 0.0])
        q0 = np.polysub(np.array([1.0]), C * w)                  # u^2 + q1 u + q0: (s0, s1) against |P0 - P1|
        q1 = np.array([-2.0 * cg])
        d, e = np.polysub(q0, p0), np.polysub(q1, p1)
        quartic = np.polysub(np.polymul(d, d), np.polymul(e, np.polysub(np.polymul(p1, q0), np.polymul(p0, q1))))
        if not np.isfinite(quartic).all() or quartic[0] == 0:
            return []
        out = []
        for root in np.roots(quartic):
            if abs(root.imag) > 1e-7 * max(1.0, abs(root.real)):
                continue
            v = root.real
            u = -np.polyval(d, v) / np.polyval(e, v)
            s0 = np.sqrt(B2 / np.polyval(w, v))
            s = np.array([s0, u * s0, v * s0])
            if not (np.isfinite(s).all() and (s > 0).all()):
                continue
            got = orientation(P, s[:, None] * f, plant)
            if got is None:
                continue
            R, T = got
            if not (np.isfinite(R).all() and np.isfinite(T).all()):
                continue
            if np.abs(R.reshape(3, 3).T @ R.reshape(3, 3) - np.eye(3)).max() > ROT_TOL:
                continue
            # a complex pair numpy reports as two nearly real roots gives distances that do not reproduce the triangle
            Y = s[:, None] * f
            if abs(np.sum((Y[1] - Y[2]) ** 2) - A2) > 1e-6 * A2 or abs(np.sum((Y[0] - Y[1]) ** 2) - C2) > 1e-6 * C2:
                continue
            out.append((R, T))
        return out[:4]


# ------------------------------------------------------------------------------------------------ the count and the choice
def inlier_mask(K, R, T, P, x, inlier_px, plant=None):
    _, Y, u, v, _, r0, r1, _ = rr.residuals(K, R, T, P, x)
    with np.errstate(all="ignore"):
        d2 = r0 * r0 + r1 * r1
        thr = f64(inlier_px) * f64(inlier_px)
        inside = (d2 < thr) if plant == "open_disc" else (d2 <= thr)
        return (Y[:, 2] > 0.0) & np.isfinite(u) & np.isfinite(v) & inside


def pnp_ransac(points, xy, n, K, seed, R_in, T_in, polish=None, plant=None, **kw):
    """points (S, 3) f64, xy (S, 2) f32, n, K 3 x 3 f32, seed, the bits an item left alone keeps.  polish: None or a dict of
    vslam_resect_params fields.  -> dict(found, winner_h, counts [hypotheses] of lists, inlier (S,) int32, n_inliers, corr_index,
    R_raw, T_raw (before the polish), R, T, stats)"""
    p = params(**kw)
    S = len(points)
    n = min(max(int(n), 0), S)
    P = np.asarray(points, f64).reshape(-1, 3)[:n]
    x = np.asarray(xy, np.float32).astype(f64).reshape(-1, 2)[:n]
    Kv = np.asarray(K, np.float32).astype(f64).reshape(9)
    Ri, Ti = np.array(R_in, f64).reshape(9), np.array(T_in, f64).reshape(3)
    nan = float("nan")
    res = dict(found=False, winner_h=-1, counts=[[] for _ in range(p["hypotheses"])], inlier=np.zeros(S, np.int32), n_inliers=0,
               corr_index=np.zeros(0, np.int32), R_raw=Ri, T_raw=Ti, R=Ri.copy(), T=Ti.copy(), stats=np.full(4, nan))
    if n < 4 or not (np.isfinite(P).all() and np.isfinite(x).all() and np.isfinite(Kv).all()):
        return res
    f_all = bearings(Kv, x)
    best = None   # (count, -(4 h + s)) maximal
    for h in range(p["hypotheses"]):
        idx = sample(seed, h, n)
        if idx is None:
            continue
        for s, (R, T) in enumerate(p3p(P[idx], f_all[idx], plant)):
            c = int(inlier_mask(Kv, R, T, P, x, p["inlier_px"], plant).sum())
            res["counts"][h].append(c)
            key = (c, (4 * h + s) if plant == "tie_larger" else -(4 * h + s))
            if best is None or key > best[0]:
                best = (key, h, R, T)
    if best is None or best[0][0] < p["min_inliers"]:
        return res
    _, h, R, T = best
    mask = inlier_mask(Kv, R, T, P, x, p["inlier_px"], plant)
    res.update(found=True, winner_h=h, R_raw=R, T_raw=T, R=R.copy(), T=T.copy(), n_inliers=int(mask.sum()),
               corr_index=np.flatnonzero(mask).astype(np.int32))
    res["inlier"][:n] = mask
    if polish is not None:
        R2, T2, stats, info = rr.resect(P[mask], np.asarray(xy, np.float32).reshape(-1, 2)[:n][mask], K, R, T, **polish)
        res.update(R=R2, T=T2, stats=stats)
        if plant == "mask_after_polish":
            m2 = inlier_mask(Kv, R2, T2, P, x, p["inlier_px"])
            res["inlier"][:n] = m2
            res.update(n_inliers=int(m2.sum()), corr_index=np.flatnonzero(m2).astype(np.int32))
    return res


# ------------------------------------------------------------------------------------------------ scenes
def rotation(rng, max_deg):
    w = rng.normal(size=3)
    w = w / np.linalg.norm(w) * np.deg2rad(rng.uniform(0.2, 1.0) * max_deg)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx


def planted(n, outliers, seed, noise_px=0.0, planar=False, inlier_px=2.0):
    """-> dict(points (n, 3) f64, xy (n, 2) f32, K, R (9,), T (3,), planted (n,) bool: the correspondences left exact, margin: the
    smallest distance of a replaced keypoint to its true projection)"""
    rng = np.random.default_rng(1000 * n + seed)
    K = rr.kmat()
    Kd = K.astype(f64)
    R = rotation(rng, 40.0)
    T = rng.uniform(-1.0, 1.0, 3)
    px = np.stack([rng.uniform(20, WIDTH - 20, n), rng.uniform(20, HEIGHT - 20, n), np.ones(n)], 1)
    rays = np.linalg.solve(Kd, px.T).T
    if planar:
        nrm = np.array([0.2, -0.1, 1.0])
        depth = (5.0 / (rays @ nrm))[:, None]
    else:
        depth = rng.uniform(2.0, 9.0, (n, 1))
    P = (rays * depth - T) @ R       # R^t (Y - T), row-wise
    _, _, u, v, _, _, _, _ = rr.residuals(Kd.reshape(9), R.reshape(9), T, P, np.zeros((n, 2)))
    true_xy = np.stack([u, v], 1)
    xy = true_xy + (rng.normal(size=(n, 2)) * noise_px if noise_px else 0.0)
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    xy[out] = np.stack([rng.uniform(0, WIDTH, out.sum()), rng.uniform(0, HEIGHT, out.sum())], 1)
    xy = xy.astype(np.float32)
    margin = float(np.linalg.norm(xy[out].astype(f64) - true_xy[out], axis=1).min()) if out.any() else np.inf
    return dict(points=P, xy=xy, K=K, R=R.reshape(9), T=T, planted=~out, margin=margin, n=n)


def pose_error(R, T, sc):
    return max(float(np.abs(R - sc["R"]).max()), float(np.abs(T - sc["T"]).max()))


def centre(R, T):
    return -(R.reshape(3, 3).T @ T)


# ------------------------------------------------------------------------------------------------ world points to keypoints
MATCH_DEFAULTS = dict(dist_threshold=64, ratio10=8)


def match_points(points, n_points, offsets, obs_desc, xy, desc, n_kp, taken=None, **kw):
    """vslam_match_points: tests/ref_search.py's search_item restricted as the header says -- no visibility, no disc.  The rule is
    run on stand-ins that make both always true (every finite point at (0, 0, 1) under the identity, every keypoint at the pixel
    it projects to), so d, the choice, the proposal rule and the resolution are ref_search's own code; the compacted rows are
    then copied from the real arrays.  -> search_item's dict; stats[0] counts the points taking part."""
    import ref_search as rs
    p = dict(MATCH_DEFAULTS)
    p.update(kw)
    points = np.asarray(points, np.float32).reshape(-1, 4)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    stand_in = np.zeros_like(points)
    stand_in[:, 2] = 1.0
    stand_in[~np.isfinite(points[:, :3]).all(1), 0] = np.nan
    r = rs.search_item(stand_in, n_points, offsets, obs_desc, np.eye(3).reshape(9), np.zeros(3), np.eye(3, dtype=np.float32), 1, 1,
                       np.zeros_like(xy), desc, n_kp, taken, radius_px=1.0, **p)
    r["corr_points"] = points[r["corr_point"], :3].astype(f64)
    r["corr_xy"] = xy[r["corr_kp"]].copy()
    return r
