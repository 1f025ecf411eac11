"""float64 reference of vslam_refit_fundamental, written from the contract in include/vslam_amd.h and from
src/RansacFilter.cpp:81-89 (the order of A's columns) -- not from the device code.

refit(xy1, xy2, matches, F_in) fits F over ALL the given correspondences in two independent ways that share only the
normalised design matrix A:
  eigh   the eigenvector of the smallest eigenvalue of A^t A (what the device forms);
  svd    the right singular vector of the smallest singular value of A itself (never squares the condition).
Both then take the rank-2 step through numpy's SVD, denormalise, scale to unit Frobenius norm, take F_in's sign and round once
to f32.  The eigh form is the reference proper; the svd form measures how far two correct float64 formulations are apart
(stats["delta"]), which is what the device comparison's tolerance is built from.
"""
import numpy as np

GAP_BOUND = 1e-6      # (lambda_8 - lambda_9) / lambda_1 below this: the null vector is not isolated enough to compare entries


def sampson(F, p1, p2):
    """True Sampson distance e^2 / (Fx1_0^2 + Fx1_1^2 + Ftx2_0^2 + Ftx2_1^2) per correspondence; p1, p2 (n, 2)."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    x1 = np.c_[np.asarray(p1, np.float64), np.ones(len(p1))]
    x2 = np.c_[np.asarray(p2, np.float64), np.ones(len(p2))]
    a = x1 @ F.T          # rows F x1
    b = x2 @ F            # rows F^t x2
    e = (x2 * a).sum(1)
    with np.errstate(all="ignore"):
        return e * e / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


def _hartley(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    if not d > 0:
        return None, d
    s = np.sqrt(2.0) / d
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]]), d


def _finish(f, T1, T2, F_in):
    Fh = f.reshape(3, 3)
    U, s, Vt = np.linalg.svd(Fh)
    Fh = (U[:, :2] * s[:2]) @ Vt[:2]
    F = T2.T @ Fh @ T1
    F = F / np.sqrt((F * F).sum())
    if (F * F_in).sum() < 0:
        F = -F
    return F


def refit(xy1, xy2, matches, F_in, kp_stride=None, winner=0):
    """xy1, xy2 (K, 2) f32, matches (n, 2) the compacted inlier matches, F_in (9,) or (3, 3) f32.
    Returns F (3, 3) float32 and stats: dict(stats=(4,) f64 as d_stats holds them, skipped, F64 (eigh form, unrounded),
    F64_svd, delta = max |F64 - F64_svd|, gap = (lambda_8 - lambda_9) / lambda_1, comparable = gap >= GAP_BOUND)."""
    xy1 = np.asarray(xy1, np.float32).astype(np.float64).reshape(-1, 2)
    xy2 = np.asarray(xy2, np.float32).astype(np.float64).reshape(-1, 2)
    K = kp_stride if kp_stride is not None else max(len(xy1), len(xy2))
    m = np.asarray(matches, np.int64).reshape(-1, 2)
    F32_in = np.asarray(F_in, np.float32).reshape(3, 3)
    Fi = F32_in.astype(np.float64)
    ok = (m[:, 0] >= 0) & (m[:, 0] < K) & (m[:, 1] >= 0) & (m[:, 1] < K)
    m = m[ok]
    n = len(m)
    nan = float("nan")

    def skipped():
        return F32_in.copy(), dict(stats=np.array([n, nan, nan, nan]), skipped=True, F64=Fi, F64_svd=Fi, delta=0.0, gap=nan,
                                   comparable=False)
    if winner < 0 or n < 8:
        return skipped()
    p1, p2 = xy1[m[:, 0]], xy2[m[:, 1]]
    T1, d1 = _hartley(p1)
    T2, d2 = _hartley(p2)
    if T1 is None or T2 is None:
        return skipped()
    q1 = np.c_[p1, np.ones(n)] @ T1.T
    q2 = np.c_[p2, np.ones(n)] @ T2.T
    u1, v1, u2, v2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(n)], axis=1)
    if not np.isfinite(A).all():
        return skipped()
    lam, V = np.linalg.eigh(A.T @ A)                    # ascending
    F_e = _finish(V[:, 0], T1, T2, Fi)
    sv, Wt = np.linalg.svd(A, full_matrices=n < 9)[1:]  # descending; Wt is 9 x 9 (n = 8: the full form adds the null direction)
    F_s = _finish(Wt[8], T1, T2, Fi)
    F32 = F_e.astype(np.float32)
    if not (np.isfinite(F32).all() and np.isfinite(F_s).all()):
        return skipped()
    # the gap from the singular values of A (squared): they hold small eigenvalues to full relative accuracy
    ev = np.zeros(9)
    ev[:len(sv)] = sv ** 2
    ev = np.sort(ev)                                   # ascending: ev[0] = lambda_9, ev[1] = lambda_8, ev[8] = lambda_1
    gap = (ev[1] - ev[0]) / ev[8]
    st = np.array([n, sampson(Fi, p1, p2).mean(), sampson(F32.astype(np.float64), p1, p2).mean(),
                   ev[0] / ev[1] if ev[1] > 0 else nan])
    return F32, dict(stats=st, skipped=False, F64=F_e, F64_svd=F_s, delta=float(np.abs(F_e - F_s).max()), gap=float(gap),
                     comparable=bool(gap >= GAP_BOUND), p1=p1, p2=p2)


# ------------------------------------------------------------------------------------------------ inputs
def two_view(seed, n_in, n_held=0, sigma=0.5, w=640, h=480, f=525.0):
    """The generator of the accuracy sketch: a camera of focal f at (w / 2, h / 2), a rotation of about 1 degree about a random
    axis, a baseline of 0.3 in a random direction, depths 3 .. 9; N(0, sigma) pixel noise on both images of the n_in inliers,
    none on the n_held held-out correspondences.  Returns p1, p2 (n_in, 2) f32 noisy, h1, h2 (n_held, 2) f64 exact, F_true."""
    rng = np.random.default_rng(seed)
    Km = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    ang = np.deg2rad(1.0) * rng.uniform(0.8, 1.2)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = rng.normal(size=3); t *= 0.3 / np.linalg.norm(t)

    def views(n):
        z = rng.uniform(3, 9, n)
        px = np.c_[rng.uniform(0, w, n), rng.uniform(0, h, n), np.ones(n)]
        X = (np.linalg.inv(Km) @ px.T).T * z[:, None]
        x2 = (Km @ (R @ X.T + t[:, None])).T
        return px[:, :2], x2[:, :2] / x2[:, 2:]
    a1, a2 = views(n_in)
    h1, h2 = views(n_held)
    p1 = (a1 + rng.normal(0, sigma, a1.shape)).astype(np.float32)
    p2 = (a2 + rng.normal(0, sigma, a2.shape)).astype(np.float32)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ft = np.linalg.inv(Km).T @ tx @ R @ np.linalg.inv(Km)
    return p1, p2, h1, h2, Ft / np.linalg.norm(Ft)


def eight_point_F(p1, p2, idx):
    """F_in as RANSAC hands it over: the un-normalised eight-point fit (ref64.fundamental_8pt) on the 8 correspondences idx."""
    import ref64
    return ref64.fundamental_8pt(p1[idx][None], p2[idx][None])["F"][0].astype(np.float32)


def case(seed, K, n, sigma=0.5):
    """One comparison input: n noisy correspondences among K keypoint slots (shuffled slots, so matches are no identity map),
    F_in from 8 of them.  Returns xy1, xy2 (K, 2) f32, matches (K, 2) int32 (the first n are used), best (4,) int32, F_in (9,)."""
    rng = np.random.default_rng(seed + 7919)
    p1, p2, _, _, _ = two_view(seed, n, 0, sigma)
    xy1 = rng.uniform(0, 640, (K, 2)).astype(np.float32)
    xy2 = rng.uniform(0, 480, (K, 2)).astype(np.float32)
    s1, s2 = rng.permutation(K)[:n], rng.permutation(K)[:n]
    xy1[s1], xy2[s2] = p1, p2
    matches = np.full((K, 2), -7, np.int32)              # slots past n are never read
    matches[:n] = np.stack([s1, s2], 1)
    F_in = eight_point_F(p1, p2, rng.permutation(n)[:8]).reshape(9)
    best = np.array([0, n, 0, n], np.int32)
    return xy1, xy2, matches, best, F_in


# The comparison inputs of tests/test_gpu_refit.py: (kp_stride, n) at which each path of the device sums can go wrong
# (fewer correspondences than lanes, exactly one round of 256, a tail, many rounds, the largest stride).
COMPARISON_SHAPES = [(64, 8), (64, 9), (64, 63), (64, 64), (1024, 255), (1024, 256), (1024, 257), (1024, 1023), (8160, 8160)]
MIXED_BATCH = (1024, [300, 8, 1023, 77, 256, 511, 40])   # several pairs of different n in one batch


def comparison_cases():
    """[(name, xy1, xy2, matches, best, F_in)] -- fixed seeds; shared by the CPU test that records delta_ref and the GPU test."""
    out = []
    for i, (K, n) in enumerate(COMPARISON_SHAPES):
        out.append((f"K{K}_n{n}",) + case(100 + i, K, n))
    K, ns = MIXED_BATCH
    for j, n in enumerate(ns):
        out.append((f"mixed{j}_n{n}",) + case(200 + j, K, n))
    return out


_RESULTS = None


def comparison_results():
    """{name: (F, stats)} of refit() over comparison_cases(), computed once and shared."""
    global _RESULTS
    if _RESULTS is None:
        _RESULTS = {c[0]: refit(c[1], c[2], c[3][:c[4][3]], c[5], kp_stride=len(c[1])) for c in comparison_cases()}
    return _RESULTS


def delta_ref():
    """The largest entry-wise difference of the two formulations over the comparable comparison inputs: 3.6e-12 as measured
    (tests/test_ref_refit.py asserts the order of magnitude); the device comparison allows 16 of these."""
    return max(st["delta"] for _, st in comparison_results().values() if st["comparable"])


def accuracy_pairs(pairs=32, n_in=64, n_held=200, seed=5000):
    """The accuracy claim's inputs: per pair p1, p2 (n_in, 2) noisy, h1, h2 held out and exact, F_in the eight-point fit on 8 of
    the inliers."""
    out = []
    for k in range(pairs):
        p1, p2, h1, h2, _ = two_view(seed + k, n_in, n_held)
        idx = np.random.default_rng(seed + 1000 + k).permutation(n_in)[:8]
        out.append((p1, p2, h1, h2, eight_point_F(p1, p2, idx)))
    return out


def rms_sampson(F, h1, h2):
    return float(np.sqrt(sampson(F, h1, h2).mean()))
