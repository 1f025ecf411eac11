"""float64 reference of vslam_refine_pairs (two-view bundle adjustment of a pair's pose and points), written from the contract in
include/vslam_amd.h -- not from the device code.

refine() is the header's algorithm in numpy float64, vectorised over the points (so its sums run in numpy's order, not the
device's).  second_formulation() minimises the same objective over the same fixed set of correspondences in an independent way,
through scipy.optimize.least_squares(method="lm") with a 6-dof camera (rotation vector and a free t), normalised to |t| = 1
afterwards:
  n <= FULL_VECTOR_MAX   over the full unknown vector (6 + 3 n), dense analytic Jacobian;
  larger n               the dense Jacobian (4 n x (6 + 3 n): 6.4 GB at n = 8160, and 20 s of QR per case at n = 300) is out of
                         reach, so the points are eliminated exactly instead: for each camera the residual is taken at the
                         points that minimise it for that camera (a Newton solve per point), and LM runs over the 6 camera
                         unknowns with the projected Jacobian.  A trial camera far from the minimum breaks the per-point
                         solves, so this form starts from refine()'s result and not from the inputs: it tests that the result
                         is a minimum of the 6-dof problem too, and reports how far LM moves from it.
Both forms share nothing with refine() but the projection and the participation rule; their distance after convergence is what
two correct float64 formulations are apart (delta_ref), which the device comparison's tolerance is built from.
"""
import numpy as np

LAMBDA0 = 1e-3
LAMBDA_MIN = 1e-15
LAMBDA_MAX = 1e12
REL_STOP = 2.0 ** -40
DIAG_FLOOR = 2.0 ** -40
MARGINAL = 1e-9          # a step whose objective ratio is this close to 1 is flagged (info["marginal"])
# The stop rule ends a run on an accepted step whose ratio is within 2^-40 < MARGINAL of 1, and the step before it is usually within
# MARGINAL too (the decreases shrink by a roughly constant factor per step), so nearly every run that converges is flagged.  What
# makes the count of accepted steps reproducible in another summation order is the distance of the closest decision from 1
# against the rounding of the objective's sum (about sqrt(n) 2^-53 relative, 1e-14 at n = 8160): info["margin"] records it and
# a run is DECIDED when it is at least DECIDED_MARGIN.
DECIDED_MARGIN = 1e-13
EIG_BOUND = 1e-9         # smallest / largest eigenvalue of the final undamped S below this: the minimum is too flat to compare entries
FULL_VECTOR_MAX = 100
KMAT = np.array([[525.0, 0, 320.0], [0, 525.0, 240.0], [0, 0, 1.0]], np.float32)   # the camera of ref_refit.two_view


# ------------------------------------------------------------------------------------------------ pieces of the contract
def project(K, Y):
    """q = K Y row by row, (q0 / q2, q1 / q2); Y (n, 3)."""
    q = (K[:, 0] * Y[:, :1] + K[:, 1] * Y[:, 1:2]) + K[:, 2] * Y[:, 2:3]
    with np.errstate(all="ignore"):
        return q[:, :2] / q[:, 2:3], q


def transform(R, t, X):
    return ((R[:, 0] * X[:, :1] + R[:, 1] * X[:, 1:2]) + R[:, 2] * X[:, 2:3]) + t


def errors(K, R, t, X, o1, o2):
    """squared reprojection error per image, (n,), (n,)"""
    u1, _ = project(K, X)
    u2, _ = project(K, transform(R, t, X))
    with np.errstate(all="ignore"):
        return ((u1 - o1) ** 2).sum(1), ((u2 - o2) ** 2).sum(1)


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def rodrigues(w):
    th2 = float(w @ w)
    if th2 < 2.0 ** -26:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = np.sqrt(th2)
        s = np.sin(0.5 * th)
        a, b = np.sin(th) / th, 2.0 * s * s / th2
    W = skew(w)
    return np.eye(3) + a * W + b * (W @ W)


def tangent_basis(t):
    k = int(np.argmin(np.abs(t)))            # the first of equal ones
    e = np.zeros(3); e[k] = 1.0
    b1 = np.cross(t, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return b1, np.cross(t, b1)


def camera(K, R, t):
    Rt = np.c_[R, t]
    return (K[:, :1] * Rt[0] + K[:, 1:2] * Rt[1]) + K[:, 2:3] * Rt[2]


def point_jacobians(K, R, t, X):
    """A1 (n, 2, 3) = d proj1 / dX, A2 (n, 2, 3) = d proj2 / dY, residual-free; and Y, RX."""
    RX = transform(R, np.zeros(3), X)
    Y = RX + t

    def dproj(Yc):
        uv, q = project(K, Yc)
        return (K[None, :2, :] - uv[:, :, None] * K[None, 2:3, :]) / q[:, 2, None, None], uv
    A1, u1 = dproj(X)
    A2, u2 = dproj(Y)
    return A1, A2, u1, u2, RX


def camera_jacobian(A2, RX, b1, b2):
    n = len(RX)
    C = np.zeros((n, 3, 5))
    C[:, 0, 1], C[:, 0, 2] = RX[:, 2], -RX[:, 1]     # -[RX]x
    C[:, 1, 0], C[:, 1, 2] = -RX[:, 2], RX[:, 0]
    C[:, 2, 0], C[:, 2, 1] = RX[:, 1], -RX[:, 0]
    C[:, :, 3], C[:, :, 4] = b1, b2
    return A2 @ C                                      # (n, 2, 5)


def participants(K, R, t, X, o1, o2, gate_sq):
    e1, e2 = errors(K, R, t, X, o1, o2)
    Y = transform(R, t, X)
    with np.errstate(all="ignore"):
        ok = np.isfinite(X).all(1) & (X[:, 2] > 0) & (Y[:, 2] > 0) & (e1 <= gate_sq) & (e2 <= gate_sq)
    return ok, e1, e2


# ------------------------------------------------------------------------------------------------ the header's algorithm
def refine(xy1, xy2, matches, K, R_in, t_in, points4d, gate_sq=16.0, max_iterations=20, kp_stride=None, winner=0):
    """xy1, xy2 (Kp, 2) f32; matches (n, 2) the compacted inlier matches; R_in (3, 3), t_in (3,), points4d (>= n, 4) f32.
    Returns R (3, 3), t (3,), c2 (3, 4), points4d (copy, refined slots replaced), all float32, and info: stats (4,) as d_stats
    holds them, left_alone, part (n,) bool, objective [accepted values, first = start], marginal, margin, last_rel, eig_ratio,
    comparable, singular (indices within the participating points of the final point blocks that are numerically singular: then
    eig_ratio is 0 and the run is not comparable), and the unrounded R64, t64, X64."""
    xy1 = np.asarray(xy1, np.float32).astype(np.float64).reshape(-1, 2)
    xy2 = np.asarray(xy2, np.float32).astype(np.float64).reshape(-1, 2)
    Kp = kp_stride if kp_stride is not None else max(len(xy1), len(xy2))
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    m = np.asarray(matches, np.int64).reshape(-1, 2)[:Kp]
    n = len(m)
    R32 = np.asarray(R_in, np.float32).reshape(3, 3); t32 = np.asarray(t_in, np.float32).reshape(3)
    P32 = np.array(points4d, np.float32).reshape(-1, 4)
    Ri, ti = R32.astype(np.float64), t32.astype(np.float64)
    inr = (m[:, 0] >= 0) & (m[:, 0] < Kp) & (m[:, 1] >= 0) & (m[:, 1] < Kp)
    ms = np.where(inr[:, None], m, 0)
    o1, o2 = xy1[ms[:, 0]], xy2[ms[:, 1]]
    X0 = P32[:n, :3].astype(np.float64)
    ok, e1, e2 = participants(K, Ri, ti, X0, o1, o2, gate_sq)
    part = ok & inr
    cnt = int(part.sum())
    nan = float("nan")
    c2_in = camera(K, Ri, ti).astype(np.float32)

    def alone():
        return R32.copy(), t32.copy(), c2_in, P32.copy(), dict(
            stats=np.array([cnt, nan, nan, nan]), left_alone=True, part=part, objective=[], marginal=False, margin=np.inf, last_rel=nan,
            eig_ratio=nan, comparable=False, singular=np.zeros(0, np.int64), R64=Ri, t64=ti, X64=X0, o1=o1, o2=o2)
    tn = np.sqrt(ti @ ti)
    if winner < 0 or cnt < 8 or not np.isfinite(ti).all() or not tn > 0:
        return alone()
    o1p, o2p = o1[part], o2[part]
    mean_in = float((e1[part] + e2[part]).sum() / (2.0 * cnt))
    # the start: R one Newton step of the polar iteration closer to a rotation, t on the unit sphere
    R = 0.5 * (Ri @ (3.0 * np.eye(3) - Ri.T @ Ri))
    t = ti / tn
    X = X0[part].copy()

    def objective(R, t, X):
        a, b = errors(K, R, t, X, o1p, o2p)
        return float((a + b).sum())
    obj = objective(R, t, X)
    history, lam, accepted, margin, last_rel = [obj], LAMBDA0, 0, np.inf, nan
    for _ in range(max_iterations):
        A1, A2, u1, u2, RX = point_jacobians(K, R, t, X)
        b1, b2 = tangent_basis(t)
        r1, r2 = u1 - o1p, u2 - o2p
        J2x = A2 @ R
        Jc = camera_jacobian(A2, RX, b1, b2)
        V = A1.transpose(0, 2, 1) @ A1 + J2x.transpose(0, 2, 1) @ J2x
        W = Jc.transpose(0, 2, 1) @ J2x                                   # (n, 5, 3)
        U = Jc.transpose(0, 2, 1) @ Jc
        gx = (A1.transpose(0, 2, 1) @ r1[:, :, None] + J2x.transpose(0, 2, 1) @ r2[:, :, None])[:, :, 0]
        gc = (Jc.transpose(0, 2, 1) @ r2[:, :, None])[:, :, 0]
        Vd = V.copy()
        for k in range(3):
            Vd[:, k, k] = V[:, k, k] + lam * np.maximum(V[:, k, k], DIAG_FLOOR)
        step_ok = True
        try:
            L = np.linalg.cholesky(Vd)
            Yv = np.linalg.solve(Vd, W.transpose(0, 2, 1))                # V*^-1 W^t  (n, 3, 5)
            z = np.linalg.solve(Vd, gx[:, :, None])[:, :, 0]
            Us = U.sum(0)
            S = Us + lam * np.diag(np.diag(Us)) - (W @ Yv).sum(0)
            rhs = gc.sum(0) - (W @ z[:, :, None])[:, :, 0].sum(0)
            np.linalg.cholesky(S)
            dc = -np.linalg.solve(S, rhs)
        except np.linalg.LinAlgError:
            step_ok = False
        cand = None
        if step_ok and np.isfinite(dc).all():
            dX = -(z + (Yv @ dc[None, :, None])[:, :, 0])
            Rn = rodrigues(dc[:3]) @ R
            tt = t + dc[3] * b1 + dc[4] * b2
            tnew = tt / np.sqrt(tt @ tt)
            Xn = X + dX
            on = objective(Rn, tnew, Xn)
            Yn = transform(Rn, tnew, Xn)
            with np.errstate(all="ignore"):
                good = np.isfinite(on) and bool((Xn[:, 2] > 0).all()) and bool((Yn[:, 2] > 0).all())
            if good and on < obj:
                cand = (Rn, tnew, Xn, on)
            if good and obj > 0:
                margin = min(margin, abs(on / obj - 1.0))
        if cand is not None:
            last_rel = (obj - cand[3]) / obj
            R, t, X, obj = cand
            history.append(obj)
            accepted += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            if last_rel < REL_STOP:
                break
        else:
            lam = lam * 10.0
            if lam > LAMBDA_MAX:
                break
    if accepted == 0:
        return alone()
    Ro, to = R.astype(np.float32), t.astype(np.float32)
    c2 = camera(K, R, t).astype(np.float32)
    Xo = X.astype(np.float32)
    if not (np.isfinite(Ro).all() and np.isfinite(to).all() and np.isfinite(c2).all() and np.isfinite(Xo).all()):
        return alone()
    P = P32.copy()
    idx = np.nonzero(part)[0]
    P[idx, :3] = Xo
    P[idx, 3] = 1.0
    mean_out = mean_error(K, Ro, to, Xo, o1p, o2p)
    # the final undamped reduced system: how well the minimum is determined
    A1, A2, u1, u2, RX = point_jacobians(K, R, t, X)
    b1, b2 = tangent_basis(t)
    J2x = A2 @ R
    Jc = camera_jacobian(A2, RX, b1, b2)
    V = A1.transpose(0, 2, 1) @ A1 + J2x.transpose(0, 2, 1) @ J2x
    W = Jc.transpose(0, 2, 1) @ J2x
    # A point that ran off to a depth of 1e9 has a block whose depth direction carries nothing (the loop's damping floor keeps
    # it solvable there; this undamped one is not): such a run has no determined minimum to compare entries at.
    singular = singular_blocks(V)
    ratio = 0.0
    if len(singular) == 0:
        try:
            S = (Jc.transpose(0, 2, 1) @ Jc).sum(0) - (W @ np.linalg.solve(V, W.transpose(0, 2, 1))).sum(0)
            if np.isfinite(S).all():
                ev = np.linalg.eigvalsh(S)
                ratio = float(ev[0] / ev[-1])
                ratio = ratio if np.isfinite(ratio) else 0.0
        except np.linalg.LinAlgError:
            ratio = 0.0
    return Ro, to, c2, P, dict(stats=np.array([cnt, mean_in, mean_out, accepted]), left_alone=False, part=part, objective=history,
                               marginal=bool(margin <= MARGINAL), margin=float(margin), last_rel=float(last_rel), eig_ratio=ratio, comparable=bool(ratio >= EIG_BOUND),
                               singular=singular, R64=R, t64=t, X64=X, o1=o1, o2=o2)


def singular_blocks(V):
    """Indices (within the participating points) of the undamped 3 x 3 point blocks that are non-finite or numerically singular
    in float64: smallest eigenvalue not above 2^-52 of the largest."""
    fin = np.isfinite(V).all((1, 2))
    ev = np.linalg.eigvalsh(np.where(fin[:, None, None], V, np.eye(3)))
    return np.nonzero(~fin | ~(ev[:, 0] > 2.0 ** -52 * ev[:, -1]))[0]


def mean_error(K, R, t, X, o1, o2):
    """d_stats[2]'s expression: the mean squared reprojection error of the given (f32) values, widened."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    a, b = errors(K, np.asarray(R, np.float32).astype(np.float64).reshape(3, 3), np.asarray(t, np.float32).astype(np.float64).reshape(3),
                  np.asarray(X, np.float32).astype(np.float64).reshape(-1, 3), o1, o2)
    return float((a + b).sum() / (2.0 * len(o1)))


# ------------------------------------------------------------------------------------------------ the second formulation
def second_formulation(K, R_start, t_start, X_start, o1, o2):
    """The minimum of the same objective through scipy's LM with a 6-dof camera: returns R, t (|t| = 1), X (rescaled)."""
    from scipy.optimize import least_squares
    K = np.asarray(K, np.float64)
    n = len(X_start)
    tiny = 1e-15

    def cam(p):
        return rodrigues(p[:3]) @ R_start, p[3:6]

    def resid_jac(R, t, X):
        A1, A2, u1, u2, RX = point_jacobians(K, R, t, X)
        return u1 - o1, u2 - o2, A1, A2, A2 @ R, RX

    def cam_block(A2, RX, R, p):
        # d Y / d p: Y = exp(p_w) R0 X + t; to first order around the CURRENT p the rotation update is left-multiplied by the
        # left Jacobian of SO(3), Jl(p_w)
        w = p[:3]
        th2 = float(w @ w)
        Wm = skew(w)
        if th2 < 1e-16:
            Jl = np.eye(3) + 0.5 * Wm
        else:
            th = np.sqrt(th2)
            Jl = np.eye(3) + (1 - np.cos(th)) / th2 * Wm + (th - np.sin(th)) / (th2 * th) * (Wm @ Wm)
        C = np.zeros((len(RX), 3, 6))
        C[:, 0, 1], C[:, 0, 2] = RX[:, 2], -RX[:, 1]
        C[:, 1, 0], C[:, 1, 2] = -RX[:, 2], RX[:, 0]
        C[:, 2, 0], C[:, 2, 1] = RX[:, 1], -RX[:, 0]
        C[:, :, :3] = C[:, :, :3] @ Jl
        C[:, :, 3:] = np.eye(3)
        return A2 @ C                                                    # (n, 2, 6)

    if n <= FULL_VECTOR_MAX:
        def f(p):
            R, t = cam(p)
            r1, r2, *_ = resid_jac(R, t, p[6:].reshape(n, 3))
            return np.concatenate([r1, r2], 1).ravel()

        def jac(p):
            R, t = cam(p)
            r1, r2, A1, A2, J2x, RX = resid_jac(R, t, p[6:].reshape(n, 3))
            Jc = cam_block(A2, RX, R, p)
            J = np.zeros((4 * n, 6 + 3 * n))
            for i in range(n):
                J[4 * i + 2: 4 * i + 4, :6] = Jc[i]
                J[4 * i: 4 * i + 2, 6 + 3 * i: 9 + 3 * i] = A1[i]
                J[4 * i + 2: 4 * i + 4, 6 + 3 * i: 9 + 3 * i] = J2x[i]
            return J
        p0 = np.concatenate([np.zeros(3), t_start, X_start.ravel()])
        sol = least_squares(f, p0, jac=jac, method="lm", ftol=tiny, xtol=tiny, gtol=tiny, max_nfev=400)
        R, t = cam(sol.x)
        X = sol.x[6:].reshape(n, 3)
    else:
        state = dict(X=X_start.copy())

        def inner(R, t):
            # the points that minimise the residual for this camera: Newton from the last ones.  A trial camera far enough out
            # for the solve to break down gets its points from the start again, and LM's own gain test refuses the step.
            X = state["X"]
            for _ in range(50):
                r1, r2, A1, A2, J2x, RX = resid_jac(R, t, X)
                V = A1.transpose(0, 2, 1) @ A1 + J2x.transpose(0, 2, 1) @ J2x
                g = (A1.transpose(0, 2, 1) @ r1[:, :, None] + J2x.transpose(0, 2, 1) @ r2[:, :, None])
                try:
                    d = np.linalg.solve(V, g)[:, :, 0]
                except np.linalg.LinAlgError:
                    return X_start
                if not np.isfinite(d).all():
                    return X_start
                X = X - d
                if np.abs(d).max() <= 1e-15 * np.abs(X).max():
                    break
            state["X"] = X
            return X

        def f(p):
            R, t = cam(p)
            r1, r2, *_ = resid_jac(R, t, inner(R, t))
            return np.concatenate([r1, r2], 1).ravel()

        def jac(p):
            R, t = cam(p)
            r1, r2, A1, A2, J2x, RX = resid_jac(R, t, inner(R, t))
            Jc = np.concatenate([np.zeros((n, 2, 6)), cam_block(A2, RX, R, p)], 1)      # (n, 4, 6)
            Jx = np.concatenate([A1, J2x], 1)                                           # (n, 4, 3)
            V = Jx.transpose(0, 2, 1) @ Jx
            Jp = Jc - Jx @ np.linalg.solve(V, Jx.transpose(0, 2, 1) @ Jc)
            return Jp.reshape(4 * n, 6)
        sol = least_squares(f, np.concatenate([np.zeros(3), t_start]), jac=jac, method="lm", ftol=tiny, xtol=tiny, gtol=tiny,
                            max_nfev=400)
        R, t = cam(sol.x)
        X = inner(R, t)
    # the objective does not change when t and the points are scaled together, by a negative factor either: |t| = 1 on the side
    # of the start
    s = (1.0 if t @ t_start >= 0 else -1.0) / np.sqrt(t @ t)
    return R, t * s, X * s


def disagreement(info, K):
    """Per output array, relative to the array's largest magnitude: how far refine()'s float64 result is from the second
    formulation's (started from refine()'s own start, the inputs, in the full-vector form)."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    part = info["part"]
    if len(info["X_start"]) <= FULL_VECTOR_MAX:
        start = (info["R_start"], info["t_start"], info["X_start"])
    else:
        start = (info["R64"], info["t64"], info["X64"])
    Rs, ts, Xs = second_formulation(K, *start, info["o1"][part], info["o2"][part])
    c2a, c2b = camera(K, info["R64"], info["t64"]), camera(K, Rs, ts)
    return dict(R=float(np.abs(Rs - info["R64"]).max()), t=float(np.abs(ts - info["t64"]).max()),
                c2=float(np.abs(c2a - c2b).max() / np.abs(c2a).max()),
                X=float(np.abs(Xs - info["X64"]).max() / np.abs(info["X64"]).max()))


# ------------------------------------------------------------------------------------------------ inputs
def pose_inputs(xy1, xy2, matches, n, F, K=KMAT, choose=False):
    """The pose chain in float64 up to the refinement's inputs: ref64's extract_Rt on F, c2 = K [R | t], ref64's triangulation of
    the n matches; each rounded to f32 as the device stages hand them on.  choose: instead of extract_Rt's own pick, the one of
    its four (R1 | R2, +-t) with the most points in front of both cameras (the cheirality check the reference leaves out).
    Returns R (3, 3), t (3,), points4d (len(matches), 4)."""
    import ref64
    rt = ref64.extract_Rt(F, K)
    c1 = np.c_[np.asarray(K, np.float32), np.zeros(3, np.float32)]
    m = np.asarray(matches)[:n]
    best = None
    for Rc, tc in ([(rt["R"], rt["t"])] if not choose else [(rt[r], s * rt["t"]) for r in ("R1", "R2") for s in (1.0, -1.0)]):
        R, t = Rc.astype(np.float32), tc.astype(np.float32)
        c2 = ref64.camera_matrix(K, R, t)[0].astype(np.float32)
        X = ref64.triangulate(xy1[m[:, 0]], xy2[m[:, 1]], c1, c2)["X"]
        with np.errstate(all="ignore"):
            front = int(((X[:, 2] > 0) & (transform(R.astype(np.float64), t.astype(np.float64), X)[:, 2] > 0)).sum())
        if best is None or front > best[0]:
            best = (front, R, t, X)
    _, R, t, X = best
    P = np.zeros((len(matches), 4), np.float32)
    P[:n, :3] = X
    P[:n, 3] = 1.0
    return R, t, P


def case(seed, Kp, n, sigma=0.5):
    """One comparison input: ref_refit.case's correspondences, F refitted over them (ref_refit.refit), then pose_inputs.
    Returns xy1, xy2, matches, best, R, t, points4d."""
    import ref_refit
    xy1, xy2, matches, best, F_in = ref_refit.case(seed, Kp, n, sigma)
    F, _ = ref_refit.refit(xy1, xy2, matches[:n], F_in, kp_stride=Kp)
    R, t, P = pose_inputs(xy1, xy2, matches, n, F)
    return xy1, xy2, matches, best, R, t, P


GATE_SQ = 16.0           # 4 x the pose chain's reproj_threshold_sq of 4
MAX_ITERATIONS = 20
COMPARISON_SHAPES = [(64, 8), (64, 9), (64, 63), (64, 64), (1024, 255), (1024, 256), (1024, 257), (1024, 1023), (8160, 8160),
                     (4096, 3200), (4096, 3201)]   # the last pair whose point state the device keeps in LDS, the first it does not
MIXED_BATCH = (1024, [300, 8, 1023, 77, 256, 511, 40])
SEAM_BATCH = (4096, [3200, 64, 3201])   # one launch: the two sides of that seam and a small pair (the first and the last shapes
                                        # are the comparison shapes above, the same inputs)
# Seeds per input, chosen on the CPU (tests/test_ref_refine.py checks what they were chosen for): the reference's extract_Rt may
# pick an (R, t) that puts the points behind a camera -- a legitimate "left alone" input, no comparison -- so each seed is the
# first from its starting value at which at least n - 2 matches participate and the refinement is comparable.
SHAPE_SEEDS = {(64, 8): 130, (64, 9): 168, (64, 63): 238, (64, 64): 304, (1024, 255): 359, (1024, 256): 424, (1024, 257): 488,
               (1024, 1023): 555, (8160, 8160): 612, (4096, 3200): 702, (4096, 3201): 770, (4096, 64): 840}
MIXED_SEEDS = {0: 1003, 1: 1070, 2: 1130, 3: 1199, 4: 1257, 5: 1327, 6: 1384}


def _first_seed(start, Kp, n):
    for seed in range(start, start + 64):
        c = case(seed, Kp, n)
        out = refine(c[0], c[1], c[2][:n], KMAT, c[4], c[5], c[6], GATE_SQ, MAX_ITERATIONS, kp_stride=Kp)
        i = out[4]
        if (not i["left_alone"] and i["stats"][0] >= n - 2 and i["comparable"] and i["margin"] >= DECIDED_MARGIN
                and i["last_rel"] < REL_STOP):
            return seed
    raise RuntimeError("no seed")


def comparison_cases():
    """[(name, xy1, xy2, matches, best, R, t, points4d)] -- fixed seeds; shared by the CPU test and the GPU test."""
    out = []
    for (Kp, n) in COMPARISON_SHAPES:
        out.append((f"K{Kp}_n{n}",) + case(SHAPE_SEEDS[(Kp, n)], Kp, n))
    Kp, ns = MIXED_BATCH
    for j, n in enumerate(ns):
        out.append((f"mixed{j}_n{n}",) + case(MIXED_SEEDS[j], Kp, n))
    Kp, ns = SEAM_BATCH
    for n in ns:
        if (Kp, n) not in COMPARISON_SHAPES:
            out.append((f"K{Kp}_n{n}",) + case(SHAPE_SEEDS[(Kp, n)], Kp, n))
    return out


_RESULTS = None


def run_case(c):
    n = int(c[4][3])
    out = refine(c[1], c[2], c[3][:n], KMAT, c[5], c[6], c[7], GATE_SQ, MAX_ITERATIONS, kp_stride=len(c[1]))
    info = out[4]
    part = info["part"]
    Ri = c[5].astype(np.float64)
    ti = c[6].astype(np.float64)
    info["R_start"] = 0.5 * (Ri @ (3.0 * np.eye(3) - Ri.T @ Ri))
    info["t_start"] = ti / np.sqrt(ti @ ti)
    info["X_start"] = c[7][:n, :3].astype(np.float64)[part]
    return out


def comparison_results():
    """{name: (R, t, c2, points4d, info)} of refine() over comparison_cases(), with info["delta"] the disagreement with the
    second formulation; computed once and shared."""
    global _RESULTS
    if _RESULTS is None:
        _RESULTS = {}
        for c in comparison_cases():
            out = run_case(c)
            out[4]["delta"] = disagreement(out[4], KMAT) if not out[4]["left_alone"] else None
            _RESULTS[c[0]] = out
    return _RESULTS


def delta_ref():
    """The largest disagreement of the two formulations over the comparable comparison inputs, any output array, relative to
    the array's largest magnitude; the device comparison allows 16 of these.  Measured value: see tests/test_ref_refine.py."""
    return max(max(o[4]["delta"].values()) for o in comparison_results().values() if o[4]["comparable"])


# ------------------------------------------------------------------------------------------------ the accuracy claim
def F_of(K, R, t):
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    Ki = np.linalg.inv(K)
    F = Ki.T @ skew(np.asarray(t, np.float64).reshape(3)) @ np.asarray(R, np.float64).reshape(3, 3) @ Ki
    return F / np.sqrt((F * F).sum())


def accuracy_inputs():
    """ref_refit.accuracy_pairs() taken to the refinement's inputs: per pair xy1, xy2 (n, 2), matches (identity), R, t,
    points4d, and the held-out exact correspondences h1, h2.  The refitted F feeds extract_Rt; of its four (R, t) the one that
    passes the cheirality check is taken (pose_inputs(choose=True)), as in the sketch the claim comes from."""
    import ref_refit
    out = []
    for p1, p2, h1, h2, F_in in ref_refit.accuracy_pairs():
        n = len(p1)
        m = np.stack([np.arange(n)] * 2, 1).astype(np.int32)
        F, _ = ref_refit.refit(p1, p2, m, F_in)
        R, t, P = pose_inputs(p1, p2, m, n, F, choose=True)
        out.append((p1, p2, m, R, t, P, h1, h2))
    return out
