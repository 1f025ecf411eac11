"""vslam_sim3_ransac and vslam_sim3_refine (include/vslam_sim3.h) restated in numpy / Python float64, written from the header's
text -- not from the device code.  Nothing is fused: one IEEE operation per Python operator, in the header's order, so the sets,
models, M_a / M_b, counts, winner, mask and compaction are comparable BIT FOR BIT with the serial walk of the kernels' text
(tests/native/sim3_serial.cpp) and with the device.  The model of a hypothesis is written in scalars; the count is written once over
arrays (the same operations element by element).  The polish's sums over correspondences are numpy's (pairwise), which is not the
device's order: that, and the library sine, is what DELTA_REF is for.

world_gather(), world_similarity(), world_sim3(), apply_sim3()   the two calls on a world, one item / one track at a time.
second_formulation()  the polish's objective through scipy's least_squares over residuals formed from 4 x 4 homogeneous products
                      (T_ba = [s R | t; 0 1], its inverse by numpy.linalg.inv), started from refine()'s result.
numeric_jacobian()    central differences of the header's residuals in d = (w, tau, sigma), against jacobians().

Measured here (tests/test_ref_sim3.py re-measures and compares), K = (525, 525, 320, 240), 640 x 480, depths 2 .. 9, s in 0.3 .. 3,
rotation up to 0.5 rad, pixels rounded to f32, a share of the pairs replaced by a random B and a random pixel xb, seeds 0 .. 19 of
every configuration of CONFIGS: the winner's inlier set equals the planted set on all 120 scenes, and the winner's s is within
SCALE_WORST (relative) of the truth.
  polish started 1 degree / 3 % / 0.05 off the truth on the planted inliers: DELTA_REF between refine() and second_formulation();
  the polished (s, R, t) against the truth at most POLISH_WORST (entry-wise; s relative, t absolute in units of 2 .. 9).
  0.5 px of keypoint noise on both images: the polished (s, R, t) within NOISE_BOUND = 4 x NOISE_WORST of the truth (model_error).
  That is the noise floor of these scenes and nothing more.
"""
import math

import numpy as np

import ref_pnp as rp
import ref_resect as rr

f64 = np.float64
DEFAULTS = dict(hypotheses=128, min_inliers=8, inlier_px=2.0)
ROT_TOL = 1e-9
WIDTH, HEIGHT = 640, 480
CONFIGS = [(12, 0.5, 64, 6), (40, 0.5, 64, 8), (257, 0.5, 64, 8), (1025, 0.5, 64, 8), (200, 0.5, 128, 8), (200, 0.7, 256, 8)]   # n, outlier share, hypotheses, min_inliers
SEEDS = list(range(20))
SCALE_BOUND = 1e-12          # the issue's: the winner's s against the truth, relative
SCALE_WORST = 4.5e-16        # measured over the 120 scenes: 4.44e-16
DELTA_REF = 6.7e-13          # measured over POLISH_CASES: 6.66e-13 between refine() and second_formulation()
POLISH_WORST = 7.3e-8        # measured over POLISH_CASES: 7.21e-8 from the truth (pixels rounded to f32 at up to 640)
POLISH_BOUND = 2.9e-7        # 4 x
PLANTED_POLISH_WORST = 5.7e-7   # measured over the 120 scenes polished from the winner: 5.63e-7 (n = 12: six pairs carry the model)
PLANTED_POLISH_BOUND = 2.3e-6   # 4 x
NOISE_WORST = 4.9e-3         # measured, n = 200 at 50 %, 128 hypotheses, seeds 0 .. 19, 0.5 px on both images: 4.80e-3
NOISE_BOUND = 2.0e-2         # 4 x, rounded up


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def sample(seed, h, n):
    """vslam_pnp.h's sampler (tests/ref_pnp.py restates it), with its n < 3 rule"""
    return rp.sample(seed, h, n) if n >= 3 else None


# ------------------------------------------------------------------------------------------------ the model
def _d2(a, c):
    d0, d1, d2 = a[0] - c[0], a[1] - c[1], a[2] - c[2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def _div(a, b):
    """IEEE division in Python floats: x / 0 is +-inf or nan, not an exception"""
    with np.errstate(all="ignore"):
        return float(f64(a) / f64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(f64(a)))


def frame(p0, p1, p2):
    """e1 = (p1 - p0) / |.|, e3 = (e1 x (p2 - p0)) / |.|, e2 = e3 x e1"""
    ab = [p1[k] - p0[k] for k in range(3)]
    ac = [p2[k] - p0[k] for k in range(3)]
    n1 = _sqrt((ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2])
    e1 = [_div(ab[k], n1) for k in range(3)]
    w = [e1[1] * ac[2] - e1[2] * ac[1], e1[2] * ac[0] - e1[0] * ac[2], e1[0] * ac[1] - e1[1] * ac[0]]
    n3 = _sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    e3 = [_div(w[k], n3) for k in range(3)]
    e2 = [e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]]
    return e1, e2, e3


def kmul(K, L, c):
    """K [L | c] (12,), rows ((K_r0 . + K_r1 .) + K_r2 .)"""
    M = [0.0] * 12
    for r in range(3):
        for j in range(3):
            M[4 * r + j] = (K[3 * r] * L[j] + K[3 * r + 1] * L[3 + j]) + K[3 * r + 2] * L[6 + j]
        M[4 * r + 3] = (K[3 * r] * c[0] + K[3 * r + 1] * c[1]) + K[3 * r + 2] * c[2]
    return M


def projections(K, s, R, t):
    """-> M_a, M_b (12,) each"""
    Mb = kmul(K, [s * R[k] for k in range(9)], t)
    L = [0.0] * 9
    u = [0.0] * 3
    for i in range(3):
        for j in range(3):
            L[3 * i + j] = _div(R[3 * j + i], s)
        u[i] = -_div((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2], s)
    return kmul(K, L, u), Mb


def model(K, A, B, plant=None):
    """A, B (3, 3): three pairs in sampling order; K (9,) floats.  -> (s, R (9,), t (3,), Ma, Mb) or None when dropped"""
    A = [[float(v) for v in row] for row in A]
    B = [[float(v) for v in row] for row in B]
    K = [float(v) for v in K]
    with np.errstate(all="ignore"):
        cA = [((A[0][k] + A[1][k]) + A[2][k]) / 3.0 for k in range(3)]
        cB = [((B[0][k] + B[1][k]) + B[2][k]) / 3.0 for k in range(3)]
        sa = (_d2(A[0], cA) + _d2(A[1], cA)) + _d2(A[2], cA)
        sb = (_d2(B[0], cB) + _d2(B[1], cB)) + _d2(B[2], cB)
        s = _sqrt(_div(sb, sa))
        FA, FB = frame(*A), frame(*B)
        R = [(FB[0][i] * FA[0][j] + FB[1][i] * FA[1][j]) + FB[2][i] * FA[2][j] for i in range(3) for j in range(3)]
        if plant == "t_from_first_point":
            t = [B[0][r] - s * ((R[3 * r] * A[0][0] + R[3 * r + 1] * A[0][1]) + R[3 * r + 2] * A[0][2]) for r in range(3)]
        else:
            t = [cB[r] - s * ((R[3 * r] * cA[0] + R[3 * r + 1] * cA[1]) + R[3 * r + 2] * cA[2]) for r in range(3)]
        Ma, Mb = projections(K, s, R, t)
        vals = np.array([s] + R + t + Ma + Mb, f64)
        if not (np.isfinite(vals).all() and s > 0.0):
            return None
        worst = 0.0
        for i in range(3):
            for j in range(i, 3):
                g = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j]
                worst = max(worst, abs(g - (1.0 if i == j else 0.0)))
        if worst > ROT_TOL:
            return None
    return s, np.array(R, f64), np.array(t, f64), np.array(Ma, f64), np.array(Mb, f64)


# ------------------------------------------------------------------------------------------------ the count and the choice
def passes(M, X, x, px, plant=None):
    """(X (n, 3), x (n, 2)) under M (12,): q_2 > 0 and the closed disc, without a division"""
    with np.errstate(all="ignore"):
        q = [((M[4 * r] * X[:, 0] + M[4 * r + 1] * X[:, 1]) + M[4 * r + 2] * X[:, 2]) + M[4 * r + 3] for r in range(3)]
        d0, d1, l = q[0] - x[:, 0] * q[2], q[1] - x[:, 1] * q[2], f64(px) * q[2]
        ll = l * l
        inside = (d0 * d0 + d1 * d1 < ll) if plant == "open_disc" else (d0 * d0 + d1 * d1 <= ll)
        return (q[2] > 0.0) & inside & np.isfinite(ll)


def inlier_mask(Ma, Mb, A, xa, B, xb, px, plant=None):
    m = passes(Mb, A, xb, px, plant)
    return m if plant == "one_direction" else m & passes(Ma, B, xa, px, plant)


def sim3_ransac(A, xa, B, xb, n, K, seed, keep, polish=None, plant=None, **kw):
    """A, B (S, 3) f64; xa, xb (S, 2) f32; n; K 3 x 3 f32; seed; keep = (s, R (9,), t (3,)): the bits an item that is not found keeps.
    polish: None or a dict of vslam_resect_params fields.  -> dict(found, winner, counts (hypotheses,) int32 with -1 for no
    model, models {h: (s, R, t, Ma, Mb)}, sets {h: [i0, i1, i2]}, inlier (S,) int32, n_inliers, corr_index, s_raw, R_raw, t_raw,
    s, R, t, stats)"""
    p = params(**kw)
    S = len(A)
    n = min(max(int(n), 0), S)
    Av, Bv = np.asarray(A, f64).reshape(-1, 3)[:n], np.asarray(B, f64).reshape(-1, 3)[:n]
    xav, xbv = (np.asarray(v, np.float32).astype(f64).reshape(-1, 2)[:n] for v in (xa, xb))
    Kv = np.asarray(K, np.float32).astype(f64).reshape(9)
    s0, R0, t0 = float(keep[0]), np.array(keep[1], f64).reshape(9), np.array(keep[2], f64).reshape(3)
    H = p["hypotheses"]
    res = dict(found=False, winner=-1, counts=np.full(H, -1, np.int32), models={}, sets={}, inlier=np.zeros(S, np.int32), n_inliers=0,
               corr_index=np.zeros(0, np.int32), s_raw=s0, R_raw=R0, t_raw=t0, s=s0, R=R0.copy(), t=t0.copy(), stats=np.full(4, np.nan))
    if n < 4 or not all(np.isfinite(v).all() for v in (Av, Bv, xav, xbv, Kv)):
        return res
    best = 0
    for h in range(H):
        idx = sample(seed, h, n)
        if idx is None:
            continue
        res["sets"][h] = idx
        m = model(Kv, Av[idx], Bv[idx], plant)
        if m is None:
            continue
        res["models"][h] = m
        c = int(inlier_mask(m[3], m[4], Av, xav, Bv, xbv, p["inlier_px"], plant).sum())
        res["counts"][h] = c
        key = (c << 10) | (h if plant == "tie_larger" else 1023 - h)
        best = max(best, key)
    if best == 0 or (best >> 10) < p["min_inliers"]:
        return res
    h = (best & 1023) if plant == "tie_larger" else 1023 - (best & 1023)
    s, R, t, Ma, Mb = res["models"][h]
    mask = inlier_mask(Ma, Mb, Av, xav, Bv, xbv, p["inlier_px"], plant)
    res.update(found=True, winner=h, s_raw=s, R_raw=R, t_raw=t, s=s, R=R.copy(), t=t.copy(), n_inliers=int(mask.sum()),
               corr_index=np.flatnonzero(mask).astype(np.int32))
    res["inlier"][:n] = mask
    if polish is not None:
        full = np.zeros(S, bool)
        full[:n] = mask
        s2, R2, t2, stats, _ = refine(A, xa, B, xb, n, full, K, s, R, t, **polish)
        res.update(s=s2, R=R2, t=t2, stats=stats)
    return res


# ------------------------------------------------------------------------------------------------ the polish
def observe(K, s, R, t, A, xa, B, xb):
    """both directions of the header -> dict(W, Yb, ub, vb, q2b, rb0, rb1, eb, Ya, ua, va, q2a, ra0, ra1, ea)"""
    with np.errstate(all="ignore"):
        RA = np.stack([(R[3 * r] * A[:, 0] + R[3 * r + 1] * A[:, 1]) + R[3 * r + 2] * A[:, 2] for r in range(3)], 1)
        W = s * RA
        Yb = W + t[None, :]
        ub, vb, q2b = rr.project(K, Yb)
        rb0, rb1 = ub - xb[:, 0], vb - xb[:, 1]
        D = B - t[None, :]
        Ya = np.stack([((R[r] * D[:, 0] + R[3 + r] * D[:, 1]) + R[6 + r] * D[:, 2]) / s for r in range(3)], 1)
        ua, va, q2a = rr.project(K, Ya)
        ra0, ra1 = ua - xa[:, 0], va - xa[:, 1]
        return dict(W=W, Yb=Yb, ub=ub, vb=vb, q2b=q2b, rb0=rb0, rb1=rb1, eb=np.sqrt(rb0 * rb0 + rb1 * rb1),
                    Ya=Ya, ua=ua, va=va, q2a=q2a, ra0=ra0, ra1=ra1, ea=np.sqrt(ra0 * ra0 + ra1 * ra1))


def tri7(i, j):
    return i * 7 - i * (i - 1) // 2 + (j - i)


def jacobians(K, s, R, o, plant=None):
    """-> Jb, Ja: [2][7] lists of (n,) arrays, the header's columns"""
    with np.errstate(all="ignore"):
        Jb, Ja = [], []
        for u, q2, row in ((o["ub"], o["q2b"], 0), (o["vb"], o["q2b"], 1)):
            a = [(K[3 * row + k] - u * K[6 + k]) / q2 for k in range(3)]
            W = o["W"]
            Jb.append([a[2] * W[:, 1] - a[1] * W[:, 2], a[0] * W[:, 2] - a[2] * W[:, 0], a[1] * W[:, 0] - a[0] * W[:, 1], a[0], a[1], a[2],
                       (a[0] * W[:, 0] + a[1] * W[:, 1]) + a[2] * W[:, 2]])
        for u, q2, row in ((o["ua"], o["q2a"], 0), (o["va"], o["q2a"], 1)):
            a = [(K[3 * row + k] - u * K[6 + k]) / q2 for k in range(3)]
            Y = o["Ya"]
            N = [a[2] * Y[:, 1] - a[1] * Y[:, 2], a[0] * Y[:, 2] - a[2] * Y[:, 0], a[1] * Y[:, 0] - a[0] * Y[:, 1]]
            rot = [-((N[0] * R[3 * k] + N[1] * R[3 * k + 1]) + N[2] * R[3 * k + 2]) for k in range(3)]
            if plant == "ja_rotation_sign":
                rot = [-c for c in rot]
            tr = [-(((a[0] * R[3 * k] + a[1] * R[3 * k + 1]) + a[2] * R[3 * k + 2]) / s) for k in range(3)]
            Ja.append(rot + tr + [-((a[0] * Y[:, 0] + a[1] * Y[:, 1]) + a[2] * Y[:, 2])])
    return Jb, Ja


def contributions(K, s, R, t, delta, A, xa, B, xb, plant=None):
    """(n, 35): what each correspondence adds to H's upper triangle (28) and to g (7)"""
    o = observe(K, s, R, t, A, xa, B, xb)
    Jb, Ja = jacobians(K, s, R, o, plant)
    with np.errstate(all="ignore"):
        wb = np.where(o["eb"] <= delta, 1.0, delta / o["eb"])
        wa = np.where(o["ea"] <= delta, 1.0, delta / o["ea"])
        out = np.empty((len(A), 35), f64)
        for i in range(7):
            for j in range(i, 7):
                out[:, tri7(i, j)] = wb * (Jb[0][i] * Jb[0][j] + Jb[1][i] * Jb[1][j]) + wa * (Ja[0][i] * Ja[0][j] + Ja[1][i] * Ja[1][j])
            out[:, 28 + i] = wb * (Jb[0][i] * o["rb0"] + Jb[1][i] * o["rb1"]) + wa * (Ja[0][i] * o["ra0"] + Ja[1][i] * o["ra1"])
    return out


def solve7(acc, lam):
    """(H + lam max(diag H, floor)) d = -g by Cholesky, 7 x 7 -> d (7,) or None"""
    N = 7
    acc = [f64(a) for a in acc]
    L = [[f64(0)] * N for _ in range(N)]
    ok = True
    with np.errstate(all="ignore"):
        for j in range(N):
            h = acc[tri7(j, j)]
            p = h + f64(lam) * max(h, f64(rr.DIAG_FLOOR)) if not np.isnan(h) else h
            for k in range(j):
                p = p - L[j][k] * L[j][k]
            ok = ok and bool(p > 0.0)
            L[j][j] = np.sqrt(p)
            for i in range(j + 1, N):
                v = acc[tri7(j, i)]
                for k in range(j):
                    v = v - L[i][k] * L[j][k]
                L[i][j] = v / L[j][j]
        fw = [f64(0)] * N
        for i in range(N):
            v = acc[28 + i]
            for k in range(i):
                v = v - L[i][k] * fw[k]
            fw[i] = v / L[i][i]
        d = [f64(0)] * N
        for i in range(N - 1, -1, -1):
            v = fw[i]
            for k in range(N - 1, i, -1):
                v = v - L[k][i] * d[k]
            d[i] = v / L[i][i]
    d = np.array([-v for v in d], f64)
    return d if ok and np.isfinite(d).all() else None


def cost(o, delta):
    return rr.rho(o["eb"], delta) + rr.rho(o["ea"], delta)


def front(o):
    return (o["Yb"][:, 2] > 0.0) & (o["Ya"][:, 2] > 0.0)


def refine(A, xa, B, xb, n, mask, K, s_in, R_in, t_in, plant=None, **kw):
    """vslam_sim3_refine for one item.  mask: (S,) bool or None.  -> s, R (9,), t (3,), stats (4,), info (moved, part)"""
    p = rr.params(**kw)
    S = len(A)
    n = min(max(int(n), 0), S)
    take = np.zeros(S, bool)
    take[:n] = True
    if mask is not None:
        take &= np.asarray(mask).astype(bool)
    A, B = np.asarray(A, f64).reshape(-1, 3)[take], np.asarray(B, f64).reshape(-1, 3)[take]
    xa, xb = (np.asarray(v, np.float32).astype(f64).reshape(-1, 2)[take] for v in (xa, xb))
    K = np.asarray(K, np.float32).astype(f64).reshape(9)
    si, Ri, ti = f64(s_in), np.array(R_in, f64).reshape(9), np.array(t_in, f64).reshape(3)
    m = len(A)
    nan = float("nan")
    info = dict(moved=False, part=np.ones(m, bool))

    def alone(count):
        return float(si), Ri.copy(), ti.copy(), np.array([count, nan, nan, nan]), info
    fin = all(np.isfinite(v).all() for v in (A, B, xa, xb, K, Ri, ti)) and np.isfinite(si)
    if m < p["min_links"] or not fin or not si > 0.0:
        return alone(m)
    delta, gate = f64(p["huber_px"]), f64(p["gate_px"])
    R0 = rr.start_rotation(Ri)
    s, R, t = si, R0, ti.copy()
    part = np.ones(m, bool)
    accepted, count = 0, m
    with np.errstate(all="ignore"):
        for rnd in range(p["rounds"]):
            o = observe(K, s, R, t, A, xa, B, xb)
            if rnd > 0:
                cand_part = front(o) & (o["eb"] <= gate) & (o["ea"] <= gate)
                if int(cand_part.sum()) < p["min_links"]:
                    break
                part = cand_part
            count = int(part.sum())
            sel = (A[part], xa[part], B[part], xb[part])
            obj = f64(cost(o, delta)[part].sum())
            lam = f64(rr.LAMBDA0)
            for _ in range(p["max_iterations"]):
                d = solve7(contributions(K, s, R, t, delta, *sel, plant=plant).sum(0), lam)
                accept = False
                if d is not None:
                    Rn, tn, sn = rr.rotate(d[:3], R), t + d[3:6], s * (1.0 + d[6])
                    if plant == "scale_frozen":
                        sn = s
                    if sn > 0.0:
                        on_ = observe(K, sn, Rn, tn, *sel)
                        on = f64(cost(on_, delta).sum())
                        accept = bool(front(on_).all()) and bool(on < obj)
                if accept:
                    rel = (obj - on) / obj
                    s, R, t, obj = sn, Rn, tn, on
                    accepted += 1
                    lam = max(lam / 10.0, f64(rr.LAMBDA_MIN))
                    if rel < rr.REL_STOP:
                        break
                else:
                    lam = lam * 10.0
                    if lam > rr.LAMBDA_MAX:
                        break
        info["part"] = part
        if accepted == 0 or not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s)):
            return alone(count)
        sel = (A[part], xa[part], B[part], xb[part])
        s1 = f64(cost(observe(K, si, R0, ti, *sel), delta).sum()) / f64(count)
        s2 = f64(cost(observe(K, s, R, t, *sel), delta).sum()) / f64(count)
    if not (np.isfinite(s1) and np.isfinite(s2)):
        return alone(count)
    info["moved"] = True
    return float(s), R, t, np.array([count, s1, s2, accepted], f64), info


# ------------------------------------------------------------------------------------------------ the second formulation
def _rodrigues(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / (th * th) * (W @ W)


def homogeneous_residuals(K, s, R, t, A, xa, B, xb):
    """(n, 4): r_b and r_a from 4 x 4 homogeneous products: T = [s R | t; 0 1] and numpy's inverse of it"""
    T = np.eye(4)
    T[:3, :3] = s * np.asarray(R, f64).reshape(3, 3)
    T[:3, 3] = t
    P = np.zeros((3, 4))
    P[:, :3] = np.asarray(K, f64).reshape(3, 3)
    hom = lambda X: np.concatenate([X, np.ones((len(X), 1))], 1)
    qb = hom(A) @ (P @ T).T
    qa = hom(B) @ (P @ np.linalg.inv(T)).T
    return np.concatenate([qb[:, :2] / qb[:, 2:3] - xb, qa[:, :2] / qa[:, 2:3] - xa], 1)


def second_formulation(A, xa, B, xb, K, s0, R0, t0, delta):
    """min sum rho(e_b) + rho(e_a) through scipy's least_squares with loss="huber" over the 2 n norms, a rotation vector applied to
    R0, a free t and a free s.  -> s, R (9,), t (3,)"""
    from scipy.optimize import least_squares
    A, B = np.asarray(A, f64), np.asarray(B, f64)
    xa, xb = np.asarray(xa, np.float32).astype(f64), np.asarray(xb, np.float32).astype(f64)
    Km = np.asarray(K, np.float32).astype(f64).reshape(9)
    Rm = np.asarray(R0, f64).reshape(3, 3)

    def f(p):
        r = homogeneous_residuals(Km, p[6], (_rodrigues(p[:3]) @ Rm).reshape(9), p[3:6], A, xa, B, xb)
        return np.concatenate([np.sqrt((r[:, :2] ** 2).sum(1)), np.sqrt((r[:, 2:] ** 2).sum(1))])
    p0 = np.concatenate([np.zeros(3), np.asarray(t0, f64), [float(s0)]])
    sol = least_squares(f, p0, jac="3-point", method="trf", loss="huber", f_scale=float(delta), ftol=1e-15, xtol=1e-15, gtol=1e-15,
                        x_scale=1.0, max_nfev=200)
    return float(sol.x[6]), (_rodrigues(sol.x[:3]) @ Rm).reshape(9), sol.x[3:6].copy()


def numeric_jacobian(K, s, R, t, A, xa, B, xb, step=1e-6):
    """central differences of (rb0, rb1, ra0, ra1) in d = (w, tau, sigma) at 0 -> (n, 4, 7)"""
    def res(d):
        o = observe(K, s * (1.0 + d[6]), rr.rotate(d[:3], R), t + d[3:6], A, xa, B, xb)
        return np.stack([o["rb0"], o["rb1"], o["ra0"], o["ra1"]], 1)
    out = np.empty((len(A), 4, 7))
    for k in range(7):
        d = np.zeros(7)
        d[k] = step
        out[:, :, k] = (res(d) - res(-d)) / (2 * step)
    return out


# ------------------------------------------------------------------------------------------------ scenes
def planted(n, outliers, seed, noise_px=0.0):
    """-> dict(A, B (n, 3) f64, xa, xb (n, 2) f32, K, s, R (9,), t (3,), planted (n,) bool: the pairs left exact).  A has depths
    2 .. 9 in camera a and projects inside the image there; B = s R A + t is kept in front of camera b with its projection
    wherever it falls.  A replaced pair gets a random B (depths 2 s .. 9 s) and a random pixel xb."""
    rng = np.random.default_rng(7000 * n + seed)
    K = rr.kmat()
    Kd = K.astype(f64)
    while True:
        s = float(rng.uniform(0.3, 3.0))
        w = rng.normal(size=3)
        R = _rodrigues(w / np.linalg.norm(w) * rng.uniform(0.05, 0.5))
        t = rng.uniform(-1.0, 1.0, 3) * s
        px = np.stack([rng.uniform(20, WIDTH - 20, n), rng.uniform(20, HEIGHT - 20, n), np.ones(n)], 1)
        A = np.linalg.solve(Kd, px.T).T * rng.uniform(2.0, 9.0, (n, 1))
        B = s * (A @ R.T) + t
        if (B[:, 2] > 0.5 * s).all():
            break
    qa, qb = A @ Kd.T, B @ Kd.T
    xa, xb = qa[:, :2] / qa[:, 2:3], qb[:, :2] / qb[:, 2:3]
    if noise_px:
        xa, xb = xa + rng.normal(size=(n, 2)) * noise_px, xb + rng.normal(size=(n, 2)) * noise_px
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    k = int(out.sum())
    if k:
        rays = np.linalg.solve(Kd, np.stack([rng.uniform(0, WIDTH, k), rng.uniform(0, HEIGHT, k), np.ones(k)], 1).T).T
        B[out] = rays * rng.uniform(2.0 * s, 9.0 * s, (k, 1))
        xb[out] = np.stack([rng.uniform(0, WIDTH, k), rng.uniform(0, HEIGHT, k)], 1)
    return dict(A=A, B=B, xa=xa.astype(np.float32), xb=xb.astype(np.float32), K=K, s=s, R=R.reshape(9), t=t, planted=~out, n=n)


def model_error(s, R, t, sc):
    """entry-wise: s relative, R and t absolute"""
    return max(abs(s / sc["s"] - 1.0), float(np.abs(np.asarray(R) - sc["R"]).max()), float(np.abs(np.asarray(t) - sc["t"]).max()))


def perturbed(sc, seed):
    """the truth turned by 1 degree, its scale 3 % off and its translation 0.05 off: a start for the polish"""
    rng = np.random.default_rng(31 * seed + 5)
    w = rng.normal(size=3)
    R = _rodrigues(w / np.linalg.norm(w) * np.deg2rad(1.0)) @ sc["R"].reshape(3, 3)
    d = rng.normal(size=3)
    return sc["s"] * 1.03, R.reshape(9), sc["t"] + 0.05 * d / np.linalg.norm(d)


POLISH_CASES = [(40, 0.5, s) for s in range(4)] + [(257, 0.5, s) for s in range(4)] + [(200, 0.7, s) for s in range(4)]


def polish_case(n, share, seed, noise_px=0.0):
    """-> (scene, its planted rows as (A, xa, B, xb), the perturbed start)"""
    sc = planted(n, share, seed, noise_px)
    m = sc["planted"]
    return sc, (sc["A"][m], sc["xa"][m], sc["B"][m], sc["xb"][m]), perturbed(sc, seed)


def delta_ref():
    """-> (largest entry-wise disagreement of refine() and second_formulation(), largest error of refine() against the truth)"""
    worst = truth = 0.0
    for n, share, seed in POLISH_CASES:
        sc, rows, (s0, R0, t0) = polish_case(n, share, seed)
        s1, R1, t1, stats, info = refine(*rows, len(rows[0]), None, sc["K"], s0, R0, t0)
        assert info["moved"]
        part = info["part"]
        s2, R2, t2 = second_formulation(*(r[part] for r in rows), sc["K"], s1, R1, t1, rr.DEFAULTS["huber_px"])
        worst = max(worst, abs(s1 - s2) / s1, float(np.abs(R1 - R2).max()), float(np.abs(t1 - t2).max()))
        truth = max(truth, model_error(s1, R1, t1, sc))
    return worst, truth


# ------------------------------------------------------------------------------------------------ on the world
def to_camera(Twc, p):
    """W^t (p - C) of a camera -> world matrix (16,): the transpose stands for the inverse"""
    D = [p[0] - Twc[3], p[1] - Twc[7], p[2] - Twc[11]]
    return np.array([(Twc[i] * D[0] + Twc[4 + i] * D[1]) + Twc[8 + i] * D[2] for i in range(3)], f64)


def world_gather(side_a, side_b, matches, n_matches, xy_a, xy_b, kp_stride):
    """side: dict(ids (kp_stride,) the frame's map_point_ids, points (N, 4) f32 the track's world points, Twc (16,) the frame's
    pose, fuse_to (N,) or None).  -> dict(A, B (m, 3) f64, xa, xb (m, 2) f32, point_a, point_b (m,) int32) in match order"""
    matches = np.asarray(matches, np.int64).reshape(-1, 2)
    n = min(max(int(n_matches), 0), kp_stride, len(matches))
    xy_a, xy_b = np.asarray(xy_a, np.float32).reshape(-1, 2), np.asarray(xy_b, np.float32).reshape(-1, 2)

    def point(side, k):
        i = int(side["ids"][k])
        N = len(side["points"])
        if i < 0 or i >= N:
            return -1, None
        if side.get("fuse_to") is not None:
            i = int(side["fuse_to"][i])
            if i < 0 or i >= N:
                return -1, None
        p = np.asarray(side["points"][i, :3], np.float32).astype(f64)
        return (i, p) if np.isfinite(p).all() else (-1, None)
    rows = []
    for k in range(n):
        a, b = matches[k]
        if not (0 <= a < kp_stride and 0 <= b < kp_stride):
            continue
        ia, pa = point(side_a, a)
        ib, pb = point(side_b, b)
        if ia < 0 or ib < 0 or not (np.isfinite(xy_a[a]).all() and np.isfinite(xy_b[b]).all()):
            continue
        rows.append((to_camera(side_a["Twc"], pa), xy_a[a], to_camera(side_b["Twc"], pb), xy_b[b], ia, ib))
    col = lambda j, dt, w: np.array([r[j] for r in rows], dt).reshape(len(rows), *w)
    return dict(A=col(0, f64, (3,)), xa=col(1, np.float32, (2,)), B=col(2, f64, (3,)), xb=col(3, np.float32, (2,)),
                point_a=col(4, np.int32, ()), point_b=col(5, np.int32, ()))


def world_similarity(Ta, Tb, s, R, t):
    """X_a = s_w R_w X_b + t_w from the camera-to-camera model (a -> b) and the two frames' camera -> world matrices"""
    with np.errstate(all="ignore"):
        sw = f64(1.0) / f64(s)
        M = [(Ta[4 * i] * R[3 * j] + Ta[4 * i + 1] * R[3 * j + 1]) + Ta[4 * i + 2] * R[3 * j + 2] for i in range(3) for j in range(3)]
        u = [(R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2] for i in range(3)]
        Rw = [(M[3 * i] * Tb[4 * j] + M[3 * i + 1] * Tb[4 * j + 1]) + M[3 * i + 2] * Tb[4 * j + 2] for i in range(3) for j in range(3)]
        tw = []
        for r in range(3):
            v = (Ta[4 * r] * u[0] + Ta[4 * r + 1] * u[1]) + Ta[4 * r + 2] * u[2]
            w = (Rw[3 * r] * Tb[3] + Rw[3 * r + 1] * Tb[7]) + Rw[3 * r + 2] * Tb[11]
            tw.append((Ta[4 * r + 3] - v / f64(s)) - sw * w)
    return float(sw), np.array(Rw, f64), np.array(tw, f64)


def world_sim3(side_a, side_b, matches, n_matches, xy_a, xy_b, kp_stride, K, seed, polish=None, **kw):
    """vslam_world_sim3 for one item -> sim3_ransac's dict over the gathered rows (stride kp_stride) plus n_corr, point_a, point_b and,
    where found, s_w, R_w, t_w"""
    g = world_gather(side_a, side_b, matches, n_matches, xy_a, xy_b, kp_stride)
    m = len(g["A"])
    pad3, pad2 = np.full((kp_stride - m, 3), np.nan), np.full((kp_stride - m, 2), np.nan, np.float32)
    keep = (0.0, np.zeros(9), np.zeros(3))
    res = sim3_ransac(np.concatenate([g["A"], pad3]), np.concatenate([g["xa"], pad2]), np.concatenate([g["B"], pad3]),
                      np.concatenate([g["xb"], pad2]), m, K, seed, keep, polish=polish, **kw)
    res.update(n_corr=m, point_a=g["point_a"], point_b=g["point_b"])
    if res["found"]:
        res["s_w"], res["R_w"], res["t_w"] = world_similarity(side_a["Twc"], side_b["Twc"], res["s"], res["R"], res["t"])
    return res


def apply_point(s, R, t, X):
    return np.array([f64(s) * ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + t[i] for i in range(3)], f64)


def apply_pose(s, R, t, Twc):
    out = np.array(Twc, f64).copy()
    Cn = apply_point(s, R, t, [Twc[3], Twc[7], Twc[11]])
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (R[3 * i] * Twc[j] + R[3 * i + 1] * Twc[4 + j]) + R[3 * i + 2] * Twc[8 + j]
        out[4 * i + 3] = Cn[i]
    return out


def apply_sim3(track, s, R, t, apply=1):
    """vslam_world_apply_sim3 on one track: dict(Twc (F, 16) f64, pose (F, 16) f32, scale (F,) f64, carry (K, 3) f64, carry_index (K,),
    points (N, 4) f32, size) -> a new dict; the recorded frames are all F rows given"""
    out = {k: (np.array(v).copy() if isinstance(v, np.ndarray) else v) for k, v in track.items()}
    R, t = np.asarray(R, f64).reshape(9), np.asarray(t, f64).reshape(3)
    if not apply or not (np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all() and s > 0.0):
        return out
    with np.errstate(all="ignore"):
        for f in range(len(out["Twc"])):
            out["Twc"][f] = apply_pose(s, R, t, track["Twc"][f])
            out["pose"][f] = out["Twc"][f].astype(np.float32)
            out["scale"][f] = track["scale"][f] * f64(s)
        for k in range(len(out["carry"])):
            if out["carry_index"][k] >= 0:
                out["carry"][k] = track["carry"][k] * f64(s)
        for i in range(min(max(int(track["size"]), 0), len(out["points"]))):
            X = np.asarray(track["points"][i, :3], np.float32).astype(f64)
            if np.isfinite(X).all():
                out["points"][i, :3] = apply_point(s, R, t, X).astype(np.float32)
    return out
