"""include/vslam_tracks.h restated from its text, not from the device code.

triangulate_item()   vslam_triangulate_tracks for one item in numpy float64, one IEEE operation per Python operator in the header's
                     order.  The points of an item are independent, so the restatement walks all of them at once: step k of a walk
                     handles the k-th entry of every row, and every sum of a point still runs over its own row in order.  What
                     depends on an observation alone (its camera, ray and centre) is formed once per entry; the header forms it again in
                     every walk, to the same bits.  The projection is ref_resect.transform / project, the 3 x 3 Cholesky
                     ref_adjust.chol3 / solve3.
triangulate_batch()  the arrays the entry point writes for a batch.
world_item()         one track of vslam_world_retriangulate given the world's CSR and cameras.
random_track_item() / batch_tracks()   the random items of the tests."""
import numpy as np

import ref_adjust as ra
import ref_resect as rr

f64 = np.float64
NO_PART, OK, TOO_FEW, LOW_PARALLAX, DEGENERATE, BEHIND, UNSUPPORTED, WORSE = -1, 0, 1, 2, 3, 4, 5, 6
DEFAULTS = dict(cos_parallax_max=0.9998, huber_px=ra.DEFAULTS["huber_px"], inlier_px=ra.DEFAULTS["gate_px"], iterations=10, min_good=2, good10=5)
QNAN64 = np.uint64(0x7FF8000000000000)
MAX_KP, MAX_CAMS = 16384, 1024
OUTS = ("out_points", "status", "counts", "info", "stats")


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params_ok(p):
    return bool(np.isfinite(p["cos_parallax_max"]) and -1.0 < p["cos_parallax_max"] <= 1.0 and np.isfinite(p["huber_px"]) and p["huber_px"] > 0 and
                np.isfinite(p["inlier_px"]) and p["inlier_px"] > 0 and 0 <= p["iterations"] <= 64 and p["min_good"] >= 2 and 0 <= p["good10"] <= 10)


def kinv(K):
    """K (9,) f64 -> Kinv (9,) or None where the header refuses"""
    with np.errstate(all="ignore"):
        c00 = K[4] * K[8] - K[5] * K[7]; c01 = K[2] * K[7] - K[1] * K[8]; c02 = K[1] * K[5] - K[2] * K[4]
        c10 = K[5] * K[6] - K[3] * K[8]; c11 = K[0] * K[8] - K[2] * K[6]; c12 = K[2] * K[3] - K[0] * K[5]
        c20 = K[3] * K[7] - K[4] * K[6]; c21 = K[1] * K[6] - K[0] * K[7]; c22 = K[0] * K[4] - K[1] * K[3]
        det = (K[0] * c00 + K[1] * c10) + K[2] * c20
        if not np.isfinite(det) or det == 0.0:
            return None
        Ki = np.array([c00, c01, c02, c10, c11, c12, c20, c21, c22], f64) / det
    return Ki if np.isfinite(Ki).all() else None


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _entries(cam, kp, R, T, C, xy, Ki):
    """what depends on an entry alone: usable (O,), its camera Rm (O, 9) / Tm (O, 3), keypoint x (O, 2) f64, ray d (O, 3), centre c (O, 3)"""
    Cs, Kp = len(R), xy.shape[1]
    ok = (cam >= 0) & (cam < C) & (kp >= 0) & (kp < Kp)
    cs, ks = np.where(ok, cam, 0), np.where(ok, kp, 0)
    Rm, Tm = R[cs], T[cs]
    xf = xy[cs, ks]
    ok &= np.isfinite(Rm).all(1) & np.isfinite(Tm).all(1) & np.isfinite(xf).all(1)
    x = xf.astype(f64)
    with np.errstate(all="ignore"):
        b = [(Ki[3 * r] * x[:, 0] + Ki[3 * r + 1] * x[:, 1]) + Ki[3 * r + 2] for r in range(3)]
        dr = np.stack([(Rm[:, k] * b[0] + Rm[:, 3 + k] * b[1]) + Rm[:, 6 + k] * b[2] for k in range(3)], 1)
        nn = (dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2]
        ok &= np.isfinite(dr).all(1) & (nn > 0.0)
        d = dr / np.sqrt(nn)[:, None]
        c = np.stack([-((Rm[:, r] * Tm[:, 0] + Rm[:, 3 + r] * Tm[:, 1]) + Rm[:, 6 + r] * Tm[:, 2]) for r in range(3)], 1)
    return ok, Rm, Tm, x, d, c


class _Rows:
    """the rows of the points taking part, walked entry by entry: for k in rows: (sel, o) = the points that have a usable k-th entry,
    and that entry's index"""

    def __init__(self, o0, o1, usable):
        self.o0, self.len, self.usable = o0, o1 - o0, usable

    def __iter__(self):
        for k in range(int(self.len.max()) if len(self.len) else 0):
            has = self.len > k
            o = np.where(has, self.o0 + k, 0)
            yield has & self.usable[o], o


def _eval(K, E, rows, X, p):
    """cost, behind, V (6), g (3), n_good at X (P, 3) for every point of `rows`"""
    _, Rm, Tm, x, _, _ = E
    P = len(X)
    cost, behind, n_good = np.zeros(P), np.zeros(P, bool), np.zeros(P, np.int32)
    V, g = np.zeros((P, 6)), np.zeros((P, 3))
    delta = f64(p["huber_px"])
    r2 = f64(p["inlier_px"]) * f64(p["inlier_px"])
    with np.errstate(all="ignore"):
        for sel, o in rows:
            R, T = Rm[o], Tm[o]
            RX = np.stack([(R[:, 3 * r] * X[:, 0] + R[:, 3 * r + 1] * X[:, 1]) + R[:, 3 * r + 2] * X[:, 2] for r in range(3)], 1)
            Y = RX + T
            front = Y[:, 2] > 0.0
            behind |= sel & ~front
            use = sel & front
            u, v, q2 = rr.project(K, Y)
            r0, r1 = u - x[o, 0], v - x[o, 1]
            e = np.sqrt(r0 * r0 + r1 * r1)
            rho = np.where(e <= delta, e * e, (2.0 * delta) * e - delta * delta)
            cost = np.where(use, cost + rho, cost)
            n_good += use & np.isfinite(u) & np.isfinite(v) & (r0 * r0 + r1 * r1 <= r2)
            A = [[(K[k] - u * K[6 + k]) / q2 for k in range(3)], [(K[3 + k] - v * K[6 + k]) / q2 for k in range(3)]]
            J = [[(A[r][0] * R[:, k] + A[r][1] * R[:, 3 + k]) + A[r][2] * R[:, 6 + k] for k in range(3)] for r in range(2)]
            w = np.where(e <= delta, 1.0, delta / e)
            t = 0
            for i in range(3):
                for j in range(i, 3):
                    V[:, t] = np.where(use, V[:, t] + w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]), V[:, t])
                    t += 1
                g[:, i] = np.where(use, g[:, i] + w * (J[0][i] * r0 + J[1][i] * r1), g[:, i])
    return dict(cost=cost, behind=behind, V=V, g=g, n_good=n_good)


def triangulate_item(points, n_points, offsets, cam, kp, R, T, n_cams, xy, K, **kw):
    """points (S, 4) f32, offsets (S + 1,), cam / kp (O,), R (Cs, 9) / T (Cs, 3) f64, xy (Cs, Kp, 2) f32, K 3 x 3 f32 -> dict(out_points
    (S, 4) f32, status (S,), counts (S, 2), info (S, 3) f64, stats (4,))"""
    p = params(**kw)
    points = np.asarray(points, np.float32).reshape(-1, 4)
    offsets = np.asarray(offsets, np.int64)
    cam, kp = np.asarray(cam, np.int64), np.asarray(kp, np.int64)
    R, T = np.asarray(R, f64).reshape(-1, 9), np.asarray(T, f64).reshape(-1, 3)
    xy = np.asarray(xy, np.float32)
    Kd = np.asarray(K, np.float32).astype(f64).reshape(9)
    Ki = kinv(Kd)
    assert params_ok(p) and Ki is not None
    S, O, Cs = len(points), len(cam), len(R)
    n = min(max(int(n_points), 0), S)
    C = min(max(int(n_cams), 0), Cs)
    status = np.full(S, NO_PART, np.int32)
    counts = np.zeros((S, 2), np.int32)
    info = np.full((S, 3), 0, f64)
    info.view(np.uint64)[:] = QNAN64
    out_points = points.copy()
    o0, o1 = offsets[:-1], offsets[1:]
    part = np.flatnonzero((np.arange(S) < n) & (o0 >= 0) & (o0 < o1) & (o1 <= O))
    E = _entries(cam, kp, R, T, C, xy, Ki)
    usable, d_all, c_all = E[0], E[4], E[5]
    rows = _Rows(o0[part], o1[part], usable)
    P = len(part)
    # the parallax test
    m, d0, d1, best = np.zeros(P, np.int32), np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P)
    for sel, o in rows:
        d = d_all[o]
        first = sel & (m == 0)
        d0[first] = d[first]
        s = dot(d0, d)
        take = sel & ((m == 0) | (s < best))
        best[take] = s[take]
        d1[take] = d[take]
        m += sel
    cosp, seen = np.zeros(P), np.zeros(P, bool)
    A, r = np.zeros((P, 6)), np.zeros((P, 3))
    for sel, o in rows:
        d, c = d_all[o], c_all[o]
        s = dot(d1, d)
        take = sel & (~seen | (s < cosp))
        cosp[take] = s[take]
        seen |= sel
        M = [1.0 - d[:, 0] * d[:, 0], -(d[:, 0] * d[:, 1]), -(d[:, 0] * d[:, 2]), 1.0 - d[:, 1] * d[:, 1], -(d[:, 1] * d[:, 2]), 1.0 - d[:, 2] * d[:, 2]]
        for q in range(6):
            A[:, q] = np.where(sel, A[:, q] + M[q], A[:, q])
        r[:, 0] = np.where(sel, r[:, 0] + ((M[0] * c[:, 0] + M[1] * c[:, 1]) + M[2] * c[:, 2]), r[:, 0])
        r[:, 1] = np.where(sel, r[:, 1] + ((M[1] * c[:, 0] + M[3] * c[:, 1]) + M[4] * c[:, 2]), r[:, 1])
        r[:, 2] = np.where(sel, r[:, 2] + ((M[2] * c[:, 0] + M[4] * c[:, 1]) + M[5] * c[:, 2]), r[:, 2])
    st = np.full(P, -2, np.int32)                    # -2: not decided yet
    st[m < 2] = TOO_FEW
    st[(st == -2) & ~(cosp <= p["cos_parallax_max"])] = LOW_PARALLAX
    L, ok = ra.chol3(A, 0.0)
    with np.errstate(all="ignore"):
        X = ra.solve3(L, r)
    st[(st == -2) & ~(ok & np.isfinite(X).all(1))] = DEGENERATE
    live = np.flatnonzero(st == -2)                  # the points that are refined
    sub = _Rows(rows.o0[live], rows.o0[live] + rows.len[live], usable)
    X = X[live]
    cur = _eval(Kd, E, sub, X, p)
    lam = np.full(len(live), ra.LAMBDA0)
    active = np.ones(len(live), bool)
    for _ in range(p["iterations"]):
        if not active.any():
            break
        L, ok = ra.chol3(cur["V"], lam)
        with np.errstate(all="ignore"):
            Xn = X + (-ra.solve3(L, cur["g"]))
            cand = _eval(Kd, E, sub, Xn, p)
            accept = active & ok & np.isfinite(Xn).all(1) & ~cand["behind"] & (cand["cost"] < cur["cost"])
            rel = (cur["cost"] - cand["cost"]) / cur["cost"]
        refuse = active & ~accept
        X[accept] = Xn[accept]
        for k in cur:
            cur[k][accept] = cand[k][accept]
        lam[accept] = np.maximum(lam[accept] / 10.0, ra.LAMBDA_MIN)
        lam[refuse] = lam[refuse] * 10.0
        active &= ~(accept & (rel < ra.REL_STOP)) & ~(refuse & (lam > ra.LAMBDA_MAX))
    n_good = _eval(Kd, E, sub, X, p)["n_good"]
    Pin = points[part[live], :3]
    in_finite = np.isfinite(Pin).all(1)
    ev = _eval(Kd, E, sub, Pin.astype(f64), p)
    cost_in = np.where(ev["behind"], np.inf, ev["cost"])
    fin = np.full(len(live), OK, np.int32)
    worse = in_finite & np.isfinite(cost_in) & (cur["cost"] > cost_in)
    fin[worse] = WORSE
    fin[~((n_good >= p["min_good"]) & (10 * n_good >= p["good10"] * m[live]))] = UNSUPPORTED
    fin[cur["behind"]] = BEHIND
    st[live] = fin
    # the outputs
    status[part] = st
    counts[part, 0] = m
    counts[part[live], 1] = n_good
    info[part[m >= 2], 0] = cosp[m >= 2]
    info[part[live], 2] = cur["cost"]
    info[part[live][in_finite], 1] = cost_in[in_finite]
    good = live[fin == OK]
    out_points[part[good], :3] = X[fin == OK].astype(np.float32)
    out_points[part[good], 3] = 1.0
    stats = np.array([P, (st == OK).sum(), (st == LOW_PARALLAX).sum(), ((st != OK) & (st != LOW_PARALLAX)).sum()], np.int32)
    return dict(out_points=out_points, status=status, counts=counts, info=info, stats=stats, X=X, live=part[live])


def triangulate_batch(points, n_points, offsets, cam, kp, R, T, n_cams, xy, K, **kw):
    rs = [triangulate_item(points[b], n_points[b], offsets[b], cam[b], kp[b], R[b], T[b], n_cams[b], xy[b], K, **kw) for b in range(len(points))]
    return {k: np.stack([r[k] for r in rs]) for k in OUTS}


def world_item(world_points, size, offsets, frame, kp, Twc, frames, xy, K, **kw):
    """One track of vslam_world_retriangulate: world_points (P, 4) f32, the world's CSR, Twc (max_frames, 16), xy (xy_frames, Kp, 2)"""
    import ref_fuse as rf
    R, T = rf.cameras(np.asarray(Twc, f64).reshape(-1, 16), frames)
    xyc = np.zeros((len(R),) + xy.shape[1:], np.float32)
    xyc[:frames] = xy[:frames]
    return triangulate_item(world_points, size, offsets, frame, kp, R, T, frames, xyc, K, **kw)


# ------------------------------------------------------------------------------------------------ random items
def _rot(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def random_track_item(seed, n, cams, rows=None, cam_stride=None, S=None, noise_px=0.5, junk=0.2, kp_stride=None):
    """n points in front of `cams` cameras 0.25 apart on a line, rows of rows[0] .. rows[1] entries (1 .. cams when None) in distinct
    cameras, every keypoint the exact projection plus noise rounded to f32.  A tenth of the entries miss by 10 to 60 pixels; `junk`
    of them are unusable (camera out of range, keypoint out of range or NaN, one camera NaN); a few points lie very far away (no
    parallax), a few have the keypoints of their first and last entry swapped (rays that meet behind the cameras), a few see one
    camera only.  Input rows: the truth moved by up to 0.3 for most (a cost to compare against), NaN for a fifth."""
    rng = np.random.default_rng(seed)
    S, Cs = S or n, cam_stride or cams
    lo, hi = rows or (1, cams)
    K = rr.kmat()
    Kd = K.astype(f64)
    R, T = np.zeros((Cs, 9)), np.zeros((Cs, 3))
    for c in range(Cs):
        Rc = _rot(rng.normal(0, 0.02, 3))
        R[c] = Rc.reshape(9)
        T[c] = -Rc @ np.array([0.25 * (c - (cams - 1) / 2) * (6.0 / max(cams, 6)), rng.normal(0, 0.02), rng.normal(0, 0.02)])
    if cams > 3:
        R[cams // 2, 4] = np.nan
    truth = np.stack([rng.uniform(-1.2, 1.2, S), rng.uniform(-0.9, 0.9, S), rng.uniform(4, 9, S)], 1)
    far = rng.uniform(size=S) < 0.04
    truth[far, 2] = rng.uniform(2e3, 2e4, far.sum())
    points = np.ones((S, 4), np.float32)
    points[:, :3] = truth + rng.uniform(-0.3, 0.3, (S, 3))
    points[rng.uniform(size=S) < 0.2, :3] = np.nan
    counts = rng.integers(lo, hi + 1, S)
    counts[rng.uniform(size=S) < 0.02] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    O = max(int(offsets[-1]), 1)
    cam, kp = np.zeros(O, np.int32), np.zeros(O, np.int32)
    per_cam = np.zeros(Cs, np.int64)
    for i in range(S):
        cs = rng.permutation(cams)[:counts[i]]
        if rng.uniform() < 0.03 and counts[i] >= 2:
            cs[:] = cs[0]                               # one camera only: one ray several times over
        cam[offsets[i]:offsets[i + 1]] = cs
        for j, c in enumerate(cs):
            kp[offsets[i] + j] = per_cam[c]
            per_cam[c] += 1
    Kp = kp_stride or int(per_cam.max()) + 2
    xy = rng.uniform(0, 640, (Cs, Kp, 2)).astype(np.float32)
    owner = np.repeat(np.arange(S), counts)
    Rm, Tm = R[cam].reshape(-1, 3, 3), T[cam]
    with np.errstate(all="ignore"):
        Y = np.einsum("oij,oj->oi", Rm, truth[owner]) + Tm
        q = Y @ Kd.T
        uv = q[:, :2] / q[:, 2:] + rng.normal(0, noise_px, (len(owner), 2)) if noise_px else q[:, :2] / q[:, 2:]
    miss = rng.uniform(size=len(owner)) < 0.1
    a = rng.uniform(0, 2 * np.pi, len(owner))
    uv = uv + np.where(miss, rng.uniform(10, 60, len(owner)), 0.0)[:, None] * np.stack([np.cos(a), np.sin(a)], 1)
    for i in np.flatnonzero((rng.uniform(size=S) < 0.04) & (counts >= 2)):
        f, l = offsets[i], offsets[i + 1] - 1
        uv[[f, l]] = uv[[l, f]]
    xy[cam[:len(owner)], kp[:len(owner)]] = uv.astype(np.float32)
    bad = rng.uniform(size=O) < junk
    kind = rng.integers(0, 3, O)
    xy[cam[bad & (kind == 0)], kp[bad & (kind == 0)], 0] = np.nan
    cam[bad & (kind == 1)] = rng.choice([-1, cams, Cs + 3])
    kp[bad & (kind == 2)] = rng.choice([-2, Kp])
    return dict(points=points, n=n, offsets=offsets, cam=cam, kp=kp, R=R, T=T, n_cams=cams, xy=xy, K=K, truth=truth)


def batch_tracks(items):
    """items of different sizes padded into one batch: the strides are the largest; padding rows are NaN points with empty rows"""
    S, O = max(len(it["points"]) for it in items), max(len(it["cam"]) for it in items)
    Cs, Kp = max(len(it["R"]) for it in items), max(it["xy"].shape[1] for it in items)
    B = len(items)
    b = dict(points=np.full((B, S, 4), np.nan, np.float32), n=np.array([it["n"] for it in items], np.int32), offsets=np.zeros((B, S + 1), np.int32),
             cam=np.zeros((B, O), np.int32), kp=np.zeros((B, O), np.int32), R=np.zeros((B, Cs, 9)), T=np.zeros((B, Cs, 3)),
             n_cams=np.array([it["n_cams"] for it in items], np.int32), xy=np.zeros((B, Cs, Kp, 2), np.float32))
    for i, it in enumerate(items):
        s, o, c, k = len(it["points"]), len(it["cam"]), len(it["R"]), it["xy"].shape[1]
        b["points"][i, :s], b["offsets"][i, :s + 1], b["offsets"][i, s + 1:] = it["points"], it["offsets"], it["offsets"][-1]
        b["cam"][i, :o], b["kp"][i, :o], b["R"][i, :c], b["T"][i, :c], b["xy"][i, :c, :k] = it["cam"], it["kp"], it["R"], it["T"], it["xy"]
    return b


def batch_reference(b, K, **kw):
    return triangulate_batch(b["points"], b["n"], b["offsets"], b["cam"], b["kp"], b["R"], b["T"], b["n_cams"], b["xy"], K, **kw)


# ------------------------------------------------------------------------------------------------ accuracy, read on this reference
def from_problem(pr, two_view=False):
    """A ref_adjust.problem scene under its TRUE cameras as an item: keypoint i of camera c is point i's observation there.  Input rows
    are NaN (no start is needed).  two_view: tools/fuse_adjust_cpu.py's construction -- every physical point as the two-view map points
    (c, c + 1), c = 0 .. cams - 2, each a row of its own -- instead of one row of all its observations."""
    cams, P = len(pr["R_true"]), len(pr["X_true"])
    xy = np.zeros((cams, P, 2), np.float32)
    pid = np.repeat(np.arange(P), np.diff(pr["off"]))
    xy[pr["cam"], pid] = pr["xy"]
    if two_view:
        cam = np.array([[c, c + 1] for _ in range(P) for c in range(cams - 1)], np.int32).reshape(-1)
        kp = np.repeat(np.arange(P), 2 * (cams - 1)).astype(np.int32)
        off = np.arange(0, len(cam) + 1, 2, dtype=np.int32)
        truth = np.repeat(pr["X_true"], cams - 1, 0)
    else:
        cam, kp, off, truth = pr["cam"], pid.astype(np.int32), pr["off"], pr["X_true"]
    S = len(off) - 1
    return dict(points=np.full((S, 4), np.nan, np.float32), n=S, offsets=off, cam=cam, kp=kp, R=pr["R_true"], T=pr["T_true"], n_cams=cams, xy=xy,
                K=ra.kmat(), truth=truth)


def distances(item, **kw):
    """-> (statuses, |X - X_true| per point from the f64 result, before it is rounded to f32; NaN where the point was not refined)"""
    r = triangulate_item(item["points"], item["n"], item["offsets"], item["cam"], item["kp"], item["R"], item["T"], item["n_cams"], item["xy"],
                         item["K"], **kw)
    d = np.full(len(r["status"]), np.nan)
    d[r["live"]] = np.linalg.norm(r["X"] - item["truth"][r["live"]], axis=1)
    return r["status"], d


# (a) exact projections rounded to f32, true cameras, ref_adjust.EXACT_SHAPE over EXACT_SEEDS: the worst |X - X_true| per seed as
# tools/tracks_cpu.py prints it; the bound asserted is 4 x the worst of them (the error is the f32 rounding of the keypoints amplified
# by depth over baseline, which varies several-fold between seeds)
EXACT_WORST = {1: 4.120e-06, 3: 4.135e-06, 4: 2.744e-06, 5: 3.351e-06, 7: 3.298e-06, 8: 3.932e-06}
EXACT_BOUND = 1.66e-5   # 4 x 4.135e-06 = 1.654e-05, rounded up
# (b) 0.5 px of keypoint noise: median |X - X_true| of the six-view rows and of the two-view rows (c, c + 1), per seed, as measured
NOISY_MEDIANS = {1: (0.04015, 0.07814), 3: (0.04617, 0.09982), 4: (0.03249, 0.12120), 5: (0.03881, 0.10369), 7: (0.03597, 0.11063),
                 8: (0.04027, 0.12318)}
