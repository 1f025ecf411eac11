"""include/vslam_graph.h restated in numpy f64, written from the header's text: the residual of an edge, its two analytic Jacobians,
the usable-edge and left-alone rules, the Levenberg-Marquardt schedule and the block-Jacobi preconditioned conjugate gradient
(optimize), and vslam_world_close_loops' gather and write-back (close_loops).  The arithmetic is the header's, vectorised over the
edges and nodes: numpy's sums do not run in the device's order, and the library sine differs; that is what DELTA_REF is for.

  second_formulation()  the same minimum another way: scipy.optimize.least_squares over the same residuals, built from 4 x 4
                        homogeneous products and numeric derivatives, run to convergence.
  numeric_jacobian()    central differences of the residual through the update; JACOBIAN_WORST is the measured worst entry against
                        the analytic blocks.
  consistent()          edges built from a truth, nodes started 1 degree / 3 % / 0.05 off: the minimum is the truth, cost 0.
  drifting()            a circular track with 1 % scale drift per frame and 0.004 rad of rotation noise per pair, one loop edge.
  star()                every edge at one hub, in both directions and many per pair, every measurement noisy: the minimum costs > 0.
  weighted(), perturbed()  an item with per-edge, per-group weights from [0.25, 4]; with every measurement moved off the truth's.

At a minimum with cost > 0 the 2^-40 stop rule and the CG tolerance leave the nodes determined to about 1e-8 only, and two correct
implementations may take different numbers of CG iterations.  FLOW takes the flow out of the comparison: under cg_tolerance = 1e-30
and small caps every solve runs exactly cg_iterations and the outer loop exactly max_iterations, and what is left between two
implementations is rounding (DELTA_FLOW).  info["cg_ratio"] (rho' / rho_0 at each solve's exit) says that the conjugate gradient was
still far above its rounding floor when it was cut: past convergence it only amplifies noise.
"""
import numpy as np

DEFAULTS = dict(max_iterations=20, cg_iterations=2048, cg_tolerance=1e-8)
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, REL_STOP, DIAG_FLOOR = 1e-3, 1e-15, 1e12, 2.0 ** -40, 2.0 ** -40
MAX_NODES, MAX_EDGES = 4096, 8192

JACOBIAN_WORST = 1.8e-9      # measured over JACOBIAN_CASES at h = 1e-5: 1.76e-9, analytic against central differences
JACOBIAN_BOUND = 4 * JACOBIAN_WORST
DELTA_REF = 1.2e-14          # measured over CONSISTENT_CASES: 1.11e-14 between optimize() and second_formulation()
DRIFT_WORST = 0.092          # measured over DRIFT_CASES: the worst (centre error after) / (centre error before), 0.0918
DRIFT_BOUND = 0.5            # the issue's
FLOW = dict(cg_tolerance=1e-30)   # with max_iterations in 1 .. 3 and a small cg_iterations: both loops run exactly to their caps
FLOW_RATIO = 1e-4            # a fixed-flow case is valid when every solve ends at its cap with rho' / rho_0 >= this
CONVERGED = dict(max_iterations=64, cg_iterations=2048, cg_tolerance=1e-8)
DELTA_FLOW = 5.4e-15         # measured over graph_cases.LOOP_CASES under their fixed flow: 5.33e-15 between optimize() and the serial walk
# Run to convergence, two correct implementations agree to rounding while their flows coincide and to about 1e-8 sqrt(cost) once one
# of them takes another number of CG iterations: measured between optimize() and the serial walk over graph_cases.CONVERGED_CASES
# and WEIGHT_CASES, 4.13e-9 on weighted_drift(16, 2) (848 against 1312 CG iterations) and at most 6.0e-12 on the others
CONVERGED_NODES = 4.2e-9
CONVERGED_COST = 5.0e-15     # over the same cases: 4.996e-15, the final cost's relative difference
WEIGHT_WORST = 6.4e-8        # measured over WEIGHT_CASES: 6.33e-8 between optimize() and second_formulation(); unit weights end >= 3.3e-2 away
WEIGHT_BOUND = 16 * WEIGHT_WORST
WEIGHT_CASES = [(n, s) for n in (16, 48) for s in range(3)]   # drifting(N, seed, extra=((N // 2, 1),)) under weighted(seed)

JACOBIAN_CASES = list(range(20))
CONSISTENT_CASES = [(n, l, s) for n, l in ((2, 0), (3, 1), (5, 2), (64, 2)) for s in (0, 1, 2, 4)]   # N, loops, seed
CONSISTENT_PRM = dict(max_iterations=64)   # at cost 0 the iteration ends by refusals, lambda from about 1e-10 to 1e12: more than 20
DRIFT_CASES = [(n, s) for n in (16, 48) for s in range(4)]


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(k)
        p[k] = v
    return p


# ------------------------------------------------------------------------------------------------ rotations
def rotate(w, R):
    """exp([w]x) R as lm_math.h's lm_rotate forms it; w (..., 3), R (..., 3, 3)"""
    w = np.asarray(w, np.float64)
    th2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    small = th2 < 2.0 ** -26
    safe = np.where(small, 1.0, th2)
    th = np.sqrt(safe)
    s = np.sin(0.5 * th)
    a = np.where(small, 1.0 - th2 / 6.0, np.sin(th) / th)
    b = np.where(small, 0.5 - th2 / 24.0, ((2.0 * s) * s) / safe)
    eye = np.eye(3)
    E = b[..., None, None] * (w[..., :, None] * w[..., None, :] - th2[..., None, None] * eye) + eye
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -w[..., 2], w[..., 1]
    K[..., 1, 0], K[..., 1, 2] = w[..., 2], -w[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -w[..., 1], w[..., 0]
    return (E + a[..., None, None] * K) @ R


def polar_step(R):
    """R (3 I - R^t R) / 2"""
    G = 3.0 * np.eye(3) - np.swapaxes(R, -1, -2) @ R
    return 0.5 * (R @ G)


def vee(X):
    return np.stack([(X[..., 2, 1] - X[..., 1, 2]) / 2.0, (X[..., 0, 2] - X[..., 2, 0]) / 2.0, (X[..., 1, 0] - X[..., 0, 1]) / 2.0], -1)


# ------------------------------------------------------------------------------------------------ the edge
def residuals(sa, Ra, ta, sb, Rb, tb, zs, ZR, zt):
    """r (E, 7) of the header, every argument with a leading edge axis"""
    sp = sa / sb
    Rp = np.einsum("eki,ekj->eij", Rb, Ra)
    v = ta - tb
    tp = np.einsum("eki,ek->ei", Rb, v) / sb[:, None]
    se = sp / zs
    Re = np.einsum("eki,ekj->eij", ZR, Rp)
    te = np.einsum("eki,ek->ei", ZR, tp - zt) / zs[:, None]
    return np.concatenate([vee(Re), te, (se - 1.0)[:, None]], 1)


def jacobians(sa, Ra, ta, sb, Rb, tb, zs, ZR, zt):
    """the header's analytic J_a, J_b (E, 7, 7) at d = 0"""
    E = len(sa)
    Q = np.einsum("eki,ejk->eij", ZR, Rb)
    v = ta - tb
    tp = np.einsum("eki,ek->ei", Rb, v) / sb[:, None]
    se = (sa / sb) / zs
    A, Bw = np.zeros((E, 3, 3)), np.zeros((E, 3, 3))
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        D = Q[:, :, k2, None] * Ra[:, None, k1, :] - Q[:, :, k1, None] * Ra[:, None, k2, :]
        A[:, :, k] = vee(D)
        Bw[:, :, k] = -(((Q[:, :, k2] * v[:, k1, None] - Q[:, :, k1] * v[:, k2, None]) / sb[:, None]) / zs[:, None])
    T = (Q / sb[:, None, None]) / zs[:, None, None]
    bs = -(np.einsum("eki,ek->ei", ZR, tp) / zs[:, None])
    Ja, Jb = np.zeros((E, 7, 7)), np.zeros((E, 7, 7))
    Ja[:, :3, :3], Ja[:, 3:6, 3:6], Ja[:, 6, 6] = A, T, se
    Jb[:, :3, :3], Jb[:, 3:6, :3], Jb[:, 3:6, 3:6], Jb[:, 3:6, 6], Jb[:, 6, 6] = -A, Bw, -T, bs, -se
    return Ja, Jb


def update(s, R, t, d):
    """a node's update d = (w, tau, sigma); leading axes broadcast"""
    d = np.asarray(d, np.float64)
    return s * (1.0 + d[..., 6]), rotate(d[..., :3], R), t + d[..., 3:6]


def numeric_jacobian(a, b, Z, h=1e-5):
    """central differences of the residual of one edge through the update of each side: a, b, Z = (s, R (3, 3), t) -> J_a, J_b (7, 7)"""
    one = lambda n: (np.array([n[0]], np.float64), np.asarray(n[1], np.float64).reshape(1, 3, 3), np.asarray(n[2], np.float64).reshape(1, 3))
    za = one(Z)
    out = []
    for side in (0, 1):
        J = np.zeros((7, 7))
        for k in range(7):
            r = []
            for sign in (1.0, -1.0):
                d = np.zeros(7)
                d[k] = sign * h
                na, nb = one(a), one(b)
                if side == 0:
                    na = one(update(a[0], np.asarray(a[1]).reshape(3, 3), np.asarray(a[2]), d))
                else:
                    nb = one(update(b[0], np.asarray(b[1]).reshape(3, 3), np.asarray(b[2]), d))
                r.append(residuals(*na, *nb, *za)[0])
            J[:, k] = (r[0] - r[1]) / (2.0 * h)
        out.append(J)
    return out


# ------------------------------------------------------------------------------------------------ the graph
def usable_edges(N, E, fixed, ab, zs, zR, zt, zw):
    ab = np.asarray(ab).reshape(-1, 2)[:E].astype(np.int64)
    a, b = ab[:, 0], ab[:, 1]
    ok = (a >= 0) & (a < N) & (b >= 0) & (b < N) & (a != b)
    fx = np.asarray(fixed)[:N] != 0
    both = np.zeros(E, bool)
    both[ok] = fx[a[ok]] & fx[b[ok]]
    zfin = np.isfinite(zs[:E]) & np.isfinite(zR[:E].reshape(E, 9)).all(1) & np.isfinite(zt[:E]).all(1)
    with np.errstate(invalid="ignore"):
        wfin = (np.isfinite(zw[:E]) & (zw[:E] >= 0)).all(1)
        pos = zs[:E] > 0
    return ok & ~both & zfin & pos & wfin


def _cost(s, R, t, a, b, zs, zR, zt, zw):
    r = residuals(s[a], R[a], t[a], s[b], R[b], t[b], zs, zR, zt)
    return float(np.sum((zw[:, 0] * ((r[:, 0] ** 2 + r[:, 1] ** 2) + r[:, 2] ** 2) + zw[:, 1] * ((r[:, 3] ** 2 + r[:, 4] ** 2) + r[:, 5] ** 2))
                        + zw[:, 2] * r[:, 6] ** 2))


def optimize(scale, R, T, fixed, n_nodes, ab, zs, zR, zt, zw, n_edges, **prm):
    """vslam_graph_optimize on one item: scale (S,), R (S, 9), T (S, 3), fixed (S,), ab (Es, 2), zs (Es,), zR (Es, 9), zt (Es, 3), zw (Es, 3).
    -> (scale, R, T as the call leaves them, stats (4,), info: written (S,) bool, cg (iterations of every solve), cg_capped, lm_capped)"""
    p = params(**prm)
    scale, R, T = np.array(scale, np.float64), np.array(R, np.float64).reshape(-1, 9), np.array(T, np.float64).reshape(-1, 3)
    S, Es = len(scale), len(np.asarray(zs))
    N, E = int(n_nodes), int(n_edges)
    nan = float("nan")
    stats = np.array([0.0, nan, nan, nan])
    info = dict(written=np.zeros(S, bool), cg=[], cg_ratio=[], cg_capped=False, lm_capped=False, moved=False, steps=0, accepted=0)
    if N < 1 or N > S or E < 0 or E > Es:
        return scale, R, T, stats, info
    zs, zR, zt, zw = (np.asarray(v, np.float64) for v in (zs, zR, zt, zw))
    zR, zt, zw = zR.reshape(Es, 9), zt.reshape(Es, 3), zw.reshape(Es, 3)
    use = usable_edges(N, E, fixed, ab, zs, zR, zt, zw)
    stats[0] = float(use.sum())
    fx = np.asarray(fixed)[:N] != 0
    nodes_ok = np.isfinite(scale[:N]).all() and np.isfinite(R[:N]).all() and np.isfinite(T[:N]).all() and (scale[:N] > 0).all()
    if not nodes_ok or not fx.any() or not use.any():
        return scale, R, T, stats, info
    idx = np.flatnonzero(use)
    abu = np.asarray(ab).reshape(-1, 2)[idx].astype(np.int64)
    a, b = abu[:, 0], abu[:, 1]
    zs, zR, zt, zw = zs[idx], zR[idx].reshape(-1, 3, 3), zt[idx], zw[idx]
    W = np.stack([zw[:, 0]] * 3 + [zw[:, 1]] * 3 + [zw[:, 2]], 1)
    deg = np.bincount(np.concatenate([a, b]), minlength=N)
    active = ~fx & (deg > 0)
    s, Rm, t = scale[:N].copy(), R[:N].reshape(N, 3, 3).copy(), T[:N].copy()
    Rm[~fx] = polar_step(Rm[~fx])
    obj0 = obj = _cost(s, Rm, t, a, b, zs, zR, zt, zw)
    lam, accepted = LAMBDA0, 0
    stopped = False
    for _ in range(p["max_iterations"]):
        info["steps"] += 1
        r = residuals(s[a], Rm[a], t[a], s[b], Rm[b], t[b], zs, zR, zt)
        Ja, Jb = jacobians(s[a], Rm[a], t[a], s[b], Rm[b], t[b], zs, zR, zt)
        H, g = np.zeros((N, 7, 7)), np.zeros((N, 7))
        for J, n in ((Ja, a), (Jb, b)):
            WJ = W[:, :, None] * J
            np.add.at(H, n, np.einsum("eik,eil->ekl", WJ, J))
            np.add.at(g, n, np.einsum("eik,ei->ek", WJ, r))
        H[~active], g[~active] = 0.0, 0.0
        damp = lam * np.maximum(np.einsum("nii->ni", H), DIAG_FLOOR)
        x, ok = _pcg(H, g, damp, active, Ja, Jb, W, a, b, p, info)
        accept = False
        if ok:
            cs, cR, ct = s.copy(), Rm.copy(), t.copy()
            cs[active], cR[active], ct[active] = update(s[active], Rm[active], t[active], x[active])
            if (cs > 0).all():
                new = _cost(cs, cR, ct, a, b, zs, zR, zt, zw)
                accept = new < obj
        if accept:
            rel = (obj - new) / obj
            s, Rm, t, obj = cs, cR, ct, new
            accepted += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            if rel < REL_STOP:
                stopped = True
                break
        else:
            lam = lam * 10.0
            if lam > LAMBDA_MAX:
                stopped = True
                break
    info["lm_capped"] = not stopped
    info["accepted"] = accepted
    if accepted == 0:
        return scale, R, T, stats, info
    s1, s2 = obj0 / stats[0], obj / stats[0]
    if not (np.isfinite(s[active]).all() and np.isfinite(Rm[active]).all() and np.isfinite(t[active]).all() and np.isfinite(s1) and np.isfinite(s2)):
        return scale, R, T, stats, info
    stats[1:] = s1, s2, float(accepted)
    w = np.flatnonzero(active)
    scale[w], R[w], T[w] = s[w], Rm[w].reshape(-1, 9), t[w]
    info["written"][w] = True
    info["moved"] = True
    return scale, R, T, stats, info


def _pcg(H, g, damp, active, Ja, Jb, W, a, b, p, info):
    """(H + lambda D) x = -g by the header's conjugate gradient -> (x, False when the step is refused)"""
    N = len(g)
    M = H + np.einsum("ni,ij->nij", damp, np.eye(7))
    M[~active] = np.eye(7)
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None, False
    Minv = np.linalg.inv(L)
    Minv = np.einsum("nki,nkj->nij", Minv, Minv)
    act = active[:, None].astype(np.float64)

    def prec(r):
        return np.einsum("nij,nj->ni", Minv, r) * act

    def op(v):
        y = W * (np.einsum("eij,ej->ei", Ja, v[a]) + np.einsum("eij,ej->ei", Jb, v[b]))
        q = np.zeros((N, 7))
        np.add.at(q, a, np.einsum("eij,ei->ej", Ja, y))
        np.add.at(q, b, np.einsum("eij,ei->ej", Jb, y))
        return (q + damp * v) * act

    x = np.zeros((N, 7))
    r = -g * act
    z = prec(r)
    pv = z.copy()
    rho = rho0 = float(np.sum(r * z))
    it, last = 0, rho
    for it in range(1, p["cg_iterations"] + 1):
        q = op(pv)
        pq = float(np.sum(pv * q))
        if not (pq > 0.0) or not np.isfinite(pq):
            if it == 1:
                return None, False
            it -= 1
            break
        alpha = rho / pq
        x = x + alpha * pv
        r = r - alpha * q
        z = prec(r)
        new = last = float(np.sum(r * z))
        if new <= p["cg_tolerance"] * rho0:
            break
        if it == p["cg_iterations"]:
            info["cg_capped"] = True
            break
        pv = z + (new / rho) * pv
        rho = new
    info["cg"].append(it)
    info["cg_ratio"].append(last / rho0)
    return x, True


# ------------------------------------------------------------------------------------------------ another way to the same minimum
def second_formulation(scale, R, T, fixed, n_nodes, ab, zs, zR, zt, zw, n_edges):
    """the minimum of the same cost by scipy.optimize.least_squares over the active nodes' updates, the residuals built from 4 x 4
    homogeneous products, run to convergence -> (scale, R, T)"""
    from scipy.optimize import least_squares
    N, E = int(n_nodes), int(n_edges)
    scale, R, T = np.array(scale, np.float64), np.array(R, np.float64).reshape(-1, 9), np.array(T, np.float64).reshape(-1, 3)
    zs, zR, zt, zw = (np.asarray(v, np.float64) for v in (zs, zR, zt, zw))
    use = np.flatnonzero(usable_edges(N, E, fixed, ab, zs, zR.reshape(-1, 9), zt.reshape(-1, 3), zw.reshape(-1, 3)))
    abu = np.asarray(ab).reshape(-1, 2)[use]
    fx = np.asarray(fixed)[:N] != 0
    active = np.flatnonzero(~fx & (np.bincount(abu.reshape(-1), minlength=N) > 0))

    def hom(s, Rm, t):
        """(n,), (n, 3, 3), (n, 3) -> (n, 4, 4)"""
        M = np.zeros((len(s), 4, 4))
        M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = s[:, None, None] * Rm, t, 1.0
        return M

    zRu, ztu = zR.reshape(-1, 3, 3)[use], zt.reshape(-1, 3)[use]
    Zinv = np.linalg.inv(hom(zs[use], zRu, ztu))
    sq = np.sqrt(zw.reshape(-1, 3)[use])
    Rs = R[:N].reshape(N, 3, 3).copy()
    Rs[~fx] = polar_step(Rs[~fx])
    start = [scale[:N].copy(), Rs, T[:N].copy()]

    def nodes_of(v):
        out = [a.copy() for a in start]
        out[0][active], out[1][active], out[2][active] = update(start[0][active], start[1][active], start[2][active], v.reshape(-1, 7))
        return out

    def fun(v):
        nd = hom(*nodes_of(v))
        Em = Zinv @ np.linalg.inv(nd[abu[:, 1]]) @ nd[abu[:, 0]]
        sR = Em[:, :3, :3]
        se = np.cbrt(np.linalg.det(sR))
        return np.concatenate([sq[:, :1] * vee(sR / se[:, None, None]), sq[:, 1:2] * Em[:, :3, 3], sq[:, 2:] * (se - 1.0)[:, None]], 1).reshape(-1)

    v = np.zeros(7 * len(active))
    for _ in range(3):   # re-centre the update: the result is the composition, as the iteration's is
        sol = least_squares(fun, v, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0, max_nfev=100)
        start = nodes_of(sol.x)
        v = np.zeros_like(v)
    scale[active], R[active], T[active] = start[0][active], start[1][active].reshape(-1, 9), start[2][active]
    return scale, R, T


def distance(got, want, written):
    """entry-wise between two results over the written nodes: s relative, R and t absolute"""
    w = np.flatnonzero(written)
    if not len(w):
        return 0.0
    return max(float(np.abs(got[0][w] / want[0][w] - 1.0).max()), float(np.abs(got[1][w] - want[1][w]).max()),
               float(np.abs(got[2][w] - want[2][w]).max()))


# ------------------------------------------------------------------------------------------------ scenes
def random_rotation(rng, angle):
    ax = rng.normal(size=3)
    return rotate(angle * ax / np.linalg.norm(ax), np.eye(3))


def relative(na, nb):
    """Z = S_b^-1 S_a of two nodes (s, R (3, 3), t)"""
    return na[0] / nb[0], nb[1].T @ na[1], nb[1].T @ (na[2] - nb[2]) / nb[0]


def pack(nodes, edges, fixed, node_stride=None, edge_stride=None, weights=(1.0, 1.0, 1.0)):
    """nodes [(s, R, t)], edges [(a, b, (z_s, Z_R, z_t))] as one item's arrays, NaN / -1 in the padding"""
    N, E = len(nodes), len(edges)
    S, Es = node_stride or N, edge_stride or max(E, 1)
    it = dict(scale=np.full(S, np.nan), R=np.full((S, 9), np.nan), T=np.full((S, 3), np.nan), fixed=np.zeros(S, np.int32), n_nodes=N,
              ab=np.full((Es, 2), -1, np.int32), zs=np.full(Es, np.nan), zR=np.full((Es, 9), np.nan), zt=np.full((Es, 3), np.nan),
              zw=np.full((Es, 3), np.nan), n_edges=E)
    for i, (s, R, t) in enumerate(nodes):
        it["scale"][i], it["R"][i], it["T"][i] = s, np.asarray(R).reshape(9), t
    it["fixed"][list(fixed)] = 1
    for k, (a, b, Z) in enumerate(edges):
        it["ab"][k] = a, b
        it["zs"][k], it["zR"][k], it["zt"][k], it["zw"][k] = Z[0], np.asarray(Z[1]).reshape(9), Z[2], weights
    return it


def args(it):
    return (it["scale"], it["R"], it["T"], it["fixed"], it["n_nodes"], it["ab"], it["zs"], it["zR"], it["zt"], it["zw"], it["n_edges"])


def consistent(N, loops, seed, node_stride=None, edge_stride=None, fixed_every=None):
    """a chain of N nodes along a curve plus `loops` further edges, every edge the truth's relation; node 0 fixed at the truth, the
    others started 1 degree / 3 % / 0.05 off -> (item, truth nodes).  fixed_every = m also holds nodes m, 2 m, ... at the truth: the chain
    falls into short pieces and the conjugate gradient needs few iterations however long the chain is (the header: its iterations
    grow with the length of the track), which keeps the large shapes of the tests quick."""
    rng = np.random.default_rng(1000 * N + seed)
    held = set(range(0, N, fixed_every)) if fixed_every else {0}
    truth = []
    for i in range(N):
        ang = 2.0 * np.pi * i / max(N, 8)
        truth.append((float(rng.uniform(0.8, 1.25)), rotate(np.array([0.0, ang, 0.0]), np.eye(3)) @ random_rotation(rng, 0.2),
                      np.array([5.0 * np.cos(ang), 0.3 * rng.normal(), 5.0 * np.sin(ang)])))
    pairs = [(i, i + 1) for i in range(N - 1)]
    while len(pairs) < N - 1 + loops:
        a, b = sorted(int(v) for v in rng.integers(0, N, 2))
        if b - a >= 2 and (a, b) not in pairs and (b, a) not in pairs:
            pairs.append((b, a) if len(pairs) % 2 else (a, b))
    edges = [(a, b, relative(truth[a], truth[b])) for a, b in pairs]
    nodes = []
    for i, (s, R, t) in enumerate(truth):
        d = rng.normal(size=3)
        off = (s * (1.0 + 0.03 * rng.choice([-1.0, 1.0])), random_rotation(rng, np.radians(1.0)) @ R, t + 0.05 * d / np.linalg.norm(d))
        nodes.append(truth[i] if i in held else off)
    return pack(nodes, edges, sorted(held), node_stride, edge_stride), truth


def drifting(N, seed, extra=()):
    """the prototype's recipe: N frames on a circle of radius 5 looking along the track, sequential edges measured with 1 % scale
    drift per frame and 0.004 rad of rotation noise per pair, the nodes composed from them (so the start carries the drift), and one
    loop edge (N - 1 -> 0) from the truth, and one more for every (a, b) of `extra` -> (item, truth nodes)"""
    rng = np.random.default_rng(77 * N + seed)
    truth = []
    for i in range(N):
        ang = 2.0 * np.pi * i / N
        truth.append((1.0, rotate(np.array([0.0, -ang, 0.0]), np.eye(3)), np.array([5.0 * np.cos(ang), 0.0, 5.0 * np.sin(ang)])))
    edges, nodes = [], [truth[0]]
    for i in range(N - 1):
        zs, zR, zt = relative(truth[i], truth[i + 1])
        Z = (zs * 1.01, random_rotation(rng, 0.004) @ zR, zt)
        edges.append((i, i + 1, Z))
        sa, Ra, ta = nodes[-1]   # S_b = S_a Z^-1
        sb = sa / Z[0]
        Rb = Ra @ Z[1].T
        nodes.append((sb, Rb, ta - sb * (Rb @ Z[2])))
    for a, b in [(N - 1, 0)] + list(extra):
        edges.append((a, b, relative(truth[a], truth[b])))
    return pack(nodes, edges, [0]), truth


def noisy(Z, rng, rot=0.004, trans=0.02, scale=0.01):
    """a measurement moved off: about `rot` rad, `trans` and `scale` relative"""
    return Z[0] * (1.0 + scale * rng.normal()), random_rotation(rng, rot * rng.uniform(0.5, 1.5)) @ Z[1], Z[2] + trans * rng.normal(size=3)


def star(N, hub, E, seed, leaves, ring=0, node_stride=None, edge_stride=None):
    """E edges, every one between `hub` (free) and one of `leaves` in turn, written (hub, leaf) and (leaf, hub) alternately, so
    every pair has many edges in both directions when E > len(leaves) -- but the last `ring` edges, which join each leaf to the next
    (without them block-Jacobi all but solves a star, and the conjugate gradient is at its floor after two iterations); every
    measurement noisy(); node 0 held at the truth, the others started 1 degree / 3 % / 0.05 off; a node that is neither the hub nor
    a leaf has no edge -> (item, truth nodes)"""
    rng = np.random.default_rng(9000 * N + seed)
    truth = [(float(rng.uniform(0.8, 1.25)), random_rotation(rng, rng.uniform(0.0, 1.0)), 3.0 * rng.normal(size=3)) for _ in range(N)]
    edges = []
    for k in range(E):
        leaf = leaves[k % len(leaves)]
        a, b = (hub, leaf) if (k + k // len(leaves)) % 2 else (leaf, hub)
        if k >= E - ring:
            a, b = leaf, leaves[(k + 1) % len(leaves)]
        edges.append((a, b, noisy(relative(truth[a], truth[b]), rng)))
    nodes = [truth[0]]
    for s, R, t in truth[1:]:
        d = rng.normal(size=3)
        nodes.append((s * (1.0 + 0.03 * rng.choice([-1.0, 1.0])), random_rotation(rng, np.radians(1.0)) @ R, t + 0.05 * d / np.linalg.norm(d)))
    return pack(nodes, edges, [0], node_stride, edge_stride), truth


def _copy(it):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in it.items()}


def weighted_drift(N, seed):
    """drifting(N, seed) with one more loop N // 2 -> 1 (both loops are written from the later frame to the earlier one), weighted
    -> (item, truth nodes)"""
    it, truth = drifting(N, seed, extra=((N // 2, 1),))
    return weighted(it, N + seed), truth


def weighted(it, seed, zero=None):
    """a copy of the item with every edge's three weights drawn from [0.25, 4] (2^u, u uniform); zero = (edge, group) sets that one to 0"""
    it = _copy(it)
    E = int(it["n_edges"])
    it["zw"][:E] = 2.0 ** np.random.default_rng(31337 + seed).uniform(-2.0, 2.0, (E, 3))
    if zero is not None:
        it["zw"][zero] = 0.0
    return it


def perturbed(it, seed, rot=0.004, trans=0.02, scale=0.01):
    """a copy of the item with every measurement moved off: about `rot` rad, `trans`, `scale` relative"""
    it = _copy(it)
    E = int(it["n_edges"])
    rng = np.random.default_rng(4242 + seed)
    ax = rng.normal(size=(E, 3))
    w = (rot * rng.uniform(0.5, 1.5, E))[:, None] * ax / np.linalg.norm(ax, axis=1, keepdims=True)
    it["zR"][:E] = (rotate(w, np.eye(3)) @ it["zR"][:E].reshape(E, 3, 3)).reshape(E, 9)
    it["zs"][:E] *= 1.0 + scale * rng.normal(size=E)
    it["zt"][:E] += trans * rng.normal(size=(E, 3))
    return it


def group_weights(it):
    """(N, 3): each node's weight per group summed over its usable edges"""
    N, E = int(it["n_nodes"]), int(it["n_edges"])
    use = usable_edges(N, E, it["fixed"], it["ab"], it["zs"], it["zR"], it["zt"], it["zw"])
    out = np.zeros((N, 3))
    for side in (0, 1):
        np.add.at(out, np.asarray(it["ab"])[:E][use, side], it["zw"][:E][use])
    return out


def centre_error(T, truth):
    return float(max(np.linalg.norm(T[i] - truth[i][2]) for i in range(len(truth))))


# ------------------------------------------------------------------------------------------------ on the world
def close_loops(tracks, loops, seq_weight=(1.0, 1.0, 1.0), loop_weight=(1.0, 1.0, 1.0), infos=None, **prm):
    """vslam_world_close_loops restated.  tracks: a list of dict(Twc (F, 16) f64, pose (F, 16) f32, scale (F,), carry (K, 3),
    carry_index (K,), points (cap, 4) f32, size, anchor (cap,) the frame of each point's first observation or -1) -- changed IN PLACE
    --; loops: a list of (track, frame_a, frame_b, use, s, R (9,), t (3,)); infos: a list that takes optimize()'s info of every
    track with a taken loop.  -> [stats (4,) per track], [written (F,) per track]"""
    all_stats, all_written = [], []
    for ti, tr in enumerate(tracks):
        F = len(tr["Twc"])
        Twc = np.asarray(tr["Twc"], np.float64).reshape(F, 4, 4)
        W, C = Twc[:, :3, :3].copy(), Twc[:, :3, 3].copy()
        nodes = [(1.0, W[f], C[f]) for f in range(F)]
        edges, wts = [], []
        for f in range(F - 1):
            edges.append((f, f + 1, (1.0, W[f + 1].T @ W[f], W[f + 1].T @ (C[f] - C[f + 1]))))
            wts.append(seq_weight)
        taken = 0
        for (lt, fa, fb, use, s, R, t) in loops:
            R, t = np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)
            ok = use != 0 and lt == ti and fa != fb and 0 <= fa < F and 0 <= fb < F
            ok = ok and np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all() and s > 0
            if ok and len(edges) < MAX_EDGES:
                edges.append((int(fa), int(fb), (float(s), R.reshape(3, 3), t)))
                wts.append(loop_weight)
                taken += 1
        nan = float("nan")
        if not taken:
            all_stats.append(np.array([0.0, nan, nan, nan]))
            all_written.append(np.zeros(F, bool))
            continue
        it = pack(nodes, edges, [0])
        it["zw"][:] = np.asarray(wts, np.float64)
        s, R, T, stats, info = optimize(*args(it), **prm)
        if infos is not None:
            infos.append(info)
        wr = info["written"]
        all_stats.append(stats)
        all_written.append(wr.copy())
        for f in np.flatnonzero(wr):
            tr["Twc"][f].reshape(4, 4)[:3, :3] = R[f].reshape(3, 3)
            tr["Twc"][f].reshape(4, 4)[:3, 3] = T[f]
            tr["pose"][f] = tr["Twc"][f].astype(np.float32)
            tr["scale"][f] = tr["scale"][f] * s[f]
        if wr[F - 1]:
            v = tr["carry_index"] >= 0
            tr["carry"][v] = tr["carry"][v] * s[F - 1]
        for i in range(int(tr["size"])):
            X = tr["points"][i, :3].astype(np.float64)
            f = int(tr["anchor"][i])
            if not np.isfinite(X).all() or f < 0 or f >= F or not wr[f]:
                continue
            Y = W[f].T @ (X - C[f])
            tr["points"][i, :3] = (s[f] * (R[f].reshape(3, 3) @ Y) + T[f]).astype(np.float32)
    return all_stats, all_written
