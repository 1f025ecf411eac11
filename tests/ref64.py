"""Float64 restatements of the pose and map-association stages, written from the reference sources (not from oracle/),
each returning its value together with the margin it can be trusted to.  They hold oracle/vso_pose.cpp and the device to an
independent definition, where the bit-exact tests only show that those two agree with each other.

  extract_Rt            src/helpers.cpp:3-35
  camera_matrix         src/vslam.cpp:83-85,125        c2 = K * R_t.rowRange(0, 3)
  triangulate           src/helpers.cpp:37-80
  reprojection_filter   src/vslam.cpp:192-251
  associate             src/vslam.cpp:129-161, orb_distance src/PointMap.cpp:36-46, radius_search src/KDTree.cpp:145-171

Every input is taken as the f32 value the stage under test sees and widened to float64; every product, SVD and division
is float64 (np.linalg.svd for the SVDs).  What the f32 stage can differ by is bounded by EPS = 2^-23 times a stated
constant times the conditioning of the step:

  R, t         max-abs   C_RT * EPS * (1 + s1 / (s2 - s3))    s = singular values of E = K^T F K.  s2 - s3 is the gap that
                                                              separates U[:,2] (the translation) from the other columns and
                                                              the W-rotated pair from the third; for a true essential matrix
                                                              s3 ~ 0 and this is s1 / s2.
  camera matrix elementwise  C_C2 * EPS * sum_k |K_ik| |Rt_kj|
  X            unit-vector distance of (X, 1) / |(X, 1)|  C_X * EPS * (1 + s1 / (s3 - s4))   s = singular values of the
                                                              4 x 4 DLT system; for exact projections s4 ~ 0 and this is s1/s3.
  reprojected point / projected map point  per coordinate  C_PROJ * EPS * |value| (one rounding of a double dot product
                                                              and one f32 division), plus the double sum's own rounding.

RANSAC (src/RansacFilter.cpp:36-140) is held the same way, the integer parts by tests/ref_int.py:

  fundamental_8pt       src/RansacFilter.cpp:69-103
  residuals             src/RansacFilter.cpp:105-140
  hold_ransac           the two above plus the accept rule of :44-66, on one pair's device (or oracle) outputs

  F            Frobenius, either sign   C_F * EPS * (1 + kappa) + the float64 solve's own error.  kappa combines the
                                        conditioning of the null vector, taken on the column-scaled 8 x 9 system
                                        (|D v|_1 / s8: see fundamental_8pt), with the gap of the 3 x 3 rank-2 step.
                                        Decided when the bound is below F_LIMIT = 1e-2: F has unit norm up to the dropped
                                        singular value, so that separates F from its transpose, a permuted row or a wrong
                                        rank-2 step.
  residual e   absolute                 carried through F x1, F^T x2, n, the quotient n^2 / a0^2 and the three squares:
                                        C_DOT * EPS * (absolute-value sum) per dot product, C_OPS * EPS * (value) per
                                        quotient / square / sum.
Calibration (the oracle and the device are bit-identical, so a ratio seen on one is the other's).  Largest error / bound:
                                         8-point solve (C_F = 8)   residual sum (C_DOT = 3, C_OPS = 4)
  14 regular pairs of tests/test_oracle_ransac_ref.py     0.118                 0.128     asserted there: <= 1/4, > 0.001
  its degenerate pairs (coordinates x 1e-9 among them)    0.024                 0.124     printed; <= 1 asserted by the hold
  the other inputs of tests/test_gpu_ransac.py            0.140                 0.139
  fixed fuzz slice (tests/test_gpu_fuzz.py, 400 cases)    0.163                 0.143
  soak and hard regime, every fourth pair (test_gpu_soak) 0.104                 0.154
so the margin that governs is 6.1x for C_F and 6.5x for the residual constants (4x is the least allowed).  On the regular
pairs 86 .. 100 % of a pair's solves are decided (noisy integer points 96 .. 100 %, exact sub-pixel points 86 .. 91 %; 78 % of
all solves have a bound below 1e-3, where F is told from its transpose one solve at a time), 0 .. 0.07 % of a pair's
evaluations are undecided, and no decided evaluation of any hypothesis disagrees with the oracle's mask.
A decision (trace sign, t_z sign, re <= thresholdSq, 0 <= x < W, d^2 < r^2) is *decided* when the quantity lies further
from its boundary than the error bound carried to it; only decided outcomes are asserted.  The constants were calibrated
once (tests/test_oracle_pose.py, tests/test_oracle_assoc.py report the largest observed error / bound ratio) and carry a
margin of at least 4x over what the oracle and the device reach.
"""
import numpy as np

EPS = 2.0 ** -23
C_RT = 8.0
C_C2 = 4.0
C_X = 4.0
C_PROJ = 4.0

_W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])   # src/helpers.cpp:13-16


def _f64(a, shape=None):
    a = np.asarray(a, np.float32).astype(np.float64)
    return a.reshape(shape) if shape is not None else a


# ------------------------------------------------------------------------------------------------------- extract_Rt
def extract_Rt(F, K):
    """src/helpers.cpp:3-35.  Returns a dict:
      R1, R2        the two candidates U W V^T and U W^T V^T, each negated when its determinant is negative (:18-26);
      R             R2 if trace(R1) < 0 else R1 under numpy's labelling (:29);
      t             U[:,2] / |U[:,2]|, negated when t_z < 0 (:9-11, :31-33);
      s             singular values of E; cond = s1 / (s2 - s3); tol = C_RT * EPS * (1 + cond), max-abs on R and t;
      t_separated   s2 - s3 separates U[:,2] from the other columns well enough that tol < 1e-2, and E has no exactly
                    zero row (see below);
      t_sign        |t_z| > tol: the sign rule of :31 is decided, otherwise t is defined up to sign;
      rot_decided   exactly one candidate has trace >= 0, both traces are further than 3 tol from 0 and t_separated.  The
                    SVD's sign freedom swaps the labels R1 / R2, so only then is the choice of :29 independent of it;
      R_expected    the candidate with trace >= 0 when rot_decided, else None."""
    Fd, Kd = _f64(F, (3, 3)), _f64(K, (3, 3))
    E = Kd.T @ Fd @ Kd                                  # :4
    U, s, Vt = np.linalg.svd(E)                         # :7
    nu = np.linalg.norm(U[:, 2])
    t = U[:, 2] / nu                                    # :9-11
    if t[2] < 0:                                        # :31-33
        t = -t
    R1 = U @ _W @ Vt                                    # :18
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = U @ _W.T @ Vt                                  # :23
    if np.linalg.det(R2) < 0:
        R2 = -R2
    tr1, tr2 = np.trace(R1), np.trace(R2)
    R = R2 if tr1 < 0 else R1                           # :29
    gap = s[1] - s[2]
    cond = s[0] / gap if gap > 0 else np.inf
    tol = C_RT * EPS * (1.0 + cond)
    # An exactly zero row of E keeps every f32 Jacobi rotation inside a coordinate plane: the third column the reference's
    # SVD returns is then the normalised residue of the rotations, not a null vector (its random fill is only for a norm
    # below FLT_MIN), so U[:,2] is not defined by E to any accuracy there.
    zero_row = bool((E == 0).all(axis=1).any())
    t_separated = bool(tol < 1e-2 and not zero_row)
    t_sign = bool(t_separated and abs(t[2]) > tol)
    rot_decided = bool(t_separated and ((tr1 >= 0) != (tr2 >= 0)) and min(abs(tr1), abs(tr2)) > 3 * tol)
    R_expected = (R1 if tr1 >= 0 else R2) if rot_decided else None
    return dict(R1=R1, R2=R2, R=R, t=t, s=s, cond=cond, tol=tol, t_separated=t_separated, t_sign=t_sign,
                rot_decided=rot_decided, R_expected=R_expected, traces=(tr1, tr2))


def rt_errors(ref, R, t):
    """(R error, t error) of an f32 result against extract_Rt's dict, max-abs; the R error is None when the rotation is not
    decided and t is compared up to sign when its sign is not decided (None when t is not separated)."""
    R = _f64(R, (3, 3)); t = _f64(t, (3,))
    er = float(np.abs(R - ref["R_expected"]).max()) if ref["rot_decided"] else None
    if not ref["t_separated"]:
        return er, None
    et = float(np.abs(t - ref["t"]).max())
    if not ref["t_sign"]:
        et = min(et, float(np.abs(t + ref["t"]).max()))
    return er, et


# --------------------------------------------------------------------------------------------------- camera matrix
def camera_matrix(K, R, t):
    """c2 = K * [R | t] (src/vslam.cpp:83-85,125), with the elementwise bound C_C2 * EPS * (|K| |[R|t]|)."""
    Kd = _f64(K, (3, 3))
    Rt = np.c_[_f64(R, (3, 3)), _f64(t, (3,))]
    return Kd @ Rt, C_C2 * EPS * (np.abs(Kd) @ np.abs(Rt))


# ----------------------------------------------------------------------------------------------------- triangulate
def triangulate(p1, p2, c1, c2):
    """src/helpers.cpp:37-80: per point the 4 x 4 system of :49-52, its SVD (:59), X = V_t.row(3) / V_t(3,3) (:72-75).
    Returns a dict: X (n, 3); v (n, 4) the unit null vector, sign chosen so v[3] >= 0; s (n, 4) singular values;
    cond = s1 / (s3 - s4); tol = C_X * EPS * (1 + cond) on the unit vector (X, 1) / |(X, 1)|; at_inf where |v[3]| <= 4 tol
    (a point at infinity: X is not defined to any accuracy, only v is)."""
    p1 = _f64(p1).reshape(-1, 2); p2 = _f64(p2).reshape(-1, 2)
    c1 = _f64(c1, (3, 4)); c2 = _f64(c2, (3, 4))
    n = len(p1)
    A = np.empty((n, 4, 4))
    A[:, 0] = p1[:, :1] * c1[2] - c1[0]
    A[:, 1] = p1[:, 1:] * c1[2] - c1[1]
    A[:, 2] = p2[:, :1] * c2[2] - c2[0]
    A[:, 3] = p2[:, 1:] * c2[2] - c2[1]
    if n == 0:
        z = np.zeros((0,))
        return dict(X=np.zeros((0, 3)), v=np.zeros((0, 4)), s=np.zeros((0, 4)), cond=z, tol=z, at_inf=z.astype(bool))
    _, s, Vt = np.linalg.svd(A)
    v = Vt[:, 3, :]
    v = v * np.where(v[:, 3:] < 0, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        X = v[:, :3] / v[:, 3:]
        gap = s[:, 2] - s[:, 3]
        cond = np.where(gap > 0, s[:, 0] / gap, np.inf)
    tol = C_X * EPS * (1.0 + cond)
    return dict(X=X, v=v, s=s, cond=cond, tol=tol, at_inf=np.abs(v[:, 3]) <= 4 * tol)


def homogeneous_error(X4, ref):
    """Distance of the f32 points (n, 4) (x, y, z, 1) from ref's unit null vectors, as unit vectors, either sign."""
    h = _f64(X4).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        u = h / np.linalg.norm(h, axis=1, keepdims=True)
        e = np.minimum(np.linalg.norm(u - ref["v"], axis=1), np.linalg.norm(u + ref["v"], axis=1))
    return np.where(np.isfinite(e), e, np.inf)


# --------------------------------------------------------------------------------------------- reprojection filter
def reprojection_filter(points_4d, p1, p2, c1, c2, map_point_ids, threshold_sq):
    """src/vslam.cpp:192-251, with its quirks restated from the source:
      * reproj = points_4d * c.t() (:193-194); the de-homogenise loop runs `for (i = 0; i < rows; i += 3)` over the FLAT
        N x 3 data (:201-211), so only flat indices 0, 3, 6, ... < N -- rows 0 .. ceil(N/3) - 1 -- are divided by h;
      * d = reproj(:, 0:2) - initial_points (:228-229); re = d.row(i).dot(d.row(i));
      * a match is skipped when map_point_ids[i] > 0, indexed by the MATCH index i (:240);
      * kept when re1 <= thresholdSq and re2 <= thresholdSq (:242-245); reproj_error += re1 + re2 (:249).
    Returns a dict: kept (ascending match indices), err (the sum), re1 / re2, divided (the rows the loop divides), tol1 /
    tol2 (bounds on re), slack = the smallest |re - thresholdSq| / tol over the decisions the filter takes (inf if none),
    err_tol = the bound on err."""
    P = _f64(points_4d).reshape(-1, 4)
    q1 = _f64(p1).reshape(-1, 2); q2 = _f64(p2).reshape(-1, 2)
    n = len(P)
    ids = np.asarray(map_point_ids).reshape(-1)[:n]
    thr = float(np.float32(threshold_sq))
    out = {}
    res = []
    divided = np.arange(n) * 3 < n                     # flat index 3k < N  <=>  row k is divided
    for q, c in ((q1, _f64(c1, (3, 4))), (q2, _f64(c2, (3, 4)))):
        terms = P[:, None, :] * c[None, :, :]          # (n, 3, 4)
        r = terms.sum(2)
        mag = np.abs(terms).sum(2)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r[divided, :2] /= r[divided, 2:3]
            # f32 rounding of the dot product, of the division and of the subtraction, plus the double sum's own rounding
            ex = C_PROJ * EPS * (np.abs(r[:, :2]) + np.abs(q)) + 2.0 ** -50 * mag[:, :2] / np.where(divided, np.abs(r[:, 2]), 1.0)[:, None]
            d = r[:, :2] - q
            re = (d * d).sum(1)
            e = np.sqrt((ex * ex).sum(1))
            tol = 2 * np.sqrt(re) * e + e * e + C_PROJ * EPS * re
        res.append((re, tol))
    (re1, tol1), (re2, tol2) = res
    skip = ids > 0                                     # :240
    with np.errstate(invalid="ignore"):
        ok1 = re1 <= thr
        ok2 = re2 <= thr
    kept = np.nonzero(~skip & ok1 & ok2)[0]
    err = float(np.sum(re1[kept] + re2[kept]))
    with np.errstate(invalid="ignore", divide="ignore"):
        s1 = np.abs(re1 - thr) / tol1
        s2 = np.abs(re2 - thr) / tol2
    s1 = np.where(np.isfinite(re1), s1, 0.0)          # a NaN / inf distance is never trusted to decide anything
    s2 = np.where(np.isfinite(re2), s2, 0.0)
    # the decision at i: skipped; or re1 decides it (rejected with a margin); or re1 passes with a margin and re2 decides
    first_rejects = ~ok1 & (s1 > 1)
    per = np.where(skip, np.inf, np.where(first_rejects, s1, np.minimum(s1, s2)))
    slack = float(per.min()) if n else np.inf
    err_tol = float(np.sum(tol1[kept] + tol2[kept] + EPS * (re1[kept] + re2[kept])))
    out.update(kept=kept, err=err, re1=re1, re2=re2, tol1=tol1, tol2=tol2, divided=divided, slack=slack, per=per,
               err_tol=err_tol)
    return out


# ------------------------------------------------------------------------------------------------- map association
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint32)


def orb_distance(kp_desc_row, obs):
    """src/PointMap.cpp:36-46: the minimum Hamming distance to the map point's stored observations; u32_max without any."""
    if len(obs) == 0:
        return 0xFFFFFFFF
    return int(_POP[np.bitwise_xor(obs, kp_desc_row[None, :])].sum(1).min())


def radius_search(nodes, xy, q, radius):
    """src/KDTree.cpp:145-171 on the given pre-order node array (node, then its len/2-node left subtree, then the right one),
    float64: visit order node, left, right; both children when |split| <= r, else the side of the query; a hit when
    d^2 < r^2.  Returns the hit indices in visit order."""
    n = len(nodes)
    r = float(radius); rsq = r * r
    hits = []
    stack = [(0, n, 0)] if n > 0 else []
    while stack:
        pos, ln, axis = stack.pop()
        idx = int(nodes[pos])
        px, py = xy[idx]
        split = (q[0] - px) if axis == 0 else (q[1] - py)
        nl = ln // 2
        nr = ln - nl - 1
        left = (pos + 1, nl, 1 - axis) if nl > 0 else None
        right = (pos + 1 + nl, nr, 1 - axis) if nr > 0 else None
        if abs(split) <= r:
            dx, dy = q[0] - px, q[1] - py
            if dx * dx + dy * dy < rsq:
                hits.append(idx)
            nxt = [left, right]
        elif split < 0:
            nxt = [left]
        else:
            nxt = [right]
        for c in reversed(nxt):                        # left is visited first
            if c is not None:
                stack.append(c)
    return hits


def associate(map_points, c2, img_w, img_h, nodes, kp_xy, kp_desc, obs_offsets, obs_desc, map_point_ids, radius=2.0,
              dist_threshold=64):
    """src/vslam.cpp:129-161: project every map point with c2 in float64 and de-homogenise (:136-140; h's sign is not
    tested); in view when 0 <= x < W and 0 <= y < H (:141); radius_search in the frame's tree (:149); the first hit with
    map_point_ids[idx] < 0 (:151) and orb_distance < dist_threshold (:153) is claimed (:154-157), map point by map point in
    order.  No cap on the number of hits.  Returns a dict: ids (updated copy), claim (keypoint or -1 per map point), q (the
    projections), in_view, hits (per map point, visit order; None out of view), slack = the smallest |distance to a
    boundary| / bound over every in-view and radius decision (inf if there is none)."""
    P = _f64(map_points).reshape(-1, 4)
    C = _f64(c2, (3, 4))
    xy = _f64(kp_xy).reshape(-1, 2)
    desc = np.asarray(kp_desc, np.uint8).reshape(-1, 32)
    od = np.asarray(obs_desc, np.uint8).reshape(-1, 32)
    offs = np.asarray(obs_offsets).reshape(-1)
    ids = np.asarray(map_point_ids, np.int32).reshape(-1).copy()
    m = len(P)
    r = float(np.float32(radius))
    rsq = r * r
    terms = P[:, None, :] * C[None, :, :]
    pr = terms.sum(2)
    mag = np.abs(terms).sum(2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = pr[:, :2] / pr[:, 2:3]
        eq = C_PROJ * EPS * np.abs(q) + 2.0 ** -50 * mag[:, :2] / np.abs(pr[:, 2:3])
        in_view = (q[:, 0] >= 0) & (q[:, 0] < img_w) & (q[:, 1] >= 0) & (q[:, 1] < img_h)
        # the smallest distance to a boundary of a coordinate that decides: a coordinate far outside decides alone
        sx = np.minimum(np.abs(q[:, 0]), np.abs(img_w - q[:, 0])) / eq[:, 0]
        sy = np.minimum(np.abs(q[:, 1]), np.abs(img_h - q[:, 1])) / eq[:, 1]
    fin = np.isfinite(q).all(1) & np.isfinite(eq).all(1)
    # out of view by a decided coordinate, or in view with both decided; a non-finite projection is out in f32 as well
    # only if it is non-finite there too, which holds when h is exactly 0 (the f32 rounding of 0 is 0)
    out_x = ~((q[:, 0] >= 0) & (q[:, 0] < img_w))
    out_y = ~((q[:, 1] >= 0) & (q[:, 1] < img_h))
    view_slack = np.where(in_view, np.minimum(sx, sy),
                          np.maximum(np.where(out_x, sx, 0), np.where(out_y, sy, 0)))
    view_slack = np.where(fin, view_slack, np.where(pr[:, 2] == 0, np.inf, 0.0))
    slack = float(view_slack.min()) if m else np.inf
    claim = np.full(m, -1, np.int32)
    hits_all = [None] * m
    for i in range(m):
        if not in_view[i]:
            continue
        qi = q[i]
        d = xy - qi[None, :]
        d2 = (d * d).sum(1)
        # f32 d^2 from the f32 projection: the coordinate error carried through, plus the f32 rounding of d and d^2
        e = np.sqrt((eq[i] ** 2).sum()) + EPS * np.abs(d).sum(1)
        tol = 2 * np.sqrt(d2) * e + e * e + 4 * EPS * (d2 + rsq)
        if len(d2):
            slack = min(slack, float((np.abs(d2 - rsq) / tol).min()))
        hits = radius_search(nodes, xy, qi, r)
        hits_all[i] = hits
        for idx in hits:
            if ids[idx] >= 0:                          # :151
                continue
            if orb_distance(desc[idx], od[offs[i]:offs[i + 1]]) < dist_threshold:   # :152-153
                ids[idx] = i
                claim[i] = idx
                break                                  # :157
    return dict(ids=ids, claim=claim, q=q, in_view=in_view, hits=hits_all, slack=slack)


def acceptable_hits(res, i, kp_desc, obs_offsets, obs_desc, dist_threshold=64):
    """The number of radius hits of map point i whose orb_distance is under the threshold (whatever their ids): what the
    device keeps per map point (include/vslam_amd.h, vslam_associate_map_points: at most 16)."""
    if res["hits"][i] is None:
        return 0
    od = np.asarray(obs_desc, np.uint8).reshape(-1, 32)
    desc = np.asarray(kp_desc, np.uint8).reshape(-1, 32)
    o0, o1 = int(obs_offsets[i]), int(obs_offsets[i + 1])
    return sum(orb_distance(desc[k], od[o0:o1]) < dist_threshold for k in res["hits"][i])


# ----------------------------------------------------------------------------------- holding device outputs to these
def hold_pose(F, K, R, t, c2, p1=None, p2=None, pts=None, ids=None, kept=None, err=None, threshold_sq=4.0):
    """Hold one pair's pose outputs (what extract_Rt, the camera matrix, triangulate with c1 = [K | 0] and the reprojection
    filter returned for it) to the references above, each stage given the inputs it actually received.  Asserts every
    decided outcome; returns counts: rt (0/1 decided), points / points_undecided, filter / filter_undecided, and the largest
    error / bound ratio seen."""
    st = dict(rt=0, points=0, points_undecided=0, filter=0, filter_undecided=0, worst=0.0)
    rt = extract_Rt(F, K)
    er, et = rt_errors(rt, R, t)
    for e in (er, et):
        if e is not None:
            assert e <= rt["tol"], ("extract_Rt", e, rt["tol"])
            st["worst"] = max(st["worst"], e / rt["tol"])
    st["rt"] = int(er is not None and et is not None)
    c2r, c2tol = camera_matrix(K, R, t)
    d = np.abs(_f64(c2, (3, 4)) - c2r)
    ratio = np.where(c2tol > 0, d / np.where(c2tol > 0, c2tol, 1.0), np.where(d > 0, np.inf, 0.0))
    assert (ratio <= 1).all(), ("camera matrix", float(ratio.max()))
    st["worst"] = max(st["worst"], float(ratio.max()))
    if pts is None:
        return st
    c1 = np.c_[_f64(K, (3, 3)), np.zeros(3)]
    tri = triangulate(p1, p2, c1, c2)
    e = homogeneous_error(np.asarray(pts).reshape(-1, 4), tri)
    ok = ~tri["at_inf"] & (tri["tol"] < 1e-2)
    assert (e[ok] <= tri["tol"][ok]).all(), ("triangulate", float((e[ok] / tri["tol"][ok]).max()))
    if ok.any():
        st["worst"] = max(st["worst"], float((e[ok] / tri["tol"][ok]).max()))
    st["points"], st["points_undecided"] = int(ok.sum()), int((~ok).sum())
    if kept is None:
        return st
    fr = reprojection_filter(pts, p1, p2, c1, c2, ids, threshold_sq)
    dec = fr["per"] > 1
    n = len(fr["per"])
    got = np.zeros(n, bool); got[np.asarray(kept, np.int64)] = True
    want = np.zeros(n, bool); want[fr["kept"]] = True
    assert np.array_equal(got[dec], want[dec]), ("reprojection filter", np.nonzero(got != want)[0][:10])
    if dec.all():
        assert abs(float(err) - fr["err"]) <= fr["err_tol"], ("reprojection error sum", float(err), fr["err"], fr["err_tol"])
    st["filter"], st["filter_undecided"] = int(dec.sum()), int((~dec).sum())
    return st


def hold_association(map_points, c2, img_w, img_h, nodes, kp_xy, kp_desc, obs_offsets, obs_desc, ids_in, ids_out, claim,
                     radius=2.0, dist_threshold=64):
    """Hold one item's association outputs (claims and updated map_point_ids) to associate(); the claims are chained, so a
    scene is held only when it has no borderline decision.  Returns True when held, False when undecided."""
    r = associate(map_points, c2, img_w, img_h, nodes, kp_xy, kp_desc, obs_offsets, obs_desc, ids_in, radius, dist_threshold)
    if not r["slack"] > 1:
        return False
    assert np.array_equal(np.asarray(claim), r["claim"]), ("claims", np.nonzero(np.asarray(claim) != r["claim"])[0][:10])
    assert np.array_equal(np.asarray(ids_out), r["ids"]), "map_point_ids"
    return True


# =============================================================================================== RANSAC (RansacFilter.cpp)
# See the module docstring's RANSAC section for the bounds and their calibration.
C_F = 8.0             # 8-point solve: Frobenius bound C_F * EPS * (1 + kappa)
F_LIMIT = 1e-2        # a solve is decided when its bound is below this
F_TIGHT = 1e-3        # ... and can tell F from its transpose when below this (reported, see fundamental_check)
C_DOT = 3.0           # residual: one f32 dot product of three terms, times its absolute-value sum
C_OPS = 4.0           # residual: the quotient, a square, the four-term sum, each times its value
_TINY = 2.0 ** -126   # smallest normal f32: below it a product has lost relative accuracy
_HUGE = 2.0 ** 120    # above it a square overflows f32


def fundamental_8pt(p1_set, p2_set):
    """src/RansacFilter.cpp:69-103 for a batch of samples p1_set, p2_set (H, 8, 2): the 8 x 9 system of :81-89 with its
    entries rounded to f32 as the reference stores them, its SVD (:94), F0 = V_t.row(8) (:95), the 3 x 3 SVD (:98), the third
    singular value set to 0 (:99), F = U diag(D) V_t (:101).  Returns a dict:
      F (H, 3, 3); s9 (H, 8) and s3 (H, 3) the singular values of both steps; sc (H, 8) those of the column-scaled system;
      kappa = (1 + |D v|_1 / s9_8) * (1 + 2 * s3_3 / (s3_2 - s3_3)) - 1: the null vector v taken on the column-scaled
              system (D = the column norms of A; see the comment in the code), then the gap of the 3 x 3 step that separates
              the dropped singular direction from the kept ones;
      tol = C_F * EPS * (1 + kappa) + this reference's own float64 error, Frobenius, on min(|F - F'|, |F + F'|) (the sign of
            a null vector is free);
      decided = tol < F_LIMIT.  A zero column, a repeated or collinear sample, any rank below 8 give kappa = inf."""
    p1 = _f64(p1_set).reshape(-1, 8, 2); p2 = _f64(p2_set).reshape(-1, 8, 2)
    H = len(p1)
    if H == 0:
        z = np.zeros(0)
        return dict(F=np.zeros((0, 3, 3)), s9=np.zeros((0, 8)), s3=np.zeros((0, 3)), sc=np.zeros((0, 8)), kappa=z, tol=z,
                    decided=z.astype(bool))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    one = np.ones_like(u1)
    with np.errstate(all="ignore"):
        A = np.stack([f32(u2 * u1), f32(u2 * v1), u2, f32(v2 * u1), f32(v2 * v1), v2, u1, v1, one], axis=2)   # :81-89
        finite = np.isfinite(A).all(axis=(1, 2))
        A = np.where(finite[:, None, None], A, 0.0)
        # :94-95.  The null vector is taken through the column-scaled system A = B D, D = diag(column norms): LAPACK's error is
        # 2^-52 times the condition of the matrix it is given, and B's is thousands of times smaller than A's (pixel
        # coordinates: columns of 1e6 beside a column of ones).  B w = 0  <=>  A (D^-1 w) = 0.
        s9 = np.linalg.svd(A, compute_uv=False)
        d = np.linalg.norm(A, axis=1)                                 # (H, 9) column norms
        s8 = s9[:, 7] - 2.0 ** -48 * s9[:, 0]        # LAPACK knows s8 to 2^-52 s1 only: the lower end of what it can be
        ok = finite & (d > 0).all(1) & (s8 > 0)
        dinv = 1.0 / np.where(d > 0, d, 1.0)
        _, sc, Wt9 = np.linalg.svd(A * dinv[:, None, :])              # FULL_UV
        v = Wt9[:, 8, :] * dinv
        nv = np.linalg.norm(v, axis=1)
        v = v / nv[:, None]
        F0 = v.reshape(H, 3, 3)
        U, s3, Wt = np.linalg.svd(F0)                                 # :98
        F = (U[:, :, :2] * s3[:, None, :2]) @ Wt[:, :2, :]            # :99-101
        # What an f32 solve can differ by: a rotation of two rows perturbs every entry relative to its own column, dA = E D
        # with |E| ~ EPS, so to first order |dv| = |A^+ E D v| <= |E| |D v|_1 / s8(A): the 1-norm of the SCALED null vector
        # over the smallest singular value.
        w1 = np.abs(v * d).sum(1)                                     # |D v|_1
        k_null = np.where(ok, w1 / np.where(s8 > 0, s8, 1.0), np.inf)
        k_null = np.where(sc[:, 7] > 64 * EPS * sc[:, 0], k_null, np.inf)      # rank below 8 to working precision
        # and this reference's own error: 2^-52 cond(B), carried back through D^-1 (largest 1 / d over |D^-1 w|)
        own = 16 * 2.0 ** -52 * (dinv.max(1) / nv) * sc[:, 0] / np.where(sc[:, 7] > 0, sc[:, 7], 1.0)
        gap = s3[:, 1] - s3[:, 2]
        k_3 = np.where(gap > 0, s3[:, 2] / np.where(gap > 0, gap, 1.0), np.inf)
        kappa = (1.0 + k_null) * (1.0 + 2.0 * k_3) - 1.0
        tol = C_F * EPS * (1.0 + kappa) + own * (1.0 + 2.0 * k_3)
    tol = np.where(np.isfinite(tol), tol, np.inf)
    return dict(F=F, s9=s9, s3=s3, sc=sc, kappa=kappa, tol=tol, decided=tol < F_LIMIT)


def fundamental_error(F_dev, ref):
    """min(|F - F_dev|, |F + F_dev|), Frobenius, per hypothesis; inf where F_dev is not finite."""
    Fd = _f64(F_dev).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.minimum(np.linalg.norm((Fd - ref["F"]).reshape(-1, 9), axis=1), np.linalg.norm((Fd + ref["F"]).reshape(-1, 9), axis=1))
    return np.where(np.isfinite(e), e, np.inf)


def fundamental_check(xy1, xy2, pairs, sets, hypF):
    """Assert every decided solve of one pair: hypF (H, 9) within its bound of fundamental_8pt on the sampled matches.
    Returns (decided, undecided, worst error / bound ratio, tight) -- tight = the decided solves whose bound is below
    F_TIGHT = 1e-3: with pixel coordinates |F - F^T| is about 1e-3 of |F|, so these are the solves that can tell F from its
    transpose one by one (the others still tell a wrong rank-2 step or a permuted row, which change F by O(1))."""
    pairs = np.asarray(pairs).reshape(-1, 2); sets = np.asarray(sets).reshape(-1, 8)
    ref = fundamental_8pt(np.asarray(xy1, np.float32).reshape(-1, 2)[pairs[sets, 0]],
                          np.asarray(xy2, np.float32).reshape(-1, 2)[pairs[sets, 1]])
    hypF = np.asarray(hypF, np.float32).reshape(len(sets), 9)
    err = fundamental_error(hypF, ref)
    dec = ref["decided"]
    if not dec.any():
        return 0, int(len(sets)), 0.0, 0
    ratio = err[dec] / ref["tol"][dec]
    h = int(np.nonzero(dec)[0][ratio.argmax()])
    assert ratio.max() <= 1.0, ("8-point solve", h, float(err[h]), float(ref["tol"][h]), hypF[h], ref["F"][h].reshape(9))
    return int(dec.sum()), int((~dec).sum()), float(ratio.max()), int((ref["tol"] < F_TIGHT).sum())


def residuals(F, p1, p2, pairs, thr, chunk=1 << 21, keep=None):
    """src/RansacFilter.cpp:105-140 in float64 from the f32 inputs, for a batch of hypotheses F (H, 9) over the matches
    pairs (N, 2) into p1, p2:  a = F x1, c = F^T x2 (:119-120), n = x2 . a (:122-123),
        e = n^2 / a0^2 + a1^2 + c0^2 + c1^2      exactly as the operators of :126 bind (NOT Sampson's n^2 / (a0^2 + ...)),
    inlier when e <= thr (:130), sum over all matches (:138).  Per evaluation the error an f32 evaluation can have is carried
    to first order: da_i = C_DOT EPS (|F_i0 x| + |F_i1 y| + |F_i2|), likewise dc_i; dn = |x2| da0 + |y2| da1 + da2 +
    C_DOT EPS (|x2 a0| + |y2 a1| + |a2|); the quotient between (|n| -+ dn)^2 / (|a0| +- da0)^2 plus C_OPS EPS of itself; every
    square 2 |v| dv + dv^2 + C_OPS EPS v^2; the sum C_OPS EPS e.  An evaluation is `valid` when that bound means something:
    everything finite, da0 <= |a0| / 16, a0^2 a normal f32 and no square near the f32 overflow; it is `decided` when valid
    and |e - thr| > tol.  Returns a dict, per hypothesis: lo (decided inliers), hi (lo + undecided), n_undecided, sum and
    sum_tol (float64 sum and its bound; sum_ok where every evaluation is valid, else the two are nan / inf), worst_valid;
    with keep = a list of hypothesis indices also e / tol / decided / inlier (len(keep), N) for those."""
    F = _f64(F).reshape(-1, 9)
    H = len(F)
    pairs = np.asarray(pairs).reshape(-1, 2)
    N = len(pairs)
    q1 = _f64(p1).reshape(-1, 2)[pairs[:, 0]]; q2 = _f64(p2).reshape(-1, 2)[pairs[:, 1]]
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    ax1, ay1, ax2, ay2 = np.abs(x1), np.abs(y1), np.abs(x2), np.abs(y2)
    thr = float(np.float32(thr))
    lo = np.zeros(H, np.int64); und = np.zeros(H, np.int64)
    tot = np.zeros(H); tot_tol = np.zeros(H); sum_ok = np.zeros(H, bool)
    kept = {}
    step = max(1, chunk // max(N, 1))
    for h0 in range(0, H, step):
        f = F[h0:h0 + step, :, None]                                  # (h, 9, 1)
        af = np.abs(f)
        with np.errstate(all="ignore"):
            a0 = f[:, 0] * x1 + f[:, 1] * y1 + f[:, 2]                # :119
            a1 = f[:, 3] * x1 + f[:, 4] * y1 + f[:, 5]
            a2 = f[:, 6] * x1 + f[:, 7] * y1 + f[:, 8]
            c0 = f[:, 0] * x2 + f[:, 3] * y2 + f[:, 6]                # :120, F.t()
            c1 = f[:, 1] * x2 + f[:, 4] * y2 + f[:, 7]
            da0 = C_DOT * EPS * (af[:, 0] * ax1 + af[:, 1] * ay1 + af[:, 2])
            da1 = C_DOT * EPS * (af[:, 3] * ax1 + af[:, 4] * ay1 + af[:, 5])
            da2 = C_DOT * EPS * (af[:, 6] * ax1 + af[:, 7] * ay1 + af[:, 8])
            dc0 = C_DOT * EPS * (af[:, 0] * ax2 + af[:, 3] * ay2 + af[:, 6])
            dc1 = C_DOT * EPS * (af[:, 1] * ax2 + af[:, 4] * ay2 + af[:, 7])
            n = x2 * a0 + y2 * a1 + a2                                # :122-123
            dn = ax2 * da0 + ay2 * da1 + da2 + C_DOT * EPS * (np.abs(x2 * a0) + np.abs(y2 * a1) + np.abs(a2))
            aa0, an = np.abs(a0), np.abs(n)
            q = n * n / (a0 * a0)                                     # :126, first term
            den_lo = np.maximum(aa0 - da0, 0.0) ** 2
            q_hi = ((an + dn) ** 2 + _TINY) / den_lo
            q_lo = np.maximum(an - dn, 0.0) ** 2 / (aa0 + da0) ** 2
            dq = np.maximum(q_hi - q, q - q_lo) + C_OPS * EPS * q_hi
            sq = a1 * a1 + c0 * c0 + c1 * c1
            dsq = (2 * np.abs(a1) * da1 + da1 * da1 + 2 * np.abs(c0) * dc0 + dc0 * dc0 + 2 * np.abs(c1) * dc1 + dc1 * dc1 +
                   C_OPS * EPS * sq + 3 * _TINY)
            e = q + sq
            tol = dq + dsq + C_OPS * EPS * (q_hi + sq)
            valid = (np.isfinite(e) & np.isfinite(tol) & (16 * da0 <= aa0) & (den_lo >= _TINY) &
                     ((an + dn) < 2.0 ** 60) & (q_hi + sq + tol < _HUGE))
            decided = valid & (np.abs(e - thr) > tol)
            inl = e <= thr
        lo[h0:h0 + step] = (decided & inl).sum(1)
        und[h0:h0 + step] = (~decided).sum(1)
        allv = valid.all(1)
        sum_ok[h0:h0 + step] = allv
        with np.errstate(all="ignore"):
            s = np.where(valid, e, 0.0).sum(1)
            tot[h0:h0 + step] = np.where(allv, s, np.nan)
            # cv::sum accumulates in double (:138) and is rounded to float once
            tot_tol[h0:h0 + step] = np.where(allv, np.where(valid, tol, 0.0).sum(1) + EPS * np.abs(s), np.inf)
        if keep is not None:
            for k in keep:
                if h0 <= k < h0 + step:
                    kept[k] = (e[k - h0], tol[k - h0], decided[k - h0], inl[k - h0])
    out = dict(lo=lo, hi=lo + und, n_undecided=und, sum=tot, sum_tol=tot_tol, sum_ok=sum_ok, n=N)
    if keep is not None:
        for i, name in enumerate(("e", "tol", "decided", "inlier")):
            out[name] = np.stack([kept[k][i] for k in keep]) if len(keep) else np.zeros((0, N))
    return out


def new_ransac_stats():
    return dict(solves=0, solves_undecided=0, solves_tight=0, evals=0, evals_undecided=0, pairs=0, pairs_undecided=0, worst_F=0.0,
                worst_sum=0.0)


def add_ransac_stats(total, st):
    for k, v in st.items():
        total[k] = max(total.get(k, 0.0), v) if k.startswith("worst") else total.get(k, 0) + v
    return total


def ransac_shares(st):
    """One line for a test to print: the held / undecided shares and the worst error / bound ratios."""
    pc = lambda a, b: 100.0 * a / max(a + b, 1)
    return ("solves held %d (%.1f %%; bound < 1e-3: %d), evaluations undecided %d of %d (%.4f %%), winner checks held %d undecided %d, "
            "worst ratio F %.4f sum %.4f" % (st["solves"], pc(st["solves"], st["solves_undecided"]), st["solves_tight"], st["evals_undecided"],
                                             st["evals"] + st["evals_undecided"],
                                             100.0 - pc(st["evals"], st["evals_undecided"]), st["pairs"],
                                             st["pairs_undecided"], st["worst_F"], st["worst_sum"]))


def hold_ransac(xy1, xy2, pairs, sets, thr, out, mode="all", solve=True):
    """Hold one pair's RANSAC outputs to fundamental_8pt, residuals and the accept rule of src/RansacFilter.cpp:44-66.
    pairs (n, 2) are the preliminary matches, sets (H, 8) the sample sets, out the outputs for this pair: hypF (H, 9),
    hyp_count (H), hyp_sum (H), best (4: winner, count, sum bits, kept), F (9), mask (>= n), matches (>= kept, 2).  mode "all":
    every hypothesis carries its count and sum; "ties" (the default scoring path): a count may read -1 and a sum NaN / -inf
    where the hypothesis cannot win.  solve=False skips the comparison of hypF with the 8-point solve (hand-made hypF).
    Asserts, each stage given the inputs it actually received:
      * every decided solve: hypF within tol of fundamental_8pt, either sign;
      * with the device's own hypF through residuals: a carried count in [lo, hi]; a carried finite sum within sum_tol where
        sum_ok; in "all" mode every count and sum is carried; in "ties" mode a NaN sum only with a -1 count or where the
        sum is not sum_ok (where a -1 and a -inf are allowed follows from the winner rules below);
      * the winner: best[1] in its [lo, hi]; no hypothesis has lo above the winner's hi; among the hypotheses decided to tie
        with it (lo == hi == its count) none has a float64 sum above the winner's by more than the two bounds; F is its hypF;
        without a winner (-1) no hypothesis has a decided inlier;
      * the mask equals e <= thr on every decided match of the winner; best[3] and matches are the masked pairs in order.
    Returns counts (new_ransac_stats): solves held / undecided, evaluations decided / undecided, pairs = 1 when the winner
    check was held (at most 1 % of the winner's evaluations undecided, one at least allowed; without a winner: no hypothesis
    has an undecided evaluation), and the largest error / bound ratios."""
    st = new_ransac_stats()
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = len(pairs)
    sets = np.asarray(sets).reshape(-1, 8)
    H = len(sets)
    hypF = np.asarray(out["hypF"], np.float32).reshape(H, 9)
    cnt = np.asarray(out["hyp_count"]).reshape(H).astype(np.int64)
    hs = np.asarray(out["hyp_sum"], np.float32).reshape(H).astype(np.float64)
    best = np.asarray(out["best"]).reshape(4)
    w = int(best[0])
    # ---- the solves
    if solve:
        st["solves"], st["solves_undecided"], st["worst_F"], st["solves_tight"] = fundamental_check(xy1, xy2, pairs, sets, hypF)
    # ---- counts and sums, from the device's own hypotheses
    r = residuals(hypF, xy1, xy2, pairs, thr, keep=[w] if w >= 0 else [])
    lo, hi = r["lo"], r["hi"]
    st["evals"], st["evals_undecided"] = int(H * n - r["n_undecided"].sum()), int(r["n_undecided"].sum())
    carried = cnt >= 0
    if mode == "all":
        assert carried.all(), ("a count is missing in all-sums mode", np.nonzero(~carried)[0][:5])
    bad = np.nonzero(carried & ((cnt < lo) | (cnt > hi)))[0]
    assert bad.size == 0, ("inlier count", bad[:5], cnt[bad[:5]], lo[bad[:5]], hi[bad[:5]])
    assert (cnt[~carried] == -1).all(), "a negative count other than -1"
    fin = np.isfinite(hs)
    chk = fin & r["sum_ok"] & (carried if mode != "all" else True)
    with np.errstate(invalid="ignore"):
        sratio = np.abs(hs[chk] - r["sum"][chk]) / r["sum_tol"][chk]
    if chk.any():
        h = int(np.nonzero(chk)[0][sratio.argmax()])
        assert sratio.max() <= 1.0, ("residual sum", h, float(hs[h]), float(r["sum"][h]), float(r["sum_tol"][h]))
        st["worst_sum"] = float(sratio.max())
    if mode == "all":
        bad = np.nonzero(r["sum_ok"] & (np.abs(r["sum"]) + r["sum_tol"] < _HUGE) & ~fin)[0]
        assert bad.size == 0, ("a sum is missing in all-sums mode", bad[:5], hs[bad[:5]])
    # ---- the winner
    if w < 0:
        assert (lo == 0).all(), ("no winner, yet a hypothesis has decided inliers", int(lo.argmax()), int(lo.max()))
        assert best[3] == 0
        held = bool((hi == 0).all())
        st["pairs"], st["pairs_undecided"] = int(held), int(not held)
        return st
    assert 0 <= w < H
    assert lo[w] <= int(best[1]) <= hi[w], ("winner's count", w, int(best[1]), int(lo[w]), int(hi[w]))
    if carried[w]:
        assert int(best[1]) == cnt[w], ("best count is not the winner's", int(best[1]), int(cnt[w]))
    # a maximum-count hypothesis as float64 sees it (this also covers every abandoned hypothesis: a -1 with lo above the
    # winner's hi would be one of these)
    above = np.nonzero(lo > hi[w])[0]
    assert above.size == 0, ("a hypothesis has more inliers than the winner", w, int(hi[w]), above[:5], lo[above[:5]])
    if mode != "all":
        bad = np.nonzero(np.isnan(hs) & carried & r["sum_ok"])[0]
        assert bad.size == 0, ("a counted hypothesis without its sum", bad[:5])
    # among the hypotheses decided to tie with the winner none has the larger sum, whatever the device reports for it
    # (a finite sum, -inf "pruned", or a -1 count "abandoned on the sum")
    if r["sum_ok"][w] and lo[w] == hi[w]:
        tie = (lo == hi) & (lo == lo[w]) & r["sum_ok"]
        beat = np.nonzero(tie & (r["sum"] - r["sum_tol"] > r["sum"][w] + r["sum_tol"][w]))[0]
        assert beat.size == 0, ("a tied hypothesis has the larger residual sum", w, float(r["sum"][w]), beat[:5], r["sum"][beat[:5]])
    assert np.array_equal(np.asarray(out["F"], np.float32).reshape(9).view(np.uint32), hypF[w].view(np.uint32)), "F is not the winner's"
    # ---- mask and filtered matches
    mask = np.asarray(out["mask"]).reshape(-1)[:n] != 0
    d = r["decided"][0]
    bad = np.nonzero(d & (mask != r["inlier"][0]))[0]
    assert bad.size == 0, ("inlier mask", w, bad[:5], r["e"][0][bad[:5]], r["tol"][0][bad[:5]])
    k = int(mask.sum())
    assert int(best[3]) == k, ("kept matches", int(best[3]), k)
    assert np.array_equal(np.asarray(out["matches"]).reshape(-1, 2)[:k], pairs[mask]), "matches are not the masked pairs in order"
    held = int((~d).sum()) <= max(1, n // 100)
    st["pairs"], st["pairs_undecided"] = int(held), int(not held)
    return st
