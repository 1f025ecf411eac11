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
