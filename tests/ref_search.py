"""The search by projection (include/vslam_search.h: vslam_search_projection) restated in numpy, written from the header's text --
not from the device code: brute force over ALL keypoints of the item, no grid.  Floating point is float64, one IEEE operation per
Python operator in the header's order (the projection is ref_resect.transform / project); everything behind the disc test is
integers, so every output is held bit for bit.

search_item()        the rule for one item.  `plant` swaps in one wrong reading of the rule (PLANTS) for the tests that must catch it.
search_batch()       the items of a batch stacked into the arrays the entry point writes, over a caller's prefill.
second_formulation() the same rule through scipy.spatial.cKDTree (discs, with the exact test reapplied to a slightly wider query)
                     and np.unpackbits (distances), resolved by sorting proposals instead of keeping minima.
planted_scene()      the scenes of tests/test_ref_search.py and tests/test_gpu_search.py.

Measured on planted_scene(seed), seeds 1 .. 6, at the defaults (radius 8, threshold 64, ratio10 8); test_ref_search.py re-measures
and compares against MEASURED_*:
  found / seen  and  wrong / found  per seed: MEASURED_SHARES below (the conditions are >= 0.90 and <= 0.05).
  exact scenes (planted_scene(seed, exact=True): no noise, no near-copies), ref_resect.resect over the found correspondences from
  the start pose: max|R - R_true|, max|T - T_true| per seed in MEASURED_EXACT; EXACT_BOUND_R / EXACT_BOUND_T = 4 x the worst.
"""
import numpy as np

import ref_resect as rr

f64 = np.float64
DEFAULTS = dict(radius_px=8.0, dist_threshold=64, ratio10=8)
PLANTS = ("disc_open", "first_observation", "d1_over_all", "tie_to_higher_point", "ratio_on_single")
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)
MAX_KP = 16384

# (found / seen, wrong / found) of planted_scene(seed), seeds 1 .. 6
MEASURED_SHARES = {1: (0.9670, 0.0), 2: (0.9714, 0.0), 3: (0.9831, 0.0), 4: (0.9779, 0.0), 5: (0.9708, 0.0), 6: (0.9770, 0.0)}
# (max|R - R_true|, max|T - T_true|) of planted_scene(seed, exact=True) after ref_resect.resect, seeds 1 .. 6 (rounded up)
MEASURED_EXACT = {1: (5.9e-09, 3.3e-08), 2: (3.1e-09, 1.7e-08), 3: (7.4e-09, 4.3e-08), 4: (4.3e-09, 2.8e-08), 5: (4.5e-09, 3.8e-08),
                  6: (3.9e-09, 5.2e-08)}
EXACT_BOUND_R = 4 * max(v[0] for v in MEASURED_EXACT.values())
EXACT_BOUND_T = 4 * max(v[1] for v in MEASURED_EXACT.values())


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params_ok(p):
    r = p["radius_px"]
    return bool(np.isfinite(r) and 0 < r <= 64 and 1 <= p["dist_threshold"] <= 257 and 0 <= p["ratio10"] <= 10)


def hamming(a, b):
    """a (..., 32) u8, b (..., 32) u8 -> the 256-bit Hamming distances (broadcast)"""
    return POPCOUNT[np.bitwise_xor(a, b)].sum(-1)


def visible(points, n, offsets, obs_stride, R, T, K, width, height):
    """rule 1 -> vis (n,) bool, u, v (n,) f64"""
    P32 = np.asarray(points, np.float32).reshape(-1, 4)[:n, :3]
    P = P32.astype(f64)
    R, T = np.asarray(R, f64).reshape(9), np.asarray(T, f64).reshape(3)
    K = np.asarray(K, np.float32).astype(f64).reshape(9)
    off = np.asarray(offsets, np.int64)
    o0, o1 = off[:n], off[1:n + 1]
    with np.errstate(all="ignore"):
        vis = (o0 >= 0) & (o0 < o1) & (o1 <= obs_stride) & np.isfinite(P32).all(1)
        vis &= bool(np.isfinite(R).all() and np.isfinite(T).all())
        _, Y = rr.transform(R, T, P)
        vis &= np.isfinite(Y).all(1) & (Y[:, 2] > 0.0)
        u, v, _ = rr.project(K, Y)
        vis &= np.isfinite(u) & np.isfinite(v) & (u >= 0.0) & (u < f64(width)) & (v >= 0.0) & (v < f64(height))
    return vis, u, v


def search_item(points, n_points, offsets, obs_desc, R, T, K, width, height, xy, desc, n_kp, taken=None, plant=None, **kw):
    """points (S, 4) f32, offsets (S + 1,) i32, obs_desc (O, 32) u8, R (9,) / T (3,) f64, K 3 x 3 f32, xy (Kp, 2) f32, desc (Kp, 32)
    u8, taken (Kp,) i32 or None.  -> dict: kp_of_point, dist (S,) i32; corr_points (m, 3) f64, corr_xy (m, 2) f32, corr_point,
    corr_kp (m,) i32; n_corr; stats (4,) i32."""
    assert plant is None or plant in PLANTS
    p = params(**kw)
    points = np.asarray(points, np.float32).reshape(-1, 4)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    obs_desc = np.asarray(obs_desc, np.uint8).reshape(-1, 32)
    S, Kp, O = len(points), len(xy), len(obs_desc)
    n = min(max(int(n_points), 0), S)
    nk = min(max(int(n_kp), 0), Kp)
    off = np.asarray(offsets, np.int64)
    vis, u, v = visible(points, n, off, O, R, T, K, width, height)
    x, y = xy[:nk, 0], xy[:nk, 1]
    kp_ok = np.isfinite(x) & np.isfinite(y)
    if taken is not None:
        kp_ok &= np.asarray(taken, np.int64)[:nk] < 0
    xd, yd = x.astype(f64), y.astype(f64)
    radius = f64(p["radius_px"])
    r2 = radius * radius
    thr, ratio10 = int(p["dist_threshold"]), int(p["ratio10"])
    proposals = {}   # keypoint -> the smallest key (d0, i)
    with_candidate = proposing = 0
    for i in np.flatnonzero(vis):
        with np.errstate(all="ignore"):
            dx, dy = xd - u[i], yd - v[i]
            s = dx * dx + dy * dy
            inside = (s < r2) if plant == "disc_open" else (s <= r2)
        ks = np.flatnonzero(kp_ok & inside)
        if len(ks) == 0:
            continue
        with_candidate += 1
        obs = obs_desc[off[i]:off[i + 1]]
        if plant == "first_observation":
            obs = obs[:1]
        d = hamming(desc[ks][:, None, :], obs[None, :, :]).min(1)   # orb_distance per candidate
        order = np.lexsort((ks, d))
        d0, k0 = int(d[order[0]]), int(ks[order[0]])
        d1 = int(d[order[1]]) if len(ks) > 1 else None
        if plant == "d1_over_all":
            d1 = d0
        if plant == "ratio_on_single" and d1 is None:
            d1 = d0
        if not (d0 < thr and (ratio10 == 0 or d1 is None or 10 * d0 < ratio10 * d1)):
            continue
        proposing += 1
        key = (d0, -int(i)) if plant == "tie_to_higher_point" else (d0, int(i))
        if k0 not in proposals or key < proposals[k0]:
            proposals[k0] = key
    kp_of_point = np.full(S, -1, np.int32)
    dist = np.full(S, -1, np.int32)
    for k0, (d0, i) in proposals.items():
        kp_of_point[abs(i)] = k0
        dist[abs(i)] = d0
    found = np.flatnonzero(kp_of_point >= 0)   # ascending point index
    return dict(kp_of_point=kp_of_point, dist=dist, corr_points=points[found, :3].astype(f64), corr_xy=xy[kp_of_point[found]].copy(),
                corr_point=found.astype(np.int32), corr_kp=kp_of_point[found].copy(), n_corr=len(found),
                stats=np.array([int(vis.sum()), with_candidate, proposing, len(found)], np.int32))


def search_batch(points, n_points, offsets, obs_desc, R, T, K, width, height, xy, desc, n_kp, taken=None, prefill=None, **kw):
    """The arrays vslam_search_projection writes for a batch: points (B, S, 4), offsets (B, S + 1), obs_desc (B, O, 32), R (B, 9), T
    (B, 3), xy (B, Kp, 2), desc (B, Kp, 32), n_points / n_kp (B,), taken (B, Kp) or None.  prefill: dict of the caller's output
    arrays (copied; slots the rule does not write keep them), zeros when None."""
    B, S, Kp = points.shape[0], points.shape[1], xy.shape[1]
    shapes = dict(kp_of_point=((B, S), np.int32), dist=((B, S), np.int32), corr_points=((B, Kp, 3), f64), corr_xy=((B, Kp, 2), np.float32),
                  corr_point=((B, Kp), np.int32), corr_kp=((B, Kp), np.int32), n_corr=((B,), np.int32), stats=((B, 4), np.int32))
    out = {k: (np.zeros(s, t) if prefill is None or k not in prefill else np.array(prefill[k], t).reshape(s)) for k, (s, t) in shapes.items()}
    for b in range(B):
        r = search_item(points[b], n_points[b], offsets[b], obs_desc[b], R[b], T[b], K, width, height, xy[b], desc[b], n_kp[b],
                        None if taken is None else taken[b], **kw)
        m = r["n_corr"]
        out["kp_of_point"][b], out["dist"][b], out["n_corr"][b], out["stats"][b] = r["kp_of_point"], r["dist"], m, r["stats"]
        for k in ("corr_points", "corr_xy", "corr_point", "corr_kp"):
            out[k][b, :m] = r[k]
    return out


def second_formulation(points, n_points, offsets, obs_desc, R, T, K, width, height, xy, desc, n_kp, taken=None, **kw):
    """-> kp_of_point, dist (S,) i32 through another route: cKDTree.query_ball_point at a radius a little wider than the rule's,
    the exact disc test reapplied; distances as the set bits of the unpacked XOR; proposals sorted by (k0, d0, i) and the first of
    each keypoint kept."""
    from scipy.spatial import cKDTree
    p = params(**kw)
    points = np.asarray(points, np.float32).reshape(-1, 4)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    obs_desc = np.asarray(obs_desc, np.uint8).reshape(-1, 32)
    S = len(points)
    n = min(max(int(n_points), 0), S)
    nk = min(max(int(n_kp), 0), len(xy))
    off = np.asarray(offsets, np.int64)
    vis, u, v = visible(points, n, off, len(obs_desc), R, T, K, width, height)
    ok = np.isfinite(xy[:nk]).all(1)
    if taken is not None:
        ok &= np.asarray(taken, np.int64)[:nk] < 0
    idx = np.flatnonzero(ok)
    kp_of_point = np.full(S, -1, np.int32)
    dist = np.full(S, -1, np.int32)
    if len(idx) == 0:
        return kp_of_point, dist
    pts = xy[idx].astype(f64)
    tree = cKDTree(pts)
    radius = f64(p["radius_px"])
    bits_kp = np.unpackbits(desc, axis=1)
    bits_obs = np.unpackbits(obs_desc, axis=1)
    props = []
    for i in np.flatnonzero(vis):
        near = np.array(sorted(tree.query_ball_point([u[i], v[i]], radius * 1.001 + 1e-6)), np.int64)
        if len(near) == 0:
            continue
        dx, dy = pts[near, 0] - u[i], pts[near, 1] - v[i]
        near = near[dx * dx + dy * dy <= radius * radius]
        if len(near) == 0:
            continue
        ks = idx[near]
        d = np.array([min(int((bits_kp[k] != bits_obs[o]).sum()) for o in range(off[i], off[i + 1])) for k in ks])
        best = min(zip(d, ks))
        others = [dd for dd, k in zip(d, ks) if k != best[1]]
        if best[0] >= p["dist_threshold"]:
            continue
        if p["ratio10"] != 0 and others and not 10 * best[0] < p["ratio10"] * min(others):
            continue
        props.append((int(best[1]), int(best[0]), int(i)))
    last = None
    for k0, d0, i in sorted(props):
        if k0 != last:
            kp_of_point[i], dist[i] = k0, d0
        last = k0
    return kp_of_point, dist


# ------------------------------------------------------------------------------------------------ planted scenes
def flip_bits(rng, d, most):
    """d (32,) u8 with fewer than `most` distinct bits flipped"""
    out = d.copy()
    for bit in rng.choice(256, size=int(rng.integers(0, most)), replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], f64)


def planted_scene(seed, exact=False, points=300, distractors=200, copies=10):
    """300 world points with z in 4 .. 9 (in the true camera), random 256-bit descriptors, 1 .. 3 observations per point with fewer
    than 20 bits flipped; K = (525, 525, 320, 240) at 640 x 480; 80 % of the visible points seen as keypoints with N(0, 1 px) noise
    and fewer than 20 flipped bits; 10 near-copies 2 px beside a true keypoint; 200 random distractors; keypoints in permuted
    order; the start pose 0.01 rad about z and (0.02, 0.01, -0.02) off the true one.  exact=True: no noise, no near-copies.
    -> dict of one item's arrays (strides = the counts) and own (S,): the point's own keypoint or -1, R_true, T_true."""
    rng = np.random.default_rng(1000 + seed)
    W, H = 640, 480
    K = rr.kmat()
    z = rng.uniform(4.0, 9.0, points)
    Yc = np.stack([z * rng.uniform(-0.7, 0.7, points), z * rng.uniform(-0.55, 0.55, points), z], 1)   # in the true camera
    a = rng.normal(size=3)
    a = 0.2 * a / np.linalg.norm(a)
    th = np.linalg.norm(a)
    Ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R_true = np.eye(3) + np.sin(th) / th * Ax + (1 - np.cos(th)) / th ** 2 * Ax @ Ax
    T_true = rng.uniform(-1.0, 1.0, 3)
    Pw = (Yc - T_true) @ R_true            # rows R_true^t (Y - T)
    P4 = np.concatenate([Pw, np.ones((points, 1))], 1).astype(np.float32)
    base = rng.integers(0, 256, (points, 32), dtype=np.uint8)
    counts = rng.integers(1, 4, points)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs = np.stack([flip_bits(rng, base[i], 20) for i in range(points) for _ in range(counts[i])])
    Rt, Tt = R_true.reshape(9), T_true
    vis, u, v = visible(P4, points, offsets, len(obs), Rt, Tt, K, W, H)
    seen = vis & (rng.uniform(size=points) < 0.8)
    kxy, kdesc, owner = [], [], []
    for i in np.flatnonzero(seen):
        noise = np.zeros(2) if exact else rng.normal(0.0, 1.0, 2)
        kxy.append([u[i] + noise[0], v[i] + noise[1]])
        kdesc.append(flip_bits(rng, base[i], 20))
        owner.append(i)
    if not exact:
        for j in rng.choice(len(kxy), copies, replace=False):
            ang = rng.uniform(0, 2 * np.pi)
            kxy.append([kxy[j][0] + 2 * np.cos(ang), kxy[j][1] + 2 * np.sin(ang)])
            kdesc.append(flip_bits(rng, kdesc[j], 20))
            owner.append(-1)
    for _ in range(distractors):
        kxy.append([rng.uniform(0, W), rng.uniform(0, H)])
        kdesc.append(rng.integers(0, 256, 32, dtype=np.uint8))
        owner.append(-1)
    perm = rng.permutation(len(kxy))
    kxy = np.array(kxy, np.float32)[perm]
    kdesc = np.array(kdesc, np.uint8)[perm]
    owner = np.array(owner)[perm]
    own = np.full(points, -1, np.int64)
    own[owner[owner >= 0]] = np.flatnonzero(owner >= 0)
    R_start = rot_z(0.01) @ R_true
    T_start = rot_z(0.01) @ T_true + np.array([0.02, 0.01, -0.02])
    return dict(points=P4, n_points=points, offsets=offsets, obs_desc=obs, K=K, width=W, height=H, xy=kxy, desc=kdesc, n_kp=len(kxy),
                R=R_start.reshape(9).copy(), T=T_start.copy(), R_true=Rt.copy(), T_true=Tt.copy(), own=own, seen=seen)


def run_scene(sc, **kw):
    return search_item(sc["points"], sc["n_points"], sc["offsets"], sc["obs_desc"], sc["R"], sc["T"], sc["K"], sc["width"], sc["height"],
                       sc["xy"], sc["desc"], sc["n_kp"], **kw)


def scene_shares(sc, res):
    """(found / seen, wrong / found): of the points seen as a keypoint those given any keypoint; of the points given a keypoint
    those given one that is not their own"""
    got = res["kp_of_point"][:sc["n_points"]]
    found = got >= 0
    wrong = found & (got != sc["own"])
    return float((found & sc["seen"]).sum() / max(sc["seen"].sum(), 1)), float(wrong.sum() / max(found.sum(), 1))


def scene_resect(sc, res):
    """ref_resect.resect over the found correspondences from the scene's start pose -> (max|R - R_true|, max|T - T_true|)"""
    R, T, _, info = rr.resect(res["corr_points"], res["corr_xy"], sc["K"], sc["R"], sc["T"])
    return float(np.abs(R - sc["R_true"]).max()), float(np.abs(T - sc["T_true"]).max()), info["moved"]


def batch_of(scenes):
    """scenes (dicts of planted_scene's keys, or any with the same arrays) padded to common strides -> the arrays of search_batch"""
    B = len(scenes)
    S = max(len(s["points"]) for s in scenes)
    O = max(max(len(s["obs_desc"]) for s in scenes), 1)
    Kp = max(max(len(s["xy"]) for s in scenes), 1)
    out = dict(points=np.zeros((B, S, 4), np.float32), n_points=np.zeros(B, np.int32), offsets=np.zeros((B, S + 1), np.int32),
               obs_desc=np.zeros((B, O, 32), np.uint8), R=np.zeros((B, 9)), T=np.zeros((B, 3)), xy=np.zeros((B, Kp, 2), np.float32),
               desc=np.zeros((B, Kp, 32), np.uint8), n_kp=np.zeros(B, np.int32))
    for b, s in enumerate(scenes):
        n, o, k = len(s["points"]), len(s["obs_desc"]), len(s["xy"])
        out["points"][b, :n] = s["points"]
        out["offsets"][b, :n + 1] = s["offsets"]
        out["offsets"][b, n + 1:] = s["offsets"][n]
        out["obs_desc"][b, :o] = s["obs_desc"]
        out["xy"][b, :k] = s["xy"]
        out["desc"][b, :k] = s["desc"]
        out["n_points"][b], out["n_kp"][b] = s["n_points"], s["n_kp"]
        out["R"][b], out["T"][b] = s["R"], s["T"]
    return out
