"""include/vslam_fuse_project.h restated from its text, not from the device code, by COMPOSING tests/ref_search.py (the search by
projection of one pose) and tests/ref_fuse.py (valid entries, a sound CSR, the fusion): neither is restated here.

project_item()    the rule for one item: per camera the TRIED points compacted into an item of their own and handed to
                  ref_search.search_item (compaction keeps the points' order, so the (d0, i) order is the item's); holders from a
                  table filled with np.minimum.at.  `plant` swaps in one wrong reading of the rule (PLANTS).
project_second()  the same rule a second way: one search_item call per camera over ALL the points with the rows of the points that
                  are not tried emptied; holders from a dictionary.
project_batch()   the arrays the entry point writes for a batch, over a caller's prefill.
merge_extras() / world_csr() / world_fuse_project()   what vslam_world_fuse_project does to a world beside its map: the extra log, the
                  map's log with each point's extras appended, the fusion over it.
random_item() / batch_of()   the random items of the tests."""
import numpy as np

import ref_fuse as rf
import ref_search as rs

f64 = np.float64
PLANTS = ("skip_off", "holder_largest", "held_taken", "order_ic")
OUTS = ("found_point", "found_cam", "found_kp", "found_dist", "found_holder")
MAX_KP, MAX_CAMS = 16384, 1024


def _arrays(points, offsets, cam, kp, obs_desc, R, T, xy, desc, n_kp):
    return (np.asarray(points, np.float32).reshape(-1, 4), np.asarray(offsets, np.int64), np.asarray(cam, np.int64), np.asarray(kp, np.int64),
            np.asarray(obs_desc, np.uint8).reshape(-1, 32), np.asarray(R, f64).reshape(-1, 9), np.asarray(T, f64).reshape(-1, 3),
            np.asarray(xy, np.float32), np.asarray(desc, np.uint8), np.asarray(n_kp, np.int64))


def _empty():
    z = np.zeros(0, np.int32)
    return dict(found_point=z, found_cam=z, found_kp=z, found_dist=z, found_holder=z, n_found=0, stats=np.zeros(6, np.int32))


def _taking_part(points, n, off, O):
    """rule 1 -> (S,) bool"""
    S = len(points)
    part = np.zeros(S, bool)
    part[:n] = (off[:n] >= 0) & (off[:n] < off[1:n + 1]) & (off[1:n + 1] <= O) & np.isfinite(points[:n, :3]).all(1)
    return part


def _cameras(R, T, n_cams, cam_mask):
    """rule 2 -> the cameras taking part, ascending"""
    Cs = len(R)
    C = min(max(int(n_cams), 0), Cs)
    ok = np.isfinite(R).all(1) & np.isfinite(T).all(1) & (np.arange(Cs) < C)
    if cam_mask is not None:
        ok &= np.asarray(cam_mask, np.int64)[:Cs] >= 0
    return np.flatnonzero(ok)


def _finish(found, tried, visible, proposing, found_stride, plant=None):
    """found: (c, i, k, d0, holder) tuples in any order -> the outputs"""
    found.sort(key=(lambda t: (t[1], t[0])) if plant == "order_ic" else (lambda t: (t[0], t[1])))
    m = len(found) if found_stride is None else min(len(found), int(found_stride))
    a = np.array(found, np.int32).reshape(-1, 5)
    stats = np.array([tried, visible, proposing, len(found), int((a[:, 4] >= 0).sum()), m], np.int32)
    return dict(found_cam=a[:m, 0].copy(), found_point=a[:m, 1].copy(), found_kp=a[:m, 2].copy(), found_dist=a[:m, 3].copy(),
                found_holder=a[:m, 4].copy(), n_found=m, stats=stats)


def project_item(points, n_points, offsets, cam, kp, obs_desc, R, T, n_cams, xy, desc, n_kp, K, width, height, cam_mask=None,
                 found_stride=None, plant=None, **kw):
    """points (S, 4) f32, offsets (S + 1,), cam / kp (O,), obs_desc (O, 32) u8, R (Cs, 9) / T (Cs, 3) f64, xy (Cs, Kp, 2) f32, desc (Cs, Kp,
    32) u8, n_kp (Cs,), cam_mask (Cs,) or None, K 3 x 3 f32; found_stride None: every found pair is written.  -> dict: found_point,
    found_cam, found_kp, found_dist, found_holder (m,) i32; n_found = m; stats (6,) i32."""
    assert plant is None or plant in PLANTS
    points, off, cam, kp, obs_desc, R, T, xy, desc, n_kp = _arrays(points, offsets, cam, kp, obs_desc, R, T, xy, desc, n_kp)
    S, O, Cs, Kp = len(points), len(cam), len(R), xy.shape[1]
    n = min(max(int(n_points), 0), S)
    if not rf.csr_ok(off, n, O):
        return _empty()
    part = _taking_part(points, n, off, O)
    rows = np.repeat(np.arange(n), np.diff(off[:n + 1]))                  # the point of every CSR row below offsets[n]
    e_cam, e_kp = cam[off[0]:off[n]], kp[off[0]:off[n]]
    valid = (e_cam >= 0) & (e_cam < Cs) & (e_kp >= 0) & (e_kp < Kp)
    holder = np.full((Cs, Kp), -1 if plant == "holder_largest" else n, np.int64)
    (np.maximum if plant == "holder_largest" else np.minimum).at(holder, (e_cam[valid], e_kp[valid]), rows[valid])
    holder[holder == n] = -1
    seen = np.zeros((S, Cs), bool)
    seen[rows[valid], e_cam[valid]] = True
    found, tried_n, visible, proposing = [], 0, 0, 0
    for c in _cameras(R, T, n_cams, cam_mask):
        idx = np.flatnonzero(part if plant == "skip_off" else part & ~seen[:, c])
        tried_n += len(idx)
        if len(idx) == 0:
            continue
        counts = (off[idx + 1] - off[idx]).astype(np.int64)
        sub_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        sub_obs = np.concatenate([obs_desc[off[i]:off[i + 1]] for i in idx])
        taken = np.where(holder[c] >= 0, 0, -1).astype(np.int32) if plant == "held_taken" else None
        r = rs.search_item(points[idx], len(idx), sub_off, sub_obs, R[c], T[c], K, width, height, xy[c], desc[c], n_kp[c], taken, **kw)
        visible += int(r["stats"][0])
        proposing += int(r["stats"][2])
        for j in np.flatnonzero(r["kp_of_point"] >= 0):
            k = int(r["kp_of_point"][j])
            found.append((int(c), int(idx[j]), k, int(r["dist"][j]), int(holder[c, k])))
    return _finish(found, tried_n, visible, proposing, found_stride, plant)


def project_second(points, n_points, offsets, cam, kp, obs_desc, R, T, n_cams, xy, desc, n_kp, K, width, height, cam_mask=None,
                   found_stride=None, **kw):
    """The same outputs another way: per camera one search_item call over all S points, the rows of every point that is not tried
    emptied (an empty row is invisible by the search's own rule 1); holders from a dictionary walked from the last point down."""
    points, off, cam, kp, obs_desc, R, T, xy, desc, n_kp = _arrays(points, offsets, cam, kp, obs_desc, R, T, xy, desc, n_kp)
    S, O, Cs, Kp = len(points), len(cam), len(R), xy.shape[1]
    n = min(max(int(n_points), 0), S)
    if not (off[0] >= 0 and (np.diff(off[:n + 1]) >= 0).all() and (off[:n + 1] <= O).all()):
        return _empty()
    holders, cams_of = {}, [set() for _ in range(S)]
    for i in range(n - 1, -1, -1):
        for o in range(off[i], off[i + 1]):
            if 0 <= cam[o] < Cs and 0 <= kp[o] < Kp:
                holders[(int(cam[o]), int(kp[o]))] = i
                cams_of[i].add(int(cam[o]))
    found, tried_n, visible, proposing = [], 0, 0, 0
    for c in range(Cs):
        if c >= min(max(int(n_cams), 0), Cs) or not (np.isfinite(R[c]).all() and np.isfinite(T[c]).all()):
            continue
        if cam_mask is not None and int(cam_mask[c]) < 0:
            continue
        tried = [i < n and 0 <= off[i] < off[i + 1] <= O and bool(np.isfinite(points[i, :3]).all()) and c not in cams_of[i] for i in range(S)]
        tried_n += sum(tried)
        counts = [int(off[i + 1] - off[i]) if tried[i] else 0 for i in range(S)]
        off2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        obs2 = np.concatenate([obs_desc[off[i]:off[i + 1]] for i in range(S) if tried[i]] + [np.zeros((0, 32), np.uint8)])
        r = rs.search_item(points, n, off2, obs2, R[c], T[c], K, width, height, xy[c], desc[c], n_kp[c], None, **kw)
        visible += int(r["stats"][0])
        proposing += int(r["stats"][2])
        for i, k, d in zip(r["corr_point"], r["corr_kp"], r["dist"][r["corr_point"]]):
            found.append((c, int(i), int(k), int(d), holders.get((c, int(k)), -1)))
    return _finish(found, tried_n, visible, proposing, found_stride)


def project_batch(items, K, width, height, found_stride, prefill=None, **kw):
    """items: batch_of()'s dict of stacked arrays -> the arrays vslam_fuse_project writes, over `prefill` (a dict of the caller's output
    arrays; zeros when None): slots from an item's n_found on keep the prefill"""
    B = len(items["n"])
    shapes = {k: (B, found_stride) for k in OUTS}
    shapes.update(n_found=(B,), stats=(B, 6))
    out = {k: (np.zeros(s, np.int32) if prefill is None or k not in prefill else np.array(prefill[k], np.int32).reshape(s)) for k, s in shapes.items()}
    for b in range(B):
        r = project_item(items["points"][b], items["n"][b], items["offsets"][b], items["cam"][b], items["kp"][b], items["obs_desc"][b],
                         items["R"][b], items["T"][b], items["n_cams"][b], items["xy"][b], items["desc"][b], items["n_kp"][b], K, width, height,
                         None if items.get("cam_mask") is None else items["cam_mask"][b], found_stride, **kw)
        m = r["n_found"]
        out["n_found"][b], out["stats"][b] = m, r["stats"]
        for k in OUTS:
            out[k][b, :m] = r[k]
    return out


# ------------------------------------------------------------------------------------------------ on the world
def merge_extras(size, off, frame, kp, extras, obs_capacity):
    """The map's log (off (P + 1,), frame / kp: its rows) with each point's extras appended to its row in the order they were
    appended.  extras: (E, 3) rows (point, frame, kp), the log in order; the longest prefix is admitted with which the total stays
    within obs_capacity.  -> (off (P + 1,), frame, kp, src (total,): the map's row, or obs_capacity + e for extra e), int32"""
    off = np.asarray(off, np.int64)
    P = len(off) - 1
    n = min(max(int(size), 0), P)
    extras = np.asarray(extras, np.int64).reshape(-1, 3)
    admit = min(len(extras), max(int(obs_capacity) - int(off[n]), 0))
    rows = [[(int(frame[o]), int(kp[o]), o) for o in range(off[i], off[i + 1])] for i in range(n)]
    for e in range(admit):
        rows[extras[e, 0]].append((int(extras[e, 1]), int(extras[e, 2]), int(obs_capacity) + e))
    out = np.zeros(P + 1, np.int32)
    out[1:n + 1] = np.cumsum([len(r) for r in rows])
    out[n + 1:] = out[n]
    flat = np.array([t for r in rows for t in r], np.int32).reshape(-1, 3)
    return out, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].copy()


def world_csr(fuse_to, size, off, frame, kp, map_desc, extras, extra_desc, max_frames, kp_stride, obs_capacity):
    """One track of the world's CSR once extras exist: merge_extras, then the fusion with d_mask = fuse_to, descriptors gathered from
    the map's (map_desc (O, 32)) or the log's (extra_desc (E, 32)) -> (the fusion's result, desc (total, 32))"""
    o2, f2, k2, src = merge_extras(size, off, frame, kp, extras, obs_capacity)
    r = rf.fuse_item(size, o2, f2, k2, max_frames, kp_stride, fuse_to)
    both = np.concatenate([np.asarray(map_desc, np.uint8).reshape(-1, 32)[:obs_capacity], np.zeros((max(obs_capacity - len(map_desc), 0), 32), np.uint8),
                           np.asarray(extra_desc, np.uint8).reshape(-1, 32)])
    return r, both[src[r["out_src"]]]


def world_fuse_project(fuse_to, world_points, size, off, frame, kp, map_desc, extras, extra_desc, Twc, frames, xy, desc, n_kp, K, width,
                       height, lo, hi, max_frames, kp_stride, obs_capacity, **kw):
    """One track of vslam_world_fuse_project on the state read back before the call: fuse_to (P,) or None ("no fusion"), extras (E, 3)
    / extra_desc (E, 32) the log so far, the map's own CSR and its descriptors, xy / desc / n_kp the caller's keypoints of every
    frame.  -> dict(item: project_item's result, extras, extra_desc: the log afterwards, fuse_to, world_points afterwards, stats (8,))"""
    P = len(off) - 1
    extras = np.asarray(extras, np.int64).reshape(-1, 3)
    extra_desc = np.asarray(extra_desc, np.uint8).reshape(-1, 32)
    before = np.arange(P, dtype=np.int32) if fuse_to is None else np.asarray(fuse_to, np.int32)
    if fuse_to is None and len(extras) == 0:
        c_off, c_frame, c_kp = np.asarray(off, np.int32), np.asarray(frame, np.int32), np.asarray(kp, np.int32)
        c_desc = np.asarray(map_desc, np.uint8).reshape(-1, 32)[:c_off[min(max(int(size), 0), P)]]
    else:
        r0, c_desc = world_csr(before, size, off, frame, kp, map_desc, extras, extra_desc, max_frames, kp_stride, obs_capacity)
        c_off, c_frame, c_kp = r0["out_offsets"], r0["out_cam"], r0["out_kp"]
    R, T = rf.cameras(Twc, frames)
    mask = np.where((np.arange(max_frames) >= lo) & (np.arange(max_frames) < hi), 0, -1).astype(np.int32)
    item = project_item(world_points, size, c_off, c_frame, c_kp, c_desc, R, T, frames, xy, desc, n_kp, K, width, height, mask, obs_capacity, **kw)
    take = min(item["n_found"], obs_capacity - len(extras))
    new = np.stack([item["found_point"][:take], item["found_cam"][:take], item["found_kp"][:take]], 1).astype(np.int64)
    new_desc = np.asarray(desc, np.uint8)[item["found_cam"][:take], item["found_kp"][:take]].reshape(-1, 32)
    extras, extra_desc = np.concatenate([extras, new]), np.concatenate([extra_desc, new_desc])
    o2, f2, k2, _ = merge_extras(size, off, frame, kp, extras, obs_capacity)
    r, after, pts = rf.world_fuse(before, world_points, size, o2, f2, k2, max_frames, kp_stride)
    return dict(item=item, extras=extras.astype(np.int32), extra_desc=extra_desc, fuse_to=after, world_points=pts, fusion=r,
                stats=np.concatenate([item["stats"], [take, len(extras)]]).astype(np.int32))


# ------------------------------------------------------------------------------------------------ random items
def random_item(seed, n, n_cams, kp_stride=96, cam_stride=None, S=None, width=640, height=480):
    """n map points that are copies of max(n // 3, 1) physical features (so most features are in the item three times), each observed in 1
    .. 3 of the cameras that see its feature; the cameras on a line as ref_fuse.random_cull_item has them; per camera a keypoint
    for about 70 % of the features while slots last (their projection with N(0, 0.5 px) noise, the feature's descriptor through
    ref_search.flip_bits), distractors behind them, n_kp differing per camera -- one above kp_stride, one cutting keypoints off;
    a non-finite camera, a few non-finite points and keypoints, empty rows, entries out of range; rows past n junk."""
    import ref_resect as rr
    rng = np.random.default_rng(seed)
    S, Cs = S or n, cam_stride or n_cams
    K = rr.kmat()
    Kd = K.astype(f64)
    R, T = np.zeros((Cs, 9)), np.zeros((Cs, 3))
    for c in range(Cs):
        w = rng.normal(0, 0.03, 3)
        th = np.linalg.norm(w)
        a = w / th
        Ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R[c] = (np.eye(3) + np.sin(th) * Ax + (1 - np.cos(th)) * Ax @ Ax).reshape(9)
        T[c] = [-0.05 * c, rng.normal(0, 0.02), rng.normal(0, 0.02)]
    if n_cams > 3:
        R[n_cams // 2, 4] = np.nan
    F = max(n // 3, 1)
    X = np.stack([rng.uniform(-1.5, 1.5, F), rng.uniform(-1.1, 1.1, F), rng.uniform(4, 9, F)], 1)
    base = rng.integers(0, 256, (F, 32), dtype=np.uint8)
    xy = rng.uniform(0, [width, height], (Cs, kp_stride, 2)).astype(np.float32)
    desc = rng.integers(0, 256, (Cs, kp_stride, 32), dtype=np.uint8)
    n_kp = np.zeros(Cs, np.int32)
    kp_of = np.full((Cs, F), -1, np.int64)
    for c in range(n_cams):
        if not np.isfinite(R[c]).all():
            n_kp[c] = kp_stride
            continue
        cap = int(rng.integers(kp_stride // 2, kp_stride + 1))
        feats = rng.permutation(np.flatnonzero(rng.uniform(size=F) < 0.7))[:max(cap - 8, 1)]
        slots = rng.permutation(cap)[:len(feats)]
        Y = X[feats] @ R[c].reshape(3, 3).T + T[c]
        q = Y @ Kd.T
        xy[c, slots] = (q[:, :2] / q[:, 2:] + rng.normal(0, 0.5, (len(feats), 2))).astype(np.float32)
        for f, k in zip(feats, slots):
            desc[c, k] = rs.flip_bits(rng, base[f], 20)
        kp_of[c, feats] = slots
        n_kp[c] = cap
    if n_cams >= 2:
        n_kp[0] = kp_stride + 5                  # clamped to kp_stride
        n_kp[1] = max(int(n_kp[1]) - 6, 0)       # cuts keypoints off: entries that name them stay valid, the search does not see them
    xy[0, 3] = np.nan
    points = np.ones((S, 4), np.float32)
    feat = np.arange(S) % F
    points[:, :3] = X[feat] + rng.normal(0, 0.002, (S, 3))
    cams, kps = [], []
    counts = np.zeros(S, np.int64)
    for i in range(S):
        sees = np.flatnonzero(kp_of[:, feat[i]] >= 0)
        pick = rng.permutation(sees)[:int(rng.integers(1, 4))]
        if rng.uniform() < 0.03:
            pick = pick[:0]                      # an empty row
        counts[i] = len(pick)
        cams += list(pick)
        kps += list(kp_of[pick, feat[i]])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    O = max(int(offsets[-1]), 1)
    cam, kp = np.zeros(O, np.int32), np.zeros(O, np.int32)
    cam[:len(cams)], kp[:len(kps)] = cams, kps
    owner = np.repeat(np.arange(S), counts)
    obs_desc = np.zeros((O, 32), np.uint8)
    for o, i in enumerate(owner):
        obs_desc[o] = rs.flip_bits(rng, base[feat[i]], 20)
    bad = rng.uniform(size=O) < 0.03
    cam[bad] = rng.choice([-1, Cs, Cs + 3])
    kp[rng.uniform(size=O) < 0.02] = kp_stride
    for i in rng.integers(0, max(n, 1), 2 if n > 8 else 0):
        points[i, rng.integers(0, 3)] = [np.nan, np.inf, -np.inf][rng.integers(0, 3)]
    return dict(points=points, n=n, offsets=offsets, cam=cam, kp=kp, obs_desc=obs_desc, R=R, T=T, n_cams=n_cams, xy=xy, desc=desc, n_kp=n_kp,
                cam_mask=None, K=K, width=width, height=height)


def reference(c, **kw):
    p = dict(c.get("params", {}))
    p.update(kw)
    return project_item(c["points"], c["n"], c["offsets"], c["cam"], c["kp"], c["obs_desc"], c["R"], c["T"], c["n_cams"], c["xy"], c["desc"],
                        c["n_kp"], c["K"], c["width"], c["height"], c.get("cam_mask"), c.get("found_stride"), **p)


def second(c):
    return project_second(c["points"], c["n"], c["offsets"], c["cam"], c["kp"], c["obs_desc"], c["R"], c["T"], c["n_cams"], c["xy"], c["desc"],
                          c["n_kp"], c["K"], c["width"], c["height"], c.get("cam_mask"), c.get("found_stride"), **c.get("params", {}))


def batch_of(items):
    """items of different sizes padded into one batch: the strides are the largest; padding rows are junk that the counts keep out
    (offsets past an item's own repeat its last; cameras past its own are not finite).  Every item gets a mask (zeros when it had
    none)."""
    B = len(items)
    S = max(len(it["points"]) for it in items)
    O = max(len(it["cam"]) for it in items)
    Cs = max(len(it["R"]) for it in items)
    Kp = max(it["xy"].shape[1] for it in items)
    out = dict(points=np.full((B, S, 4), 3.0, np.float32), n=np.array([it["n"] for it in items], np.int32), offsets=np.zeros((B, S + 1), np.int32),
               cam=np.full((B, O), 1, np.int32), kp=np.full((B, O), 2, np.int32), obs_desc=np.full((B, O, 32), 0x5A, np.uint8),
               R=np.full((B, Cs, 9), np.nan), T=np.zeros((B, Cs, 3)), n_cams=np.array([it["n_cams"] for it in items], np.int32),
               xy=np.full((B, Cs, Kp, 2), 7.0, np.float32), desc=np.zeros((B, Cs, Kp, 32), np.uint8), n_kp=np.zeros((B, Cs), np.int32),
               cam_mask=np.zeros((B, Cs), np.int32))
    for b, it in enumerate(items):
        s, o, c, k = len(it["points"]), len(it["cam"]), len(it["R"]), it["xy"].shape[1]
        out["points"][b, :s] = it["points"]
        out["offsets"][b, :s + 1] = it["offsets"]
        out["offsets"][b, s + 1:] = it["offsets"][s]
        out["cam"][b, :o], out["kp"][b, :o], out["obs_desc"][b, :o] = it["cam"], it["kp"], it["obs_desc"]
        out["R"][b, :c], out["T"][b, :c] = it["R"], it["T"]
        out["xy"][b, :c, :k], out["desc"][b, :c, :k] = it["xy"], it["desc"]
        out["n_kp"][b, :c] = np.minimum(it["n_kp"], k) if k < Kp else it["n_kp"]
        if it.get("cam_mask") is not None:
            out["cam_mask"][b, :c] = it["cam_mask"]
    return out
