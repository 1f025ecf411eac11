"""include/vslam_fuse.h restated from its text, not from the device code.

fuse_item()     vslam_fuse_points for one item: the groups by a union-find over the points, the merged order as plain loops.
fuse_second()   the same rule a second way: an explicit link graph searched breadth first, the kept entries by a set.
fuse_batch()    the arrays the entry point writes for a batch, over a caller's prefill.
cull_item()     vslam_cull_points for one item in numpy float64, one IEEE operation per Python operator in the header's order (the
                projection is ref_resect.transform / project, the resection's own).
cull_batch()    the arrays of a batch.
world_fuse() / world_cull_apply() / cameras()   what vslam_world_fuse and vslam_world_cull do to the world's d_fuse_to and
                d_world_points, given the map's observations.
random_fuse_item() / random_cull_item()         the random items of the tests."""
import numpy as np

import ref_resect as rr

f64 = np.float64
CULL_DEFAULTS = dict(inlier_px=6.0, min_good=2, mature_good=3, mature_age=3, good10=5)
QNAN_BITS = np.uint32(0x7FC00000)
MAX_KP, MAX_CAMS = 16384, 1024


def cull_params(**kw):
    p = dict(CULL_DEFAULTS)
    p.update(kw)
    return p


def cull_params_ok(p):
    return bool(np.isfinite(p["inlier_px"]) and p["inlier_px"] > 0 and p["min_good"] >= 1 and p["mature_good"] >= 1 and
                0 <= p["mature_age"] <= 1 << 20 and 0 <= p["good10"] <= 10)


def csr_ok(offsets, n, obs_stride):
    off = [int(x) for x in offsets[:n + 1]]
    if off[0] < 0:
        return False
    for a, b in zip(off[:-1], off[1:]):
        if b < a:
            return False
    return all(x <= obs_stride for x in off)


# ------------------------------------------------------------------------------------------------ the fusion
def fuse_item(n_points, offsets, cam, kp, cam_stride, kp_stride, mask=None):
    """offsets (S + 1,), cam / kp (O,), mask (S,) or None -> dict(fuse_to (S,), out_offsets (S + 1,), out_cam, out_kp, out_src (total,),
    stats (4,)), all int32"""
    offsets = np.asarray(offsets, np.int64)
    cam, kp = np.asarray(cam, np.int64), np.asarray(kp, np.int64)
    S, O = len(offsets) - 1, len(cam)
    n = min(max(int(n_points), 0), S)
    if not csr_ok(offsets, n, O):
        z = np.zeros(0, np.int32)
        return dict(fuse_to=np.arange(S, dtype=np.int32), out_offsets=np.zeros(S + 1, np.int32), out_cam=z, out_kp=z, out_src=z,
                    stats=np.zeros(4, np.int32))
    part = [i < n and (mask is None or int(mask[i]) >= 0) for i in range(S)]

    def valid(o):
        return 0 <= cam[o] < cam_stride and 0 <= kp[o] < kp_stride
    parent = list(range(S))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    owner = {}   # (cam, kp) -> a point holding it
    for i in range(n):
        if not part[i]:
            continue
        for o in range(offsets[i], offsets[i + 1]):
            if not valid(o):
                continue
            key = (int(cam[o]), int(kp[o]))
            if key in owner:
                a, b = find(owner[key]), find(i)
                if a != b:
                    parent[max(a, b)] = min(a, b)   # the root of a class is its smallest index
            else:
                owner[key] = i
    fuse_to = np.arange(S, dtype=np.int32)
    members = {}
    for i in range(n):
        if part[i]:
            fuse_to[i] = find(i)
            members.setdefault(int(fuse_to[i]), []).append(i)
        else:
            fuse_to[i] = -1
    out_offsets = np.zeros(S + 1, np.int32)
    oc, ok, osrc = [], [], []
    for i in range(n):
        out_offsets[i] = len(oc)
        if part[i] and fuse_to[i] == i:
            seen = []
            for m in members[i]:              # ascending index
                for o in range(offsets[m], offsets[m + 1]):   # input order
                    if not valid(o):
                        continue
                    key = (int(cam[o]), int(kp[o]))
                    if key in seen:
                        continue
                    seen.append(key)
                    oc.append(key[0]); ok.append(key[1]); osrc.append(o)
    out_offsets[n:] = len(oc)
    stats = np.array([sum(part), sum(1 for m in members.values() if len(m) > 1), sum(len(m) - 1 for m in members.values()), len(oc)], np.int32)
    return dict(fuse_to=fuse_to, out_offsets=out_offsets, out_cam=np.array(oc, np.int32), out_kp=np.array(ok, np.int32),
                out_src=np.array(osrc, np.int32), stats=stats)


def fuse_second(n_points, offsets, cam, kp, cam_stride, kp_stride, mask=None):
    """The same outputs from an explicit link graph (every pair of points taking part that share a valid (cam, kp)), a breadth-first
    search from every unvisited point in ascending order, and a set for the kept entries."""
    from collections import deque
    offsets = np.asarray(offsets, np.int64)
    cam, kp = np.asarray(cam, np.int64), np.asarray(kp, np.int64)
    S, O = len(offsets) - 1, len(cam)
    n = min(max(int(n_points), 0), S)
    if not (offsets[0] >= 0 and (np.diff(offsets[:n + 1]) >= 0).all() and (offsets[:n + 1] <= O).all()):
        z = np.zeros(0, np.int32)
        return dict(fuse_to=np.arange(S, dtype=np.int32), out_offsets=np.zeros(S + 1, np.int32), out_cam=z, out_kp=z, out_src=z,
                    stats=np.zeros(4, np.int32))
    part = np.zeros(S, bool)
    part[:n] = True if mask is None else np.asarray(mask)[:n] >= 0
    ok_row = (cam >= 0) & (cam < cam_stride) & (kp >= 0) & (kp < kp_stride)
    holders = {}
    for i in np.flatnonzero(part):
        for o in range(offsets[i], offsets[i + 1]):
            if ok_row[o]:
                holders.setdefault((int(cam[o]), int(kp[o])), set()).add(int(i))
    adj = {int(i): set() for i in np.flatnonzero(part)}
    for hs in holders.values():
        hs = sorted(hs)
        for a in hs[1:]:            # a star is enough for connectivity
            adj[hs[0]].add(a)
            adj[a].add(hs[0])
    fuse_to = np.where(np.arange(S) < n, -1, np.arange(S)).astype(np.int32)
    groups = []
    for i in sorted(adj):
        if fuse_to[i] >= 0:
            continue
        comp, q = [], deque([i])
        fuse_to[i] = i
        while q:
            a = q.popleft()
            comp.append(a)
            for b_ in adj[a]:
                if fuse_to[b_] < 0:
                    fuse_to[b_] = i
                    q.append(b_)
        groups.append(sorted(comp))
    rows = {}
    for g in groups:
        seen, row = set(), []
        for m in g:
            for o in range(offsets[m], offsets[m + 1]):
                key = (int(cam[o]), int(kp[o]))
                if ok_row[o] and key not in seen:
                    seen.add(key)
                    row.append((key[0], key[1], o))
        rows[g[0]] = row
    out_offsets = np.zeros(S + 1, np.int32)
    flat = []
    for i in range(n):
        out_offsets[i] = len(flat)
        flat += rows.get(i, [])
    out_offsets[n:] = len(flat)
    arr = np.array(flat, np.int32).reshape(-1, 3)
    stats = np.array([int(part.sum()), sum(len(g) > 1 for g in groups), sum(len(g) - 1 for g in groups), len(flat)], np.int32)
    return dict(fuse_to=fuse_to, out_offsets=out_offsets, out_cam=arr[:, 0].copy(), out_kp=arr[:, 1].copy(), out_src=arr[:, 2].copy(), stats=stats)


FUSE_OUTS = ("fuse_to", "out_offsets", "out_cam", "out_kp", "out_src", "stats")


def fuse_batch(n_points, offsets, cam, kp, cam_stride, kp_stride, mask=None, prefill=None):
    """n_points (B,), offsets (B, S + 1), cam / kp (B, O), mask (B, S) or None -> the arrays vslam_fuse_points writes, over `prefill`
    (a dict of the caller's output arrays; zeros when None): slots past an item's total keep the prefill"""
    B, S, O = offsets.shape[0], offsets.shape[1] - 1, cam.shape[1]
    shapes = dict(fuse_to=(B, S), out_offsets=(B, S + 1), out_cam=(B, O), out_kp=(B, O), out_src=(B, O), stats=(B, 4))
    out = {k: (np.zeros(s, np.int32) if prefill is None or k not in prefill else np.array(prefill[k], np.int32).reshape(s)) for k, s in shapes.items()}
    for b in range(B):
        r = fuse_item(n_points[b], offsets[b], cam[b], kp[b], cam_stride, kp_stride, None if mask is None else mask[b])
        t = len(r["out_cam"])
        out["fuse_to"][b], out["out_offsets"][b], out["stats"][b] = r["fuse_to"], r["out_offsets"], r["stats"]
        for k in ("out_cam", "out_kp", "out_src"):
            out[k][b, :t] = r[k]
    return out


# ------------------------------------------------------------------------------------------------ the cull
def cull_item(points, n_points, offsets, cam, kp, R, T, n_cams, xy, K, **kw):
    """points (S, 4) f32, offsets (S + 1,), cam / kp (O,), R (Cs, 9) / T (Cs, 3) f64, xy (Cs, Kp, 2) f32, K 3 x 3 f32 -> dict(keep (S,),
    counts (S, 2), stats (4,)), int32"""
    p = cull_params(**kw)
    points = np.asarray(points, np.float32).reshape(-1, 4)
    offsets = np.asarray(offsets, np.int64)
    cam, kp = np.asarray(cam, np.int64), np.asarray(kp, np.int64)
    R, T = np.asarray(R, f64).reshape(-1, 9), np.asarray(T, f64).reshape(-1, 3)
    xy = np.asarray(xy, np.float32)
    Kd = np.asarray(K, np.float32).astype(f64).reshape(9)
    S, O, Cs, Kp = len(points), len(cam), len(R), xy.shape[1]
    n = min(max(int(n_points), 0), S)
    C = min(max(int(n_cams), 0), Cs)
    r = f64(p["inlier_px"])
    r2 = r * r
    cam_ok = np.isfinite(R).all(1) & np.isfinite(T).all(1)
    keep = np.full(S, -1, np.int32)
    counts = np.zeros((S, 2), np.int32)
    for i in range(n):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if not (0 <= o0 < o1 <= O) or not np.isfinite(points[i, :3]).all():
            continue
        P = points[i:i + 1, :3].astype(f64)
        n_usable = n_good = 0
        last = -1
        for o in range(o0, o1):
            c, k = int(cam[o]), int(kp[o])
            if not (0 <= c < C and 0 <= k < Kp) or not cam_ok[c] or not np.isfinite(xy[c, k]).all():
                continue
            n_usable += 1
            last = max(last, c)
            with np.errstate(all="ignore"):
                _, Y = rr.transform(R[c], T[c], P)
                if not Y[0, 2] > 0.0:
                    continue
                u, v, _ = rr.project(Kd, Y)
                if not (np.isfinite(u[0]) and np.isfinite(v[0])):
                    continue
                r0, r1 = u[0] - f64(xy[c, k, 0]), v[0] - f64(xy[c, k, 1])
                n_good += bool(r0 * r0 + r1 * r1 <= r2)
        need = p["mature_good"] if last + p["mature_age"] < C else p["min_good"]
        keep[i] = 1 if (n_good >= need and 10 * n_good >= p["good10"] * n_usable) else 0
        counts[i] = n_usable, n_good
    part = keep >= 0
    stats = np.array([part.sum(), (keep == 1).sum(), (keep == 0).sum(), counts[part, 1].sum()], np.int32)
    return dict(keep=keep, counts=counts, stats=stats)


CULL_OUTS = ("keep", "counts", "stats")


def cull_batch(points, n_points, offsets, cam, kp, R, T, n_cams, xy, K, **kw):
    rs = [cull_item(points[b], n_points[b], offsets[b], cam[b], kp[b], R[b], T[b], n_cams[b], xy[b], K, **kw) for b in range(len(points))]
    return {k: np.stack([r[k] for r in rs]) for k in CULL_OUTS}


# ------------------------------------------------------------------------------------------------ on the world
def cameras(Twc, frames):
    """include/vslam_adjust.h, "camera c", for frames 0 .. frames - 1 of one track: Twc (max_frames, 16) -> R (max_frames, 9), T
    (max_frames, 3); rows from `frames` on are zero"""
    Fr = len(Twc)
    R, T = np.zeros((Fr, 9)), np.zeros((Fr, 3))
    for f in range(frames):
        M = Twc[f]
        for r in range(3):
            for c in range(3):
                R[f, 3 * r + c] = M[4 * c + r]
            T[f, r] = -((M[r] * M[3] + M[4 + r] * M[7]) + M[8 + r] * M[11])
    return R, T


def nan_rows(world_points, rows):
    w = np.array(world_points, np.float32)
    bits = w.view(np.uint32)
    bits[rows, :3] = QNAN_BITS
    bits[rows, 3] = 0
    return w


def world_fuse(fuse_to, world_points, size, offsets, frame, kp, max_frames, kp_stride):
    """One track of vslam_world_fuse: fuse_to (P,) before the call, the map's own CSR -> (the item's result, fuse_to after, world_points
    after)"""
    r = fuse_item(size, offsets, frame, kp, max_frames, kp_stride, fuse_to)
    new = r["fuse_to"]
    idx = np.arange(len(new))
    newly = (new >= 0) & (new != idx) & (np.asarray(fuse_to) == idx)
    return r, new.copy(), nan_rows(world_points, np.flatnonzero(newly))


def world_cull_apply(fuse_to, world_points, keep):
    """One track of vslam_world_cull behind the cull itself: keep (P,) -> fuse_to after, world_points after"""
    f = np.array(fuse_to, np.int32)
    culled = np.flatnonzero(np.asarray(keep) == 0)
    out = f.copy()
    out[culled] = -1
    for i in range(len(f)):
        if f[i] >= 0 and f[i] != i and keep[f[i]] == 0:
            out[i] = -1
    return out, nan_rows(world_points, culled)


# ------------------------------------------------------------------------------------------------ random items
def random_fuse_item(seed, n, cam_stride=6, kp_stride=64, obs=(1, 3), S=None, junk=0.05, masked=0.05):
    """n points of obs[0] .. obs[1] observations over a cam_stride x kp_stride table small enough that cells are shared often; a share
    of entries with cam or kp out of range, some rows repeated inside a point, a share of the points masked; rows past n junk"""
    rng = np.random.default_rng(seed)
    S = S or n
    counts = rng.integers(obs[0], obs[1] + 1, S)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    O = max(int(offsets[-1]), 1)
    cam = rng.integers(0, cam_stride, O).astype(np.int32)
    kp = rng.integers(0, kp_stride, O).astype(np.int32)
    bad = rng.uniform(size=O) < junk
    cam[bad & (rng.uniform(size=O) < 0.5)] = rng.choice([-1, cam_stride, cam_stride + 7])
    kp[bad & (cam >= 0) & (cam < cam_stride)] = rng.choice([-3, kp_stride, 1 << 20])
    for i in np.flatnonzero(counts >= 2)[::5]:
        cam[offsets[i] + 1], kp[offsets[i] + 1] = cam[offsets[i]], kp[offsets[i]]   # a duplicate inside one row
    mask = np.where(rng.uniform(size=S) < masked, -1, rng.integers(0, 50, S)).astype(np.int32)
    return dict(n=n, offsets=offsets, cam=cam, kp=kp, cam_stride=cam_stride, kp_stride=kp_stride, mask=mask)


def batch_fuse(items):
    """items of different sizes padded into one batch: the strides are the largest; padding rows are junk that n keeps out"""
    S = max(len(it["offsets"]) - 1 for it in items)
    O = max(len(it["cam"]) for it in items)
    B = len(items)
    offsets = np.zeros((B, S + 1), np.int32)
    cam, kp = np.full((B, O), 3, np.int32), np.full((B, O), 5, np.int32)
    mask = np.zeros((B, S), np.int32)
    for b, it in enumerate(items):
        s, o = len(it["offsets"]) - 1, len(it["cam"])
        offsets[b, :s + 1] = it["offsets"]
        offsets[b, s + 1:] = -7
        cam[b, :o], kp[b, :o] = it["cam"], it["kp"]
        mask[b, :s] = it["mask"] if it.get("mask") is not None else 0
    return dict(n=np.array([it["n"] for it in items], np.int32), offsets=offsets, cam=cam, kp=kp, mask=mask)


def random_cull_item(seed, n, n_cams, obs=(1, 8), kp_stride=96, cam_stride=None, S=None):
    """n points in front of n_cams cameras on a line, every observation the exact projection rounded to f32 plus, for a third of
    them, 2 to 12 pixels of error (so that both sides of the disc and of both count rules occur); a few non-finite points, cameras
    and keypoints, a few entries out of range, a few empty rows"""
    rng = np.random.default_rng(seed)
    S, Cs = S or n, cam_stride or n_cams
    K = rr.kmat()
    Kd = K.astype(f64)
    R, T = np.zeros((Cs, 9)), np.zeros((Cs, 3))
    for c in range(Cs):
        w = rng.normal(0, 0.03, 3)
        th = np.linalg.norm(w)
        k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R[c] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).reshape(9)
        T[c] = [-0.05 * c, rng.normal(0, 0.02), rng.normal(0, 0.02)]
    if Cs > 3:
        R[Cs // 2, 4] = np.nan
    points = np.ones((S, 4), np.float32)
    points[:, :2] = rng.uniform(-1.5, 1.5, (S, 2))
    points[:, 2] = rng.uniform(4, 9, S)
    for i in rng.integers(0, max(n, 1), 3):
        points[i, rng.integers(0, 3)] = [np.nan, np.inf, -np.inf][rng.integers(0, 3)]
    points[rng.integers(0, max(n, 1)), 2] = -5.0            # behind every camera
    counts = rng.integers(obs[0], obs[1] + 1, S)
    counts[rng.uniform(size=S) < 0.03] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    O = max(int(offsets[-1]), 1)
    owner = np.repeat(np.arange(S), counts)
    cam = rng.integers(0, n_cams, O).astype(np.int32)
    kp = rng.integers(0, kp_stride, O).astype(np.int32)
    xy = rng.uniform(0, 640, (Cs, kp_stride, 2)).astype(np.float32)
    with np.errstate(all="ignore"):
        for o in range(len(owner)):                           # a later entry of a (cam, kp) overwrites an earlier one: more misses
            P = points[owner[o], :3].astype(f64)
            Y = R[cam[o]].reshape(3, 3) @ P + T[cam[o]]
            q = Kd @ Y
            uv = q[:2] / q[2]
            if rng.uniform() < 0.33:
                a = rng.uniform(0, 2 * np.pi)
                uv = uv + rng.uniform(2, 12) * np.array([np.cos(a), np.sin(a)])
            xy[cam[o], kp[o]] = uv.astype(np.float32)
    xy[0, 3] = np.nan
    bad = rng.uniform(size=O) < 0.03
    cam[bad] = rng.choice([-1, n_cams, Cs + 3])
    kp[rng.uniform(size=O) < 0.02] = kp_stride
    return dict(points=points, n=n, offsets=offsets, cam=cam, kp=kp, R=R, T=T, n_cams=n_cams, xy=xy, K=K)
