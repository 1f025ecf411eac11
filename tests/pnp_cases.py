"""What the tests of vslam_pnp_ransac share: the hand cases, and the serial program (tests/native/pnp_serial.cpp) built once with
the sanitizers and run over a list of cases.  A case: dict(points (S, 3) f64, xy (S, 2) f32, n, K, seed, R0 (9,), T0 (3,), params
{hypotheses, min_inliers, inlier_px}, polish None or {vslam_resect_params fields})."""
import os
import struct
import subprocess

import numpy as np

import ref_pnp as rp
import ref_resect as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP_R = np.array([0.5, -1.5, 2.5, 3.5, -4.5, 5.5, 6.5, 7.5, -8.5])   # no rotation: an item left alone keeps these bits
KEEP_T = np.array([11.25, -12.5, 13.75])


def build_serial(tmpdir):
    out = os.path.join(str(tmpdir), "pnp_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "pnp_serial.cpp")], check=True)
    return out


def case(sc, seed=1, polish=None, n=None, pad=0, **params):
    """a planted scene (ref_pnp.planted) as a case; pad rows of NaN behind the n given"""
    P, xy = np.asarray(sc["points"], np.float64), np.asarray(sc["xy"], np.float32)
    if pad:
        P = np.concatenate([P, np.full((pad, 3), np.nan)])
        xy = np.concatenate([xy, np.full((pad, 2), np.nan, np.float32)])
    return dict(points=P, xy=xy, n=len(sc["points"]) if n is None else n, K=sc.get("K", rr.kmat()), seed=seed, R0=KEEP_R, T0=KEEP_T,
                params=rp.params(**params), polish=None if polish is None else rr.params(**polish), scene=sc)


def run_serial(exe, tmpdir, cases):
    src, dst = os.path.join(str(tmpdir), "pnp_in.bin"), os.path.join(str(tmpdir), "pnp_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            p, q = c["params"], c["polish"] or rr.params()
            S = len(c["points"])
            f.write(struct.pack("8i", S, int(c["n"]), p["hypotheses"], p["min_inliers"], 0 if c["polish"] is None else 1,
                                q["max_iterations"], q["rounds"], q["min_links"]))
            f.write(struct.pack("I", c["seed"] & 0xFFFFFFFF))
            f.write(struct.pack("3d", p["inlier_px"], q["huber_px"], q["gate_px"]))
            for a, dt in ((c["K"], np.float32), (c["R0"], np.float64), (c["T0"], np.float64), (c["points"], np.float64),
                          (c["xy"], np.float32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
    subprocess.run([exe, src, dst], check=True)
    buf = open(dst, "rb").read()
    pos, out = 0, []

    def take(n, dt):
        nonlocal pos
        a = np.frombuffer(buf, dt, n, pos)
        pos += a.nbytes
        return a
    for c in cases:
        S, H = len(c["points"]), c["params"]["hypotheses"]
        r = dict(counts=take(4 * H, np.int32).reshape(H, 4))
        r["winner"], r["n_inliers"] = (int(v) for v in take(2, np.int32))
        r.update(inlier=take(S, np.int32), corr_index=take(r["n_inliers"], np.int32), R_raw=take(9, np.float64), T_raw=take(3, np.float64),
                 R=take(9, np.float64), T=take(3, np.float64), stats=take(4, np.float64))
        out.append(r)
    assert pos == len(buf)
    return out


def reference(c, plant=None):
    return rp.pnp_ransac(c["points"], c["xy"], c["n"], c["K"], c["seed"], c["R0"], c["T0"], polish=c["polish"], plant=plant, **c["params"])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def hand_cases():
    """name -> (case, found expected)"""
    rng = np.random.default_rng(5)
    out = {}
    sc = rp.planted(40, 0.5, 3)
    out["n3"] = (case(sc, n=3), False)
    out["n4_all_exact"] = (case(rp.planted(4, 0.0, 1), min_inliers=4), True)
    out["below_min_inliers"] = (case(sc, min_inliers=int(sc["planted"].sum()) + 1), False)
    out["at_min_inliers"] = (case(sc, min_inliers=int(sc["planted"].sum())), True)
    for name, (row, col) in dict(nan_point=(5, 1), inf_point=(0, 2)).items():
        c = case(sc)
        c["points"] = c["points"].copy()
        c["points"][row, col] = np.nan if "nan" in name else np.inf
        out[name] = (c, False)
    c = case(sc)
    c["xy"] = c["xy"].copy()
    c["xy"][7, 0] = np.nan
    out["nan_keypoint"] = (c, False)
    c = case(sc)
    c["K"] = c["K"].copy()
    c["K"][0, 0] = np.inf
    out["inf_K"] = (c, False)
    out["nan_rows_past_n"] = (case(sc, pad=9), True)
    line = rp.planted(40, 0.0, 4)
    t = rng.uniform(-2, 2, 40)
    line["points"] = np.array([0.3, -0.2, 5.0])[None, :] + t[:, None] * np.array([1.0, 0.5, 0.25])[None, :]
    out["collinear"] = (case(line), False)
    same = rp.planted(40, 0.0, 4)
    same["points"] = np.repeat(same["points"][:1], 40, 0)
    out["one_point_repeated"] = (case(same), False)
    dup = rp.planted(20, 0.0, 6)
    dup = dict(dup, points=np.repeat(dup["points"], 2, 0), xy=np.repeat(dup["xy"], 2, 0), planted=np.ones(40, bool))
    out["every_point_twice"] = (case(dup), True)
    out["planar"] = (case(rp.planted(60, 0.5, 2, planar=True)), True)
    for n in (3, 4, 5):   # the 16-draw cap: small n repeats indices often
        out[f"draw_cap_n{n}"] = (case(rp.planted(n, 0.0, 2), min_inliers=4, hypotheses=64), n >= 4)
    return out


_PLANTED = {}


def planted_config(k):
    """configuration k of ref_pnp.CONFIGS on ref_pnp.SEEDS, polished (min_links = 6 where six are planted): [(case, reference
    result)], computed once per process"""
    if k not in _PLANTED:
        n, share, hyp, min_in = rp.CONFIGS[k]
        cases = [case(rp.planted(n, share, s), seed=s, polish=dict(min_links=min(min_in, 8)), hypotheses=hyp, min_inliers=min_in)
                 for s in rp.SEEDS]
        _PLANTED[k] = [(c, reference(c)) for c in cases]
    return _PLANTED[k]


def match_case(seed, n_points, obs_range, n_kp, planted=0.6, taken=False, pad_points=0, pad_kp=0):
    """One item of vslam_match_points: every point has a descriptor of its own and obs_range = (lo, hi) observations of it with a
    few bits flipped; `planted` of the keypoints are noisy copies of a point's descriptor -- some points get two such keypoints, so
    ties and ratio rejections occur, and every ninth point shares its descriptor with its neighbour, so keypoints are contested --,
    the rest random.  A few points have an empty CSR
    row, an inverted one or a non-finite coordinate; taken marks a tenth of the keypoints.  pad_*: rows past n filled with junk."""
    rng = np.random.default_rng(seed)
    S, Kp = n_points + pad_points, max(n_kp + pad_kp, 1)
    base = rng.integers(0, 256, (max(n_points, 1), 32), dtype=np.uint8)
    base[5::9] = base[4::9][:len(base[5::9])]            # two points with one descriptor: both want the same keypoint

    def noisy(d, flips):
        d = d.copy()
        for row in d:
            for bit in rng.integers(0, 256, rng.integers(0, flips + 1)):
                row[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return d
    counts = rng.integers(obs_range[0], obs_range[1] + 1, S)
    counts[rng.uniform(size=S) < 0.03] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs_desc = np.zeros((max(int(counts.sum()), 1), 32), np.uint8)
    owner = np.repeat(np.arange(S), counts)
    live = owner < n_points
    obs_desc[:len(owner)][live] = noisy(base[owner[live]], 6)
    points = np.ones((S, 4), np.float32)
    points[:, :3] = rng.uniform(-5, 5, (S, 3))
    for i in rng.integers(0, max(n_points, 1), 3):
        points[i, rng.integers(0, 3)] = [np.nan, np.inf, -np.inf][rng.integers(0, 3)]
    if n_points > 10:
        offsets[7] = offsets[8] + 1 if offsets[8] + 1 <= offsets[9] else offsets[7]   # an inverted row for point 6 .. 7
    xy = rng.uniform(0, 640, (Kp, 2)).astype(np.float32)
    desc = rng.integers(0, 256, (Kp, 32), dtype=np.uint8)
    if n_points:
        k_planted = rng.permutation(n_kp)[:int(planted * n_kp)]
        who = rng.integers(0, n_points, len(k_planted))
        who[::7] = who[1::7][:len(who[::7])] if len(who) > 8 else who[::7]          # the same point behind two keypoints
        desc[k_planted] = noisy(base[who], 10)
        same = k_planted[::11]
        desc[same] = base[who[::11]]                                                  # exact copies: d = 0 ties
    tk = None
    if taken:
        tk = np.full(Kp, -1, np.int32)
        tk[rng.permutation(Kp)[:Kp // 10]] = rng.integers(0, 100, Kp // 10)
    return dict(points=points, n_points=n_points, offsets=offsets, obs_desc=obs_desc, xy=xy, desc=desc, n_kp=n_kp, taken=tk)


def match_reference(c, **params):
    return rp.match_points(c["points"], c["n_points"], c["offsets"], c["obs_desc"], c["xy"], c["desc"], c["n_kp"], c["taken"], **params)


# ------------------------------------------------------------------------------------------------ ref_world.scene through the map
SCENE_W, SCENE_H = 1280, 720
SCENE_K = np.array([[525, 0, SCENE_W // 2], [0, 525, SCENE_H // 2], [0, 0, 1]], np.float32)


def world_scene(seed, points, frames=6):
    """ref_world.scene(seed, points, frames) as what a map step takes, or None when the front end cannot be fed with it: the pose
    stage returns t with t_z >= 0 (the reference's rule), so every pair must move with t_z > 0.1, and every point must project
    inside the SCENE_W x SCENE_H image in every frame.  Camera f: orientation chained from the pairs' f32 R (made orthonormal), the
    scene's own centre; keypoints are the exact projections rounded to f32 at the scene's per-frame permutation (rebuilt from the
    pairs' matches; points in no pair of a frame take the free indices), descriptors one random row per point, the same in every
    frame; per pair the exact F of the motion and every match of the scene.
    -> dict(scene, Rwc [frames], xy [frames](n, 2) f32, desc [frames](n, 32) u8, perm [frames], pairs [dict(matches, F)])"""
    import ref_world as rw
    from test_oracle_pose import true_F
    sc = rw.scene(seed, points=points, frames=frames)
    if any(p["t"][2] <= 0.1 for p in sc["pairs"]):
        return None
    n, Kd = sc["n"], SCENE_K.astype(np.float64)
    Rwc = [np.eye(3)]
    for p in sc["pairs"]:
        U, _, Vt = np.linalg.svd(Rwc[-1] @ p["R"].astype(np.float64).reshape(3, 3).T)
        Rwc.append(U @ Vt)
    perm = [np.full(n, -1, np.int64) for _ in range(frames)]
    for f, p in enumerate(sc["pairs"], 1):
        perm[f - 1][p["ids"]] = p["matches"][:, 0]
        perm[f][p["ids"]] = p["matches"][:, 1]
    for q in perm:
        free = np.setdiff1d(np.arange(n), q[q >= 0])
        q[q < 0] = free
        assert np.array_equal(np.sort(q), np.arange(n))
    rng = np.random.default_rng(7000 + seed)
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    xy, desc = [], []
    for f in range(frames):
        Y = (sc["points"] - sc["centres"][f]) @ Rwc[f]
        q = Y @ Kd.T
        uv = q[:, :2] / q[:, 2:]
        if not ((Y[:, 2] > 1.0).all() and (uv > 8).all() and (uv[:, 0] < SCENE_W - 8).all() and (uv[:, 1] < SCENE_H - 8).all()):
            return None
        a, d = np.zeros((n, 2), np.float32), np.zeros((n, 32), np.uint8)
        a[perm[f]], d[perm[f]] = uv.astype(np.float32), base
        xy.append(a)
        desc.append(d)
    pairs = []
    for f, p in enumerate(sc["pairs"], 1):
        Rrel = Rwc[f].T @ Rwc[f - 1]
        trel = Rwc[f].T @ (sc["centres"][f - 1] - sc["centres"][f])
        pairs.append(dict(matches=p["matches"], F=true_F(SCENE_K, Rrel, trel).reshape(9)))
    return dict(scene=sc, Rwc=Rwc, xy=xy, desc=desc, perm=perm, pairs=pairs, n=n)


def first_world_scene(points, frames=6, seeds=range(4000)):
    for seed in seeds:
        ws = world_scene(seed, points, frames)
        if ws is not None:
            return seed, ws
    raise AssertionError("no seed of ref_world.scene moves forward in every pair inside the image")
