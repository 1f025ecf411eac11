"""What the tests of vslam_sim3_ransac / vslam_sim3_refine share: the hand cases, and the serial program (tests/native/sim3_serial.cpp)
built once with the sanitizers and run over a list of cases.  A case: dict(A, B (S, 3) f64, xa, xb (S, 2) f32, n, K, seed, keep (s, R
(9,), t (3,)), params {hypotheses, min_inliers, inlier_px}, polish None or {vslam_resect_params fields}, mode 0 (the RANSAC) or 1
(the refinement alone, from `keep` over `mask`), mask (S,) int32)."""
import os
import struct
import subprocess

import numpy as np

import ref_resect as rr
import ref_sim3 as r3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP_S = 7.25   # no similarity: an item left alone keeps these bits
KEEP_R = np.array([0.5, -1.5, 2.5, 3.5, -4.5, 5.5, 6.5, 7.5, -8.5])
KEEP_T = np.array([11.25, -12.5, 13.75])


def build_serial(tmpdir):
    out = os.path.join(str(tmpdir), "sim3_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "sim3_serial.cpp")], check=True)
    return out


def case(sc, seed=1, polish=None, n=None, pad=0, **params):
    """a planted scene (ref_sim3.planted) as a case; pad rows of NaN behind the n given"""
    A, B = np.asarray(sc["A"], np.float64), np.asarray(sc["B"], np.float64)
    xa, xb = np.asarray(sc["xa"], np.float32), np.asarray(sc["xb"], np.float32)
    if pad:
        A, B = (np.concatenate([v, np.full((pad, 3), np.nan)]) for v in (A, B))
        xa, xb = (np.concatenate([v, np.full((pad, 2), np.nan, np.float32)]) for v in (xa, xb))
    return dict(A=A, B=B, xa=xa, xb=xb, n=len(sc["A"]) if n is None else n, K=sc.get("K", rr.kmat()), seed=seed, keep=(KEEP_S, KEEP_R, KEEP_T),
                params=r3.params(**params), polish=None if polish is None else rr.params(**polish), mode=0, mask=np.ones(len(A), np.int32),
                scene=sc)


def refine_case(rows, K, start, mask=None, **polish):
    """the refinement alone: rows = (A, xa, B, xb), start = (s, R, t)"""
    A, xa, B, xb = rows
    return dict(A=np.asarray(A, np.float64), B=np.asarray(B, np.float64), xa=np.asarray(xa, np.float32), xb=np.asarray(xb, np.float32), n=len(A),
                K=K, seed=0, keep=start, params=r3.params(), polish=rr.params(**polish), mode=1,
                mask=np.ones(len(A), np.int32) if mask is None else np.asarray(mask, np.int32))


def run_serial(exe, tmpdir, cases):
    src, dst = os.path.join(str(tmpdir), "sim3_in.bin"), os.path.join(str(tmpdir), "sim3_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            p, q = c["params"], c["polish"] or rr.params()
            f.write(struct.pack("9i", len(c["A"]), int(c["n"]), p["hypotheses"], p["min_inliers"], 0 if c["polish"] is None else 1,
                                q["max_iterations"], q["rounds"], q["min_links"], c["mode"]))
            f.write(struct.pack("I", c["seed"] & 0xFFFFFFFF))
            f.write(struct.pack("3d", p["inlier_px"], q["huber_px"], q["gate_px"]))
            s, R, t = c["keep"]
            for a, dt in ((c["K"], np.float32), ([s], np.float64), (R, np.float64), (t, np.float64), (c["A"], np.float64), (c["B"], np.float64),
                          (c["xa"], np.float32), (c["xb"], np.float32), (c["mask"], np.int32)):
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
        S, H = len(c["A"]), c["params"]["hypotheses"]
        r = dict(sets=take(3 * H, np.int32).reshape(H, 3), models=take(37 * H, np.float64).reshape(H, 37), counts=take(H, np.int32))
        r["winner"], r["n_inliers"] = (int(v) for v in take(2, np.int32))
        r.update(inlier=take(S, np.int32), corr_index=take(r["n_inliers"], np.int32))
        for tag in ("_raw", ""):
            r["s" + tag], r["R" + tag], r["t" + tag] = float(take(1, np.float64)[0]), take(9, np.float64), take(3, np.float64)
        r["stats"] = take(4, np.float64)
        out.append(r)
    assert pos == len(buf)
    return out


def reference(c, plant=None):
    if c["mode"] == 1:
        s, R, t, stats, info = r3.refine(c["A"], c["xa"], c["B"], c["xb"], c["n"], c["mask"], c["K"], *c["keep"], plant=plant, **c["polish"])
        return dict(s=s, R=R, t=t, stats=stats, info=info)
    return r3.sim3_ransac(c["A"], c["xa"], c["B"], c["xb"], c["n"], c["K"], c["seed"], c["keep"], polish=c["polish"], plant=plant, **c["params"])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def hold_exact(name, got, ref, H):
    """the serial walk (or the device, in the same dict layout; `sets` / `models` only where present) against the reference, bit
    for bit: sets, models with M_a / M_b, every count, winner, mask, compaction, the unpolished (s, R, t)"""
    if "sets" in got:
        for h in range(H):
            assert list(got["sets"][h]) == (ref["sets"].get(h) or [-1, -1, -1]), (name, h)
    if "models" in got:
        for h in range(H):
            m = ref["models"].get(h)
            want = np.zeros(37) if m is None else np.concatenate([[m[0]], m[1], m[2], m[3], m[4]])
            assert same_bits(got["models"][h], want), (name, h)
    assert np.array_equal(got["counts"], ref["counts"]), name
    assert got["winner"] == ref["winner"] and (got["winner"] >= 0) == ref["found"], name
    assert got["n_inliers"] == ref["n_inliers"], name
    assert np.array_equal(got["inlier"], ref["inlier"]), name
    assert np.array_equal(got["corr_index"][:ref["n_inliers"]], ref["corr_index"]), name
    assert same_bits(got["s_raw"], ref["s_raw"]) and same_bits(got["R_raw"], ref["R_raw"]) and same_bits(got["t_raw"], ref["t_raw"]), name


def model_distance(a, b):
    """entry-wise between two results: s relative, R and t absolute"""
    return max(abs(a["s"] - b["s"]) / abs(b["s"]), float(np.abs(a["R"] - b["R"]).max()), float(np.abs(a["t"] - b["t"]).max()))


def behind_a_scene():
    """a planted scene without outliers whose pair 5 is consistent with the similarity (B = s R A + t, both pixels the exact
    projections) but lies BEHIND camera a while in front of camera b: direction b alone would take it"""
    for seed in range(200):
        sc = r3.planted(40, 0.0, seed)
        if sc["t"][2] / sc["s"] < 0.4:
            continue
        Kd = sc["K"].astype(np.float64)
        A = np.array([0.02, -0.03, -0.1])
        B = sc["s"] * (sc["R"].reshape(3, 3) @ A) + sc["t"]
        if B[2] <= 0.1 * sc["s"]:
            continue
        qa, qb = Kd @ A, Kd @ B
        sc["A"][5], sc["B"][5] = A, B
        sc["xa"][5], sc["xb"][5] = (qa[:2] / qa[2]).astype(np.float32), (qb[:2] / qb[2]).astype(np.float32)
        sc["planted"][5] = False
        return sc
    raise AssertionError("no seed with camera b far enough behind camera a")


def hand_cases():
    """name -> (case, found expected)"""
    rng = np.random.default_rng(5)
    out = {}
    sc = r3.planted(40, 0.5, 3)
    k = int(sc["planted"].sum())
    out["n3"] = (case(sc, n=3), False)
    out["n4_all_exact"] = (case(r3.planted(4, 0.0, 1), min_inliers=4), True)
    out["below_min_inliers"] = (case(sc, min_inliers=k + 1), False)
    out["at_min_inliers"] = (case(sc, min_inliers=k), True)
    for name, (key, row, col, val) in dict(nan_A=("A", 5, 1, np.nan), inf_B=("B", 0, 2, np.inf), nan_xa=("xa", 7, 0, np.nan),
                                           inf_xb=("xb", 39, 1, -np.inf)).items():
        c = case(sc)
        c[key] = c[key].copy()
        c[key][row, col] = val
        out[name] = (c, False)
    c = case(sc)
    c["K"] = c["K"].copy()
    c["K"][0, 0] = np.inf
    out["inf_K"] = (c, False)
    out["nan_rows_past_n"] = (case(sc, pad=9), True)
    line = r3.planted(40, 0.0, 4)
    tt = rng.uniform(-2, 2, 40)
    line["A"] = np.array([0.3, -0.2, 5.0])[None, :] + tt[:, None] * np.array([1.0, 0.5, 0.25])[None, :]
    out["collinear_A"] = (case(line), False)
    same = r3.planted(40, 0.0, 4)
    same["B"] = np.repeat(same["B"][:1], 40, 0)
    out["one_B_repeated"] = (case(same), False)
    dup = r3.planted(20, 0.0, 6)
    dup = dict(dup, **{k2: np.repeat(dup[k2], 2, 0) for k2 in ("A", "B", "xa", "xb")}, planted=np.ones(40, bool))
    out["every_pair_twice"] = (case(dup), True)
    out["all_exact_ties"] = (case(r3.planted(40, 0.0, 8), seed=8), True)
    out["behind_camera_a"] = (case(behind_a_scene(), seed=2), True)
    for n in (3, 4, 5):   # the 16-draw cap: small n repeats indices often
        out[f"draw_cap_n{n}"] = (case(r3.planted(n, 0.0, 2), min_inliers=4, hypotheses=64), n >= 4)
    return out


_PLANTED = {}


def planted_config(k):
    """configuration k of ref_sim3.CONFIGS on ref_sim3.SEEDS, polished (min_links = 6 where six are planted): [(case, reference
    result)], computed once per process"""
    if k not in _PLANTED:
        n, share, hyp, min_in = r3.CONFIGS[k]
        cases = [case(r3.planted(n, share, s), seed=s, polish=dict(min_links=min(min_in, 8)), hypotheses=hyp, min_inliers=min_in)
                 for s in r3.SEEDS]
        _PLANTED[k] = [(c, reference(c)) for c in cases]
    return _PLANTED[k]


# ------------------------------------------------------------------------------------------------ two tracks of one scene, in numpy
def ref_tracks(seed, points=60, frames=6, shift=1):
    """ref_world.scene(seed, points, frames + shift) seen by two tracks run through ref_world.World: track a records scene frames
    0 .. frames - 1, track b scene frames shift .. shift + frames - 1, so b's world has another origin, orientation and unit (its
    own first baseline).  Each track's "map": the points its pairs lift, in pair order (row = a point of ONE pair), and for frame
    f >= 1 the row that the pair (f - 1 -> f) lifted for each keypoint `second` (-1 elsewhere).  Keypoints are the exact projections
    with K = ref_resect.KVEC rounded to f32.
    -> dict(scene, tracks [a, b]: dict(world, Twc (F, 16), pose, scale, carry, carry_index, points (N, 4) f32, size, ids (F, n) row of
    each keypoint, truth (N,) the scene's point behind each row, first, g the track's unit in scene units, err / unit as
    ref_world.run_scene measures them), xy [scene frame] (n, 2) f32, perm)"""
    import ref_world as rw
    total = frames + shift
    sc = rw.scene(seed, points=points, frames=total)
    C, Rwc, perm = rr.truth_rotations(seed, points, total)
    Kd = rr.kmat().astype(np.float64)
    xy = []
    for f in range(total):
        q = ((sc["points"] - C[f]) @ Rwc[f]) @ Kd.T
        a = np.zeros((points, 2), np.float32)
        a[perm[f]] = (q[:, :2] / q[:, 2:3]).astype(np.float32)
        xy.append(a)
    tracks = []
    for first in (0, shift):
        sub = dict(points=(sc["points"] - C[first]) @ Rwc[first], centres=(C[first:first + frames] - C[first]) @ Rwc[first],
                   base=sc["base"][first:first + frames - 1], pairs=sc["pairs"][first:first + frames - 1], frames=frames, n=points)
        w, err, unit = rw.run_scene(sub)
        rows, truth, ids = [], [], np.full((frames, points), -1, np.int32)
        for f, p in enumerate(sub["pairs"], 1):
            out = np.zeros((len(p["X"]), 4), np.float32)
            w.lift(f, p["X"], 0, len(p["X"]), out)
            ids[f, p["matches"][:, 1]] = len(rows) + np.arange(len(out))
            rows.extend(out)
            truth.extend(p["ids"])
        Twc = np.stack(w.Twc)
        tracks.append(dict(world=w, Twc=Twc, pose=Twc.astype(np.float32), scale=np.array(w.scale, np.float64), carry=w.carry.copy(),
                           carry_index=np.where(w.valid, 0, -1).astype(np.int32), points=np.array(rows, np.float32), size=len(rows), ids=ids,
                           truth=np.array(truth), first=first, g=float(sub["base"][0]), err=err, unit=unit))
    return dict(scene=sc, tracks=tracks, xy=xy, perm=perm, n=points)


def ref_pair(rt, fa, fb):
    """frame fa of track a against frame fb of track b of ref_tracks(): -> (side_a, side_b, matches (m, 2), xy_a, xy_b): every scene point
    with a map point at both keypoints, in the order of the scene's points"""
    a, b = rt["tracks"]
    Fa, Fb = a["first"] + fa, b["first"] + fb
    ka, kb = rt["perm"][Fa], rt["perm"][Fb]
    keep = [j for j in range(rt["n"]) if a["ids"][fa, ka[j]] >= 0 and b["ids"][fb, kb[j]] >= 0]
    matches = np.array([(ka[j], kb[j]) for j in keep], np.int32).reshape(-1, 2)
    side = lambda t, f: dict(ids=t["ids"][f], points=t["points"], Twc=t["Twc"][f], fuse_to=None)
    return side(a, fa), side(b, fb), matches, rt["xy"][Fa], rt["xy"][Fb]
