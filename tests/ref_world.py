"""The world frame of the resident map (vslam_world_*), restated in plain numpy: the contract beside the text of
include/vslam_amd.h ("the world frame").  Everything is f64 (numpy scalars: one IEEE operation per Python operator, never
fused), every sum is written out left to right; no `@`, no `dot`, whose order is not ours.  f32 inputs are widened first.

One World is ONE track.  step() advances it by one frame from the pair's R (9,) f32, t (3,) f32, the compacted inlier matches
(n, 2) and the triangulated points X (n, >= 3) f32 in the LAST frame's camera coordinates and in the pair's own unit
(|t| = 1); lift() takes points of one pair to the world.

Rules (the numbers in brackets are the variants `plant=` swaps in, for the tests that show each error is caught):
  in range   0 <= first < min(n_last, kp_stride) and 0 <= second < min(n_cur, kp_stride); any other match is ignored.
  usable     Y = R X + t, row r = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r]; X and Y finite, X.z > 0 and Y.z > 0.
  link       in range, usable, carry[first] valid and q = |carry[first]|^2 / |X|^2 finite, |v|^2 = (x x + y y) + z z.  (q is
             finite unless a square overflows or |X|^2 underflows to 0; such a match carries on but does not vote.)
  scale      L links, L >= min_links: s = sqrt(q_(k)), k = (L - 1) // 2 in ascending order (the LOWER median) [upper_median];
             otherwise s = the previous s (1 before the first pair with a model).  links[f] = L, or -1 without a winner.
  pose       Twc_f = Twc_{f-1} * B, B = [R^t | -(s (R^t t))], (R^t t)_i = ((R[0][i] t0 + R[1][i] t1) + R[2][i] t2), the 4 x 4
             product P[r][c] = ((A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c]) + A[r][3] B[3][c], all four terms, row 3
             included [Rt_not_transposed: s (R t); wrong_side: B * Twc_{f-1}].  Nothing is re-orthonormalised.
  lift       X_w = xf(Twc_{f-1}, (s_f x, s_f y, s_f z)) rounded once to f32, w = 1; xf as in tests/ref_render.py:
             r_i = ((M[i][0] x + M[i][1] y) + M[i][2] z) + M[i][3].
  carry      keyed by `second` [carry_by_first: by `first`]: s_f Y for every in-range usable match, the HIGHER match index wins
             a keypoint; everything else invalid.  Without a winner: all invalid, pose and scale carried over.

Error against exact geometry (tests/test_ref_world.py, scenes(): 40 points, 6 frames, baselines 0.1 .. 0.4, R and t rounded to
f32, 80 % of the matches present per pair).  With u = 2^-23 (R, t and X arrive as f32: unit roundoff 2^-24 each, and a
point passes through about two of them per frame), the bound is  C * u * frames * max|X|  on every lifted point and camera
centre after one global scale (the first baseline).  Measured ratios error / (u * frames * max|X|), worst over points and
centres, for the committed seeds 1 .. 6:
    seed 1: 0.1145   2: 0.1456   3: 0.2110   4: 0.2188   5: 0.1325   6: 0.1123        (MEASURED_RATIOS below)
C_BOUND = 0.9 = 4 x the largest of them (0.2188 -> 0.875), rounded up; the four covers other seeds, not arithmetic (f64 adds
about 2^-52 per operation).  In absolute terms the worst error is 1.4e-6 at max|X| = 9 and a first baseline of 0.1 .. 0.4.

The device is held to this file BIT FOR BIT, including s: the f64 sqrt of gfx950 (v_sqrt_f64 refined by the device library)
is correctly rounded, as numpy's is; tests/test_gpu_world.py checks that on thousands of values.
"""
import numpy as np

f64 = np.float64



def _w(a):
    return np.asarray(a, np.float32).astype(np.float64)


def norm2(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def xf(M, p):
    """rows 0..2 of a row-major 4 x 4 (flat 16) applied to a 3-vector"""
    return np.array([((M[4 * i] * p[0] + M[4 * i + 1] * p[1]) + M[4 * i + 2] * p[2]) + M[4 * i + 3] for i in range(3)], f64)


def mul4(A, B):
    P = np.empty(16, f64)
    for r in range(4):
        for c in range(4):
            P[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c]
    return P


def lower_median(q):
    s = sorted(float(x) for x in q)
    return f64(s[(len(s) - 1) // 2])


class World:
    def __init__(self, kp_stride, min_links=8, plant=None):
        self.K, self.min_links, self.plant = int(kp_stride), int(min_links), plant
        self.reset()

    def reset(self):
        self.Twc = [np.eye(4, dtype=f64).reshape(16)]
        self.scale = [f64(1.0)]
        self.links = [0]
        self.carry = np.zeros((self.K, 3), f64)
        self.valid = np.zeros(self.K, bool)

    @property
    def frames(self):
        return len(self.Twc)

    def pose32(self):
        return np.stack(self.Twc).astype(np.float32)

    def step(self, matches, X, R, t, n_last, n_cur, winner=True):
        """winner=False: a pair without a model (d_best[.][0] < 0); the other arguments are then not read."""
        K = self.K
        s_prev, T_prev = self.scale[-1], self.Twc[-1]
        new_carry, new_valid = np.zeros((K, 3), f64), np.zeros(K, bool)
        if not winner:
            self.Twc.append(T_prev.copy()); self.scale.append(s_prev); self.links.append(-1)
            self.carry, self.valid = new_carry, new_valid
            return
        R, t = _w(R).reshape(9), _w(t).reshape(3)
        matches = np.asarray(matches, np.int64).reshape(-1, 2)[:K]
        X = _w(X).reshape(len(np.asarray(X)), -1)[:K, :3] if len(matches) else np.zeros((0, 3))
        nl, nc = min(int(n_last), K), min(int(n_cur), K)
        use, Ys, qs = [], [], []
        with np.errstate(all="ignore"):
            for m, (a, b) in enumerate(matches):
                x = X[m]
                Y = np.array([((R[3 * r] * x[0] + R[3 * r + 1] * x[1]) + R[3 * r + 2] * x[2]) + t[r] for r in range(3)], f64)
                ok = 0 <= a < nl and 0 <= b < nc and bool(np.isfinite(x).all() and np.isfinite(Y).all() and x[2] > 0 and Y[2] > 0)
                use.append(ok); Ys.append(Y)
                if ok and self.valid[a]:
                    q = norm2(self.carry[a]) / norm2(x)
                    if np.isfinite(q):
                        qs.append(q)
            L = len(qs)
            if L >= self.min_links:
                if self.plant == "upper_median":
                    s = np.sqrt(f64(sorted(float(v) for v in qs)[L // 2]))
                else:
                    s = np.sqrt(lower_median(qs))
            else:
                s = s_prev
            if self.plant == "Rt_not_transposed":
                v = [((R[3 * i] * t[0] + R[3 * i + 1] * t[1]) + R[3 * i + 2] * t[2]) for i in range(3)]
            else:
                v = [((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) for i in range(3)]
            B = np.zeros(16, f64)
            for r in range(3):
                for c in range(3):
                    B[4 * r + c] = R[3 * c + r]
                B[4 * r + 3] = -(s * v[r])
            B[15] = 1.0
            Tn = mul4(B, T_prev) if self.plant == "wrong_side" else mul4(T_prev, B)
            for m, (a, b) in enumerate(matches):          # ascending: the higher match index overwrites
                if use[m]:
                    key = a if self.plant == "carry_by_first" else b
                    if 0 <= key < K:
                        new_carry[key] = s * Ys[m]
                        new_valid[key] = True
        self.Twc.append(Tn); self.scale.append(f64(s)); self.links.append(L)
        self.carry, self.valid = new_carry, new_valid

    def lift(self, frame, points, lo, hi, out):
        """rows [lo, hi) of points (N, 4) f32, points of pair (frame - 1 -> frame), into out (N, 4) f32; other rows untouched"""
        M, s = self.Twc[frame - 1], self.scale[frame]
        P = _w(points)
        with np.errstate(all="ignore"):
            for i in range(max(lo, 0), min(hi, len(P))):
                p = xf(M, np.array([s * P[i, 0], s * P[i, 1], s * P[i, 2]], f64))
                out[i, :3] = p.astype(np.float32)
                out[i, 3] = 1.0
        return out


# ------------------------------------------------------------------------------------------------ exact scenes
def _rot(axis, ang):
    axis = np.asarray(axis, f64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], f64)
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)      # ground truth only: not the contract's arithmetic


def scene(seed, points=40, frames=6, present=0.8):
    """Exact geometry: world points in front of every camera, camera f at centre C_f with orientation Rwc_f (camera -> world);
    per pair the inputs as the map step would deliver them: R, t of last -> current rounded to f32 with |t| = 1, and the pair's
    points in last-frame coordinates divided by the TRUE baseline, rounded to f32.  Keypoint index of point j in frame f is a
    per-frame permutation, so `first` and `second` differ.  Returns dict(truth..., pairs=[dict(matches, X, R, t)])."""
    rng = np.random.default_rng(seed)
    Pw = np.stack([rng.uniform(-2, 2, points), rng.uniform(-1.5, 1.5, points), rng.uniform(4, 9, points)], 1)
    base = rng.uniform(0.1, 0.4, frames - 1)
    C, Rwc = [np.zeros(3)], [np.eye(3)]
    for f in range(1, frames):
        d = rng.normal(size=3); d[2] *= 0.3
        d = d / np.linalg.norm(d)
        C.append(C[-1] + base[f - 1] * (Rwc[-1] @ d))
        Rwc.append(Rwc[-1] @ _rot(rng.normal(size=3), rng.uniform(0.01, 0.05)))
    perm = [rng.permutation(points) for _ in range(frames)]      # perm[f][j] = keypoint of point j in frame f
    pairs = []
    for f in range(1, frames):
        Rrel = Rwc[f].T @ Rwc[f - 1]                              # last camera -> current camera
        trel = Rwc[f].T @ (C[f - 1] - C[f])
        b = np.linalg.norm(trel)
        keep = np.flatnonzero(rng.uniform(size=points) < present)
        Xl = (Pw[keep] - C[f - 1]) @ Rwc[f - 1]                   # rows: Rwc^t (P - C)
        pairs.append(dict(matches=np.stack([perm[f - 1][keep], perm[f][keep]], 1).astype(np.int32),
                          X=np.concatenate([(Xl / b), np.ones((len(keep), 1))], 1).astype(np.float32),
                          R=Rrel.astype(np.float32).reshape(9), t=(trel / b).astype(np.float32), ids=keep))
    return dict(points=Pw, centres=np.stack(C), base=base, pairs=pairs, frames=frames, n=points)


def run_scene(sc, plant=None, min_links=8):
    """-> (World, worst error, bound unit): error of every lifted point and camera centre against the truth after one global
    scale (the first baseline); the unit is 2^-23 * frames * max|X| in world units."""
    w = World(sc["n"], min_links, plant)
    worst = 0.0
    g = sc["base"][0]
    for f, p in enumerate(sc["pairs"], 1):
        w.step(p["matches"], p["X"], p["R"], p["t"], sc["n"], sc["n"])
        out = np.zeros((len(p["X"]), 4), np.float32)
        w.lift(f, p["X"], 0, len(p["X"]), out)
        worst = max(worst, float(np.abs(out[:, :3].astype(f64) * g - sc["points"][p["ids"]]).max()))
        worst = max(worst, float(np.abs(w.Twc[f][[3, 7, 11]] * g - sc["centres"][f]).max()))
    unit = 2.0 ** -23 * sc["frames"] * float(np.abs(sc["points"]).max())
    return w, worst, unit


SCENE_SEEDS = (1, 2, 3, 4, 5, 6)
# error / unit per seed as measured by run_scene on the committed seeds (tests/test_ref_world.py re-measures and compares)
MEASURED_RATIOS = {1: 0.1145, 2: 0.1456, 3: 0.2110, 4: 0.2188, 5: 0.1325, 6: 0.1123}
C_BOUND = 0.9
