"""Hand cases and grid-edge cases of the search by projection (include/vslam_search.h), one rule each, shared by the serial host
walk (tests/test_search_serial.py), the reference's own tests (tests/test_ref_search.py) and the device tests
(tests/test_gpu_search.py).  A case is a dict of one item's arrays in ref_search.planted_scene's keys plus `params` (fields of
vslam_search_params over the defaults), `taken` (or None) and, where the outcome is known by hand, `expect`: kp_of_point.

Hand cases use K = (1, 1, 0, 0), R = I, T = 0 and z = 1, so that (u, v) = (x, y) exactly.  D(b) is the descriptor with its first
b bits set: the Hamming distance of D(a) and D(b) is |a - b|."""
import numpy as np

f32 = np.float32
K_UNIT = np.eye(3, dtype=np.float32)
R_UNIT = np.eye(3).reshape(9)
T_ZERO = np.zeros(3)


def D(bits):
    d = np.zeros(32, np.uint8)
    for b in range(bits):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def case(points, obs, kps, width=64, height=48, taken=None, expect=None, n_points=None, n_kp=None, K=K_UNIT, R=R_UNIT, T=T_ZERO, **params):
    """points: (x, y, z) rows; obs: per point a list of descriptors; kps: (x, y, descriptor) rows"""
    P = np.ones((max(len(points), 1), 4), np.float32)
    P[:len(points), :3] = np.array(points, np.float32).reshape(-1, 3)
    counts = [len(o) for o in obs] + [0] * (len(P) - len(obs))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    flat = [d for o in obs for d in o]
    obs_desc = np.array(flat, np.uint8).reshape(-1, 32) if flat else np.zeros((1, 32), np.uint8)
    xy = np.zeros((max(len(kps), 1), 2), np.float32)
    desc = np.zeros((max(len(kps), 1), 32), np.uint8)
    for k, (x, y, d) in enumerate(kps):
        xy[k] = (x, y)
        desc[k] = d
    return dict(points=P, n_points=len(points) if n_points is None else n_points, offsets=offsets, obs_desc=obs_desc, K=np.asarray(K, np.float32),
                width=width, height=height, xy=xy, desc=desc, n_kp=len(kps) if n_kp is None else n_kp, R=np.array(R, np.float64),
                T=np.array(T, np.float64), taken=None if taken is None else np.array(taken, np.int32), params=params,
                expect=None if expect is None else np.array(expect, np.int32))


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def hand_cases():
    c = {}
    o = [[D(0)]]
    # the disc is closed: 3-4-5 at radius 5, and 4-7.5-8.5 at radius 8.5; the next representable coordinate is out
    c["disc_on_5"] = case([(10, 10, 1)], o, [(13, 14, D(0))], radius_px=5.0, expect=[0])
    c["disc_past_5"] = case([(10, 10, 1)], o, [(13, up(14), D(0))], radius_px=5.0, expect=[-1])
    c["disc_on_8.5"] = case([(10, 10, 1)], o, [(14, 17.5, D(0))], radius_px=8.5, expect=[0])
    c["disc_past_8.5"] = case([(10, 10, 1)], o, [(up(14), 17.5, D(0))], radius_px=8.5, expect=[-1])
    c["disc_axis_8.5"] = case([(10, 10, 1)], o, [(18.5, 10, D(0)), (up(18.5), 10, D(0))], radius_px=8.5, ratio10=0, expect=[0])
    # visibility at width 20, height 15, radius 1: every point has a keypoint of its own descriptor beside it
    nan, inf = float("nan"), float("inf")
    pts = [(0, 5, 1), (20, 5, 1), (5, 15, 1), (-0.5, 8, 1), (10, 2, 0), (-10, -4, -1), (nan, 6, 1), (inf, 6, 1), (10, 8, 1), (10, 12, 1),
           (3, nan, 1), (3, 3, inf)]
    obs = [[D(0)]] * 8 + [[]] + [[D(0)]] * 3
    kps = [(0, 5, D(0)), (19.5, 5, D(0)), (5, 14.5, D(0)), (0, 8, D(0)), (10, 2, D(0)), (10, 4, D(0)), (15, 6, D(0)), (17, 6, D(0)),
           (10, 8, D(0)), (10, 12, D(0)), (3, 3, D(0))]
    c["visibility"] = case(pts, obs, kps, width=20, height=15, radius_px=1.0, expect=[0, -1, -1, -1, -1, -1, -1, -1, -1, 9, -1, -1])
    # two keypoints with the same d: the lower k wins and d1 = d0 (so any ratio test rejects it)
    two = [(11, 10, D(5)), (9, 10, D(5))]
    c["tie_lower_k"] = case([(10, 10, 1)], o, two, ratio10=0, expect=[0])
    c["tie_d1_is_d0"] = case([(10, 10, 1)], o, two, ratio10=10, expect=[-1])
    # the ratio boundary at ratio10 = 8
    c["ratio_8_10"] = case([(10, 10, 1)], o, [(11, 10, D(10)), (9, 10, D(8))], ratio10=8, expect=[-1])
    c["ratio_8_11"] = case([(10, 10, 1)], o, [(11, 10, D(11)), (9, 10, D(8))], ratio10=8, expect=[1])
    c["ratio_single"] = case([(10, 10, 1)], o, [(9, 10, D(8))], ratio10=8, expect=[0])
    c["ratio_off"] = case([(10, 10, 1)], o, [(11, 10, D(10)), (9, 10, D(8))], ratio10=0, expect=[1])
    c["ratio_0_0"] = case([(10, 10, 1)], o, [(11, 10, D(0)), (9, 10, D(0))], ratio10=8, expect=[-1])
    # the threshold
    c["threshold_63"] = case([(10, 10, 1)], o, [(10, 10, D(63))], dist_threshold=64, expect=[0])
    c["threshold_64"] = case([(10, 10, 1)], o, [(10, 10, D(64))], dist_threshold=64, expect=[-1])
    c["threshold_257"] = case([(10, 10, 1)], o, [(10, 10, D(256))], dist_threshold=257, expect=[0])
    # three observations of which only the last is close
    c["last_observation"] = case([(10, 10, 1)], [[D(200), D(150), D(3)]], [(10, 10, D(0))], expect=[0])
    # two points proposing one keypoint
    both = [(10, 10, 1), (10.5, 10, 1)]
    c["contest_lower_d"] = case(both, [[D(5)], [D(3)]], [(10.25, 10, D(0))], expect=[-1, 0])
    c["contest_lower_i"] = case(both, [[D(4)], [D(4)]], [(10.25, 10, D(0))], expect=[0, -1])
    c["contest_no_second_choice"] = case(both, [[D(5)], [D(3)]], [(10.25, 10, D(0)), (12, 10, D(45))], expect=[-1, 0])
    # a taken keypoint is no candidate
    c["taken"] = case([(10, 10, 1)], o, [(10, 10, D(0)), (11, 10, D(9))], taken=[7, -1], expect=[1])
    c["taken_zero"] = case([(10, 10, 1)], o, [(10, 10, D(0)), (11, 10, D(9))], taken=[0, -1], expect=[1])
    # sizes
    c["no_keypoints"] = case([(10, 10, 1)], o, [(10, 10, D(0))], n_kp=0, expect=[-1])
    c["negative_keypoints"] = case([(10, 10, 1)], o, [(10, 10, D(0))], n_kp=-3, expect=[-1])
    c["no_points"] = case([(10, 10, 1)], o, [(10, 10, D(0))], n_points=0, expect=[-1])
    c["counts_above_strides"] = case([(10, 10, 1), (20, 20, 1)], [[D(0)], [D(9)]], [(10, 10, D(0)), (20, 20, D(9))], n_points=7, n_kp=11,
                                     expect=[0, 1])
    # keypoints that are not finite
    c["nan_keypoints"] = case([(10, 10, 1)], o, [(nan, 10, D(0)), (10, nan, D(0)), (inf, 10, D(0)), (11, 10, D(7))], expect=[3])
    # a pose that is not finite: nothing
    c["nan_pose"] = case([(10, 10, 1)], o, [(10, 10, D(0))], T=(0, nan, 0), expect=[-1])
    c["inf_rotation"] = case([(10, 10, 1)], o, [(10, 10, D(0))], R=(1, 0, 0, 0, 1, 0, inf, 0, 1), expect=[-1])
    return c


def random_case(seed, n_points, n_kp, width, height, radius, patch=None, outside=True, max_obs=3, K=None):
    """Points that project all over the image (and a little beyond), keypoints scattered on them, on cell borders of the grid, in
    a patch (patch = (x, y, side): all keypoints in that square) and outside the image; descriptors from a pool of 64 with a few
    bits flipped, so that ties, ratio rejections and contests all occur."""
    rng = np.random.default_rng(seed)
    K = np.array([[width * 0.8, 0, width / 2], [0, width * 0.8, height / 2], [0, 0, 1]], np.float32) if K is None else K
    z = rng.uniform(2.0, 6.0, n_points)
    if patch is None:
        u = rng.uniform(-0.03 * width, 1.03 * width, n_points)
        v = rng.uniform(-0.03 * height, 1.03 * height, n_points)
    else:
        u = rng.uniform(patch[0] - 2 * radius, patch[0] + patch[2] + 2 * radius, n_points)
        v = rng.uniform(patch[1] - 2 * radius, patch[1] + patch[2] + 2 * radius, n_points)
    P = np.ones((n_points, 4), np.float32)
    P[:, 0] = (u - K[0, 2]) / K[0, 0] * z
    P[:, 1] = (v - K[1, 2]) / K[1, 1] * z
    P[:, 2] = z
    pool = rng.integers(0, 256, (64, 32), dtype=np.uint8)

    def noisy(idx):
        d = pool[idx].copy()
        flips = rng.integers(0, 256, (len(idx), 6))
        on = rng.uniform(size=flips.shape) < 0.5
        for j in range(flips.shape[1]):
            rows = np.flatnonzero(on[:, j])
            d[rows, flips[rows, j] >> 3] ^= (1 << (flips[rows, j] & 7)).astype(np.uint8)
        return d
    counts = np.where(rng.uniform(size=n_points) < 0.03, 0, rng.integers(1, max_obs + 1, n_points))   # a few without observations
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pid = rng.integers(0, 64, n_points)
    obs = noisy(np.repeat(pid, counts)) if counts.sum() else np.zeros((1, 32), np.uint8)
    xy = np.zeros((max(n_kp, 1), 2), np.float32)
    kid = rng.integers(0, 64, max(n_kp, 1))
    if patch is None:
        src = rng.integers(0, n_points, n_kp)
        xy[:n_kp, 0] = u[src] + rng.uniform(-1.2 * radius, 1.2 * radius, n_kp)
        xy[:n_kp, 1] = v[src] + rng.uniform(-1.2 * radius, 1.2 * radius, n_kp)
        kid[:n_kp] = np.where(rng.uniform(size=n_kp) < 0.7, pid[src], kid[:n_kp])
        # a share of them exactly on, and one step below, multiples of the cell side in x or y (both sides of cell borders)
        c = max(radius + 2.0 ** -9, max(width, height) / 64.0)
        snap = np.flatnonzero(rng.uniform(size=n_kp) < 0.2)
        axis = rng.integers(0, 2, len(snap))
        edge = (np.round(xy[snap, axis].astype(np.float64) / c) * c).astype(np.float32)
        xy[snap, axis] = np.where(rng.uniform(size=len(snap)) < 0.5, edge, np.nextafter(edge, f32(-np.inf)))
        if outside:   # beyond the image on every side, within the radius of projections just inside
            out = np.flatnonzero(rng.uniform(size=n_kp) < 0.05)
            side = rng.integers(0, 4, len(out))
            xy[out, 0] = np.where(side == 0, -rng.uniform(0, radius, len(out)), np.where(side == 1, width + rng.uniform(0, radius, len(out)), xy[out, 0]))
            xy[out, 1] = np.where(side == 2, -rng.uniform(0, radius, len(out)), np.where(side == 3, height + rng.uniform(0, radius, len(out)), xy[out, 1]))
    else:
        xy[:n_kp, 0] = rng.uniform(patch[0], patch[0] + patch[2], n_kp)
        xy[:n_kp, 1] = rng.uniform(patch[1], patch[1] + patch[2], n_kp)
    bad = np.flatnonzero(rng.uniform(size=n_kp) < 0.01)
    xy[bad, rng.integers(0, 2, len(bad))] = np.nan
    desc = noisy(kid)
    taken = np.where(rng.uniform(size=len(xy)) < 0.05, rng.integers(0, 9, len(xy)), -1).astype(np.int32)
    a = 0.8 / max(width, height)   # a pose that moves every projection by some tenths of a pixel, whatever the image's size
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).reshape(9)
    T = np.array([1.2 / K[0, 0], -0.9 / K[1, 1], 0.2 / max(width, height)], np.float64)
    return dict(points=P, n_points=n_points, offsets=offsets, obs_desc=obs, K=K, width=width, height=height, xy=xy, desc=desc, n_kp=n_kp,
                R=R, T=T, taken=taken, params=dict(radius_px=radius), expect=None)


def grid_cases():
    """the grid's edges: images smaller than one cell up to the 64 x 64 cap, radii 1 .. 64, keypoints on both sides of cell borders
    and outside the image, all keypoints in one patch"""
    c = {}
    seed = 0
    for (w, h) in ((37, 23), (640, 480), (1280, 720), (16384, 16384)):
        for r in (1.0, 8.0, 8.5, 64.0):
            seed += 1
            c[f"{w}x{h}_r{r:g}"] = random_case(seed, 300, 400, w, h, r)
    c["patch_16px"] = random_case(99, 40, 2000, 640, 480, 8.0, patch=(301, 207, 16))
    return c
