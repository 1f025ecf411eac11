"""Hand-worked inputs of the world frame, shared by tests/test_ref_world.py (the numpy reference against the expectations
written here) and tests/test_gpu_world.py (the device against the reference, bit for bit).

A case is a SCRIPT for one track at kp_stride 64: four steps (five frames), each a dict(winner, matches (n, 2) i32, X (n, 4) f32,
R (9,) f32, t (3,) f32, n_last, n_cur, poke).  `poke` = (carry (64, 3) f64, valid (64,) bool) replaces the carry ahead of the
step, so that the ratios of the first step can be worked out by hand: carry (0, 0, c) against X = (0, 0, 1) gives q = c^2 and
s = c exactly.  Every script ends with the same tail -- a step that follows on, a pair WITHOUT a winner, and a good pair again
-- so each one also covers "a pair without a winner between two good ones".  `expect` holds the hand-worked results of step 1.
"""
import numpy as np

K = 64
I9 = np.eye(3, dtype=np.float32).reshape(9)
TX = np.array([1, 0, 0], np.float32)
RZ90 = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1], np.float32)


def step(matches, X, R=I9, t=TX, n_last=K, n_cur=K, winner=True, poke=None):
    X = np.asarray(X, np.float32).reshape(-1, 3)
    X4 = np.concatenate([X, np.ones((len(X), 1), np.float32)], 1)
    return dict(winner=winner, matches=np.asarray(matches, np.int32).reshape(-1, 2), X=X4, R=np.asarray(R, np.float32).reshape(9),
                t=np.asarray(t, np.float32).reshape(3), n_last=n_last, n_cur=n_cur, poke=poke)


def poke_z(cs):
    """carry[i] = (0, 0, cs[i]), valid, for i < len(cs)"""
    carry, valid = np.zeros((K, 3)), np.zeros(K, bool)
    carry[:len(cs), 2] = cs
    valid[:len(cs)] = True
    return carry, valid


def _tail(seed):
    """follow on (keypoints 10 + i of the last frame, where step 1 put its matches), no winner, a good pair again"""
    rng = np.random.default_rng(seed)
    n = 12
    X = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(2, 5, n)], 1)
    a = step(np.stack([10 + np.arange(n), rng.permutation(n)], 1), X, RZ90, [0.6, 0, 0.8])
    none = step(np.zeros((0, 2)), np.zeros((0, 3)), winner=False)
    b = step(np.stack([np.arange(n), np.arange(n) + 3], 1), X[::-1], I9, [0, 1, 0])
    return [a, none, b]


def _first(cs, **kw):
    n = len(cs)
    return step(np.stack([np.arange(n), 10 + np.arange(n)], 1), [[0, 0, 1]] * n, poke=poke_z(cs), **kw)


def cases():
    c = {}
    c["odd_L9"] = dict(steps=[_first([7, 1, 9, 3, 5, 2, 8, 4, 6])] + _tail(1), expect=dict(scale=5.0, links=9))
    c["even_L8_lower_median"] = dict(steps=[_first([7, 1, 3, 5, 2, 8, 4, 6])] + _tail(2), expect=dict(scale=4.0, links=8))
    c["ties"] = dict(steps=[_first([3, 2, 3, 2, 1, 3, 2, 3])] + _tail(3), expect=dict(scale=2.0, links=8))
    c["L7_below_min_links"] = dict(steps=[_first([4, 4, 4, 4, 4, 4, 4])] + _tail(4), expect=dict(scale=1.0, links=7))
    c["L8_at_min_links"] = dict(steps=[_first([4, 4, 4, 4, 4, 4, 4, 4])] + _tail(5), expect=dict(scale=4.0, links=8))
    # camera centre: R = 90 degrees about z, t = (1, 0, 0): R^t t = (0, -1, 0), so the centre moves to (0, s, 0) = (0, 2, 0)
    c["pose_by_hand"] = dict(steps=[_first([2] * 8, R=RZ90)] + _tail(6),
                             expect=dict(scale=2.0, links=8, Twc=[0, 1, 0, 0, -1, 0, 0, 2, 0, 0, 1, 0, 0, 0, 0, 1]))
    # two matches onto keypoint 20 (matches 2 and 5): the higher index wins; its Y = X + t = (1, 5, 1), s = 2 -> (2, 10, 2)
    m = np.stack([np.arange(8), 10 + np.arange(8)], 1)
    m[2, 1] = m[5, 1] = 20
    X = np.tile([0, 0, 1], (8, 1)).astype(np.float32)
    X[5] = [0, 5, 1]
    st = step(m, X, poke=poke_z([2, 2, 2, 2, 2, 2 * np.sqrt(26.0), 2, 2]))
    c["two_onto_one_second"] = dict(steps=[st] + _tail(7), expect=dict(scale=2.0, links=8, carry={20: [2, 10, 2]}, invalid=[12, 15]))
    # behind the first camera (X.z < 0), behind the second (t.z = -2 puts Y.z = -1 for every point: its own step), a NaN point
    X = np.tile([0, 0, 1], (10, 1)).astype(np.float32)
    X[3] = [0, 0, -1]
    X[6] = [np.nan, 0, 1]
    X[8] = [0, np.inf, 1]
    st = step(np.stack([np.arange(10), 10 + np.arange(10)], 1), X, poke=poke_z([3] * 10))
    c["behind_first_nan_inf"] = dict(steps=[st] + _tail(8), expect=dict(scale=1.0, links=7, invalid=[13, 16, 18], carry={10: [1, 0, 1]}))
    st = step(np.stack([np.arange(9), 10 + np.arange(9)], 1), [[0, 0, 1]] * 9, t=[0, 0, -2], poke=poke_z([3] * 9))
    c["behind_second"] = dict(steps=[st] + _tail(9), expect=dict(scale=1.0, links=0, invalid=list(range(10, 19))))
    # `first` beyond the last frame's keypoint count (n_last = 9: matches 9 and 10 are ignored), `second` beyond n_cur likewise
    m = np.stack([np.arange(11), 10 + np.arange(11)], 1)
    st = step(m, [[0, 0, 1]] * 11, n_last=9, n_cur=20, poke=poke_z([1, 1, 1, 1, 6, 6, 6, 6, 6, 9, 9]))
    c["first_beyond_count"] = dict(steps=[st] + _tail(10), expect=dict(scale=6.0, links=9, invalid=[19, 20], carry={18: [6, 0, 6]}))
    m = np.stack([np.arange(10), 10 + np.arange(10)], 1)
    m[4, 0], m[7, 1], m[8, 0] = 70, 64, -1
    st = step(m, [[0, 0, 1]] * 10, poke=poke_z([5] * 10))
    c["index_outside_table"] = dict(steps=[st] + _tail(11), expect=dict(scale=1.0, links=7, invalid=[14, 18]))
    return c


def run_reference(ref_world, script, min_links=8, plant=None):
    """-> (World after the script, [lifted X (n, 4) f32 per step])"""
    w = ref_world.World(K, min_links, plant)
    lifted = []
    for f, st in enumerate(script, 1):
        if st["poke"] is not None:
            w.carry, w.valid = st["poke"][0].copy(), st["poke"][1].copy()
        w.step(st["matches"], st["X"], st["R"], st["t"], st["n_last"], st["n_cur"], winner=st["winner"])
        out = np.zeros_like(st["X"])
        lifted.append(w.lift(f, st["X"], 0, len(st["X"]), out))
    return w, lifted
