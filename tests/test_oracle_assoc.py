"""The oracle's map association (oracle/vso_pose.cpp vso_associate_map_points: src/vslam.cpp:129-161, orb_distance
src/PointMap.cpp:36-46, radius_search src/KDTree.cpp:145-171) held to the float64 restatement of tests/ref64.py.  Every
scene is built with no borderline decision and asserts that (ref64's slack > 1), so a scene cannot drift onto a boundary
unnoticed; the exact-tie scenes are built from exactly representable values instead.  The scene builders are shared with
tests/test_gpu_assoc.py, which holds the device to the same references."""
import numpy as np
import pytest

import ref64

def _c2(w, h):
    return np.array([[525, 0, w // 2, 0], [0, 525, h // 2, 0], [0, 0, 1, 0]], np.float32)   # K [I | 0]


def _back(px, z, w, h):
    """Map points (x, y, z, 1) that K [I | 0] projects onto the pixels px at depth z."""
    return np.stack([(px[:, 0] - w // 2) / 525.0 * z, (px[:, 1] - h // 2) / 525.0 * z, z, np.ones(len(z))], 1).astype(np.float32)


def clear_of_circles(px, kp, radius, band=1e-2):
    """Mask of the target pixels px whose squared distance to every keypoint is further than `band` from radius^2: map points
    projected there take no radius decision near its boundary."""
    kp = np.asarray(kp, np.float64)
    ok = np.ones(len(px), bool)
    for a in range(0, len(px), 256):
        d = px[a:a + 256, None, :] - kp[None, :, :]
        ok[a:a + 256] = (np.abs((d * d).sum(2) - radius * radius) > band).all(1)
    return ok


def random_scene(oracle, seed, w=640, h=480, n_kp=1500, n_map=3000):
    """Contended keypoints (several map points back-projected near one keypoint), keypoints already assigned (ids 0 and
    above), map points with 0 observations, points behind the camera that still project into the image (the reference does
    not test h's sign), points with h = 0, points out of view."""
    rng = np.random.default_rng(seed)
    kp = np.unique(np.rint(np.stack([rng.uniform(0, w - 1, n_kp), rng.uniform(0, h - 1, n_kp)], 1)), axis=0).astype(np.float32)
    rng.shuffle(kp)
    n_kp = len(kp)
    desc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    src = rng.integers(0, n_kp, n_map)
    src[: n_map // 6] = src[n_map // 6: 2 * (n_map // 6)]                 # duplicates contend for one keypoint
    px = kp[src].astype(np.float64) + rng.uniform(-1.6, 1.6, (n_map, 2))
    px[rng.random(n_map) < 0.08] += 5000                                  # out of view
    z = rng.uniform(2, 10, n_map)
    mp = _back(px, z, w, h)
    behind = rng.random(n_map) < 0.1
    mp[behind, :3] *= -1                                                  # (-X, -Y, -Z): h < 0, same pixel
    at_h0 = rng.random(n_map) < 0.03
    mp[at_h0, 2] = 0                                                      # h = 0 exactly: x, y = +-inf or NaN
    n_obs = rng.integers(0, 4, n_map)                                     # 0 observations -> distance u32_max
    offs = np.zeros(n_map + 1, np.int32); offs[1:] = np.cumsum(n_obs)
    od = rng.integers(0, 256, (max(int(offs[-1]), 1), 32), dtype=np.uint8)
    for i in range(n_map):
        for o in range(offs[i], offs[i + 1]):
            if rng.random() < 0.8:
                od[o] = desc[src[i]] ^ np.packbits(rng.random(256) < rng.choice([0.02, 0.1, 0.3]))
    ids = np.full(n_kp, -1, np.int32)
    ids[rng.integers(0, n_kp, n_kp // 5)] = rng.integers(0, 50, n_kp // 5)
    return dict(kp=kp, desc=desc, nodes=oracle.kdtree_build_frame(kp), c2=_c2(w, h), mp=mp, offs=offs, od=od, ids=ids, w=w, h=h,
                radius=2.0, behind=behind, at_h0=at_h0)


def many_hits_scene(oracle, radius=10.0, w=160, h=120):
    """One map point over a one-pixel lattice with `radius` 10: ~300 keypoints in range.  Only the LAST hit in the tree's
    visit order (well past the 256th) has an acceptable descriptor, so a search that stops at 256 hits claims nothing."""
    gx, gy = np.meshgrid(np.arange(40, 80), np.arange(30, 70))
    kp = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    rng = np.random.default_rng(12)
    rng.shuffle(kp)
    nodes = oracle.kdtree_build_frame(kp)
    c2 = _c2(w, h)
    mp = _back(np.array([[60.25, 50.4]]), np.array([4.0]), w, h)
    proto = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.repeat((~proto)[None], len(kp), 0)                         # 256 bits from the observation: never accepted
    r = ref64.associate(mp, c2, w, h, nodes, kp, desc, np.array([0, 1]), proto[None], np.full(len(kp), -1, np.int32), radius)
    hits = r["hits"][0]
    target = hits[-1]
    desc[target] = proto
    return dict(kp=kp, desc=desc, nodes=nodes, c2=c2, mp=mp, offs=np.array([0, 1], np.int32), od=proto[None].copy(),
                ids=np.full(len(kp), -1, np.int32), w=w, h=h, radius=radius, target=target, n_hits=len(hits))


def acceptable_hits_scene(oracle, n_acc, w=160, h=120):
    """One map point whose radius-3 query over a one-pixel lattice finds 28 keypoints, exactly n_acc of them with an
    acceptable descriptor; the first n_acc - 1 of those (in visit order) already belong to other map points, so the claim is
    the last acceptable hit.  The device keeps 16 acceptable hits per map point (include/vslam_amd.h)."""
    gx, gy = np.meshgrid(np.arange(20, 50), np.arange(20, 50))
    kp = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    rng = np.random.default_rng(30 + n_acc)
    rng.shuffle(kp)
    nodes = oracle.kdtree_build_frame(kp)
    c2 = _c2(w, h)
    mp = _back(np.array([[35.1, 34.8]]), np.array([3.0]), w, h)
    proto = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.repeat((~proto)[None], len(kp), 0)
    ids = np.full(len(kp), -1, np.int32)
    r = ref64.associate(mp, c2, w, h, nodes, kp, desc, np.array([0, 1]), proto[None], ids, 3.0)
    hits = r["hits"][0]
    acc = np.asarray(hits)[np.sort(rng.choice(len(hits), n_acc, replace=False))]
    desc[acc] = proto
    ids[acc[:-1]] = 1
    return dict(kp=kp, desc=desc, nodes=nodes, c2=c2, mp=mp, offs=np.array([0, 1], np.int32), od=proto[None].copy(), ids=ids,
                w=w, h=h, radius=3.0, target=int(acc[-1]), n_hits=len(hits))


def exact_scene():
    """Values that every stage computes exactly (c2 = [I | 0], integer-valued points at depth 1, integer keypoints): the ties
    of the reference's comparisons, taken literally.
      map 0 projects to (W, 10): not in view (x < W), though a keypoint is 1 px away;
      map 1 projects to (0, 20): in view (x >= 0), claims the keypoint 1 px away;
      map 2 projects to (30, 30): its one acceptable keypoint lies at exactly d^2 = r^2 = 4, no hit (d^2 < r^2);
      map 3 projects to (60, 30): two observations, 10 and 200 bits from the keypoint: orb_distance is the minimum, 10;
      map 4 projects to (60, 50): one observation exactly 64 bits away: not accepted (< 64)."""
    W, H = 64, 64
    c2 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    kp = np.array([[63, 10], [1, 20], [32, 30], [10, 50], [61, 30], [60, 51]], np.float32)
    mp = np.array([[64, 10, 1, 1], [0, 20, 1, 1], [30, 30, 1, 1], [60, 30, 1, 1], [60, 50, 1, 1]], np.float32)
    rng = np.random.default_rng(1)
    desc = rng.integers(0, 256, (len(kp), 32), dtype=np.uint8)

    def flip(d, bits):
        m = np.zeros(256, bool); m[:bits] = True
        return d ^ np.packbits(m)
    od = np.stack([desc[0], desc[1], desc[2], flip(desc[4], 10), flip(desc[4], 200), flip(desc[5], 64)])
    offs = np.array([0, 1, 2, 3, 5, 6], np.int32)
    return dict(kp=kp, desc=desc, c2=c2, mp=mp, offs=offs, od=od, ids=np.full(len(kp), -1, np.int32), w=W, h=H, radius=2.0,
                expect=[-1, 1, -1, 4, -1])


def run_ref(s, nodes=None):
    return ref64.associate(s["mp"], s["c2"], s["w"], s["h"], s["nodes"] if nodes is None else nodes, s["kp"], s["desc"], s["offs"],
                           s["od"], s["ids"], s["radius"])


def run_oracle(oracle, s, nodes=None):
    return oracle.associate(s["mp"], s["c2"], s["w"], s["h"], s["nodes"] if nodes is None else nodes, s["kp"], s["desc"], s["offs"],
                            s["od"], s["ids"], radius=s["radius"])


# -------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("seed,n_kp,n_map", [(5, 1500, 3000), (2, 400, 90), (3, 2000, 10), (4, 300, 2500)])
def test_association_random_scenes(oracle, seed, n_kp, n_map):
    s = random_scene(oracle, seed, n_kp=n_kp, n_map=n_map)
    r = run_ref(s)
    assert r["slack"] > 1, "the scene has a borderline decision"
    ids, claim = run_oracle(oracle, s)
    assert np.array_equal(claim, r["claim"]) and np.array_equal(ids, r["ids"])
    if n_map >= 90:
        assert (r["claim"] >= 0).sum() > n_map // 20
        assert (r["claim"][s["behind"]] >= 0).any(), "a point behind the camera that projects into view must claim"
        assert (r["claim"][s["at_h0"]] == -1).all() and not r["in_view"][s["at_h0"]].any()
        assert (r["claim"][s["offs"][1:] == s["offs"][:-1]] == -1).all(), "no observations: orb_distance is u32_max"
        taken_before = s["ids"] >= 0
        assert not np.isin(r["claim"][r["claim"] >= 0], np.nonzero(taken_before)[0]).any()


def test_association_long_claim_chains(oracle):
    """Lattice keypoints, every descriptor acceptable, several map points per keypoint: the claims cascade in map order."""
    w, h = 160, 120
    rng = np.random.default_rng(21)
    gx, gy = np.meshgrid(np.arange(20, 60), np.arange(30, 70))
    kp = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    rng.shuffle(kp)
    proto = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.repeat(proto[None], len(kp), 0)
    desc[:, 0] ^= rng.integers(0, 256, len(kp), dtype=np.uint8)
    n_map = 2000
    px = np.stack([rng.uniform(18, 62, n_map), rng.uniform(28, 72, n_map)], 1)
    s = dict(kp=kp, desc=desc, nodes=oracle.kdtree_build_frame(kp), c2=_c2(w, h), mp=_back(px, rng.uniform(2, 6, n_map), w, h),
             offs=np.arange(n_map + 1, dtype=np.int32), od=np.repeat(proto[None], n_map, 0), ids=np.where(rng.random(len(kp)) < 0.3, 7, -1)
             .astype(np.int32), w=w, h=h, radius=2.05)
    r = run_ref(s)
    assert r["slack"] > 1
    ids, claim = run_oracle(oracle, s)
    assert np.array_equal(claim, r["claim"]) and np.array_equal(ids, r["ids"])
    assert (r["claim"] >= 0).sum() > 0.9 * (s["ids"] < 0).sum()


def test_association_more_than_256_radius_hits(oracle):
    """radius_search has no cap (src/KDTree.cpp:145-149): the acceptable keypoint after the 256th hit is claimed."""
    s = many_hits_scene(oracle)
    assert s["n_hits"] > 256
    r = run_ref(s)
    assert r["slack"] > 1 and r["hits"][0].index(s["target"]) >= 256
    assert r["claim"][0] == s["target"]
    ids, claim = run_oracle(oracle, s)
    assert claim[0] == s["target"] and ids[s["target"]] == 0


@pytest.mark.parametrize("n_acc", [16, 17])
def test_association_16_and_17_acceptable_hits(oracle, n_acc):
    s = acceptable_hits_scene(oracle, n_acc)
    r = run_ref(s)
    assert r["slack"] > 1
    assert ref64.acceptable_hits(r, 0, s["desc"], s["offs"], s["od"]) == n_acc
    assert r["claim"][0] == s["target"]
    ids, claim = run_oracle(oracle, s)
    assert np.array_equal(claim, r["claim"]) and np.array_equal(ids, r["ids"])


def test_association_exact_ties(oracle):
    s = exact_scene()
    s["nodes"] = oracle.kdtree_build_frame(s["kp"])
    r = run_ref(s)
    assert list(r["claim"]) == s["expect"]
    assert list(r["in_view"]) == [False, True, True, True, True]
    ids, claim = run_oracle(oracle, s)
    assert list(claim) == s["expect"] and np.array_equal(ids, r["ids"])


def test_radius_search_visits_in_tree_order(oracle):
    """ref64's walk of the node array against the oracle's (src/KDTree.cpp:151-171): same hits, same order."""
    rng = np.random.default_rng(8)
    for n in (1, 2, 3, 17, 600, 3000):
        xy = np.rint(rng.uniform(0, 100, (n, 2))).astype(np.float32)
        nodes = oracle.kdtree_build_frame(xy)
        for _ in range(30):
            q = rng.uniform(-5, 105, 2).astype(np.float32) + np.float32(0.37)
            rad = float(rng.choice([1.0, 2.0, 7.5]))
            got, cnt = oracle.kdtree_radius_frame(nodes, xy, q, rad, cap=n)
            want = ref64.radius_search(nodes, xy.astype(np.float64), q.astype(np.float64), rad)
            assert cnt == len(want) and list(got) == want
