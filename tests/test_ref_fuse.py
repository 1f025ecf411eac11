"""tests/ref_fuse.py against a second form of each rule (a breadth-first search over an explicit link graph and a set-based dedupe for the
fusion; for the cull, the hand cases whose answers are written out), and on the maps that the reference's loop builds from exact
scenes: pnp_cases.world_scene (60 and 400 points, six frames) through ref_map.PointMapModel with the oracle.  CPU only.

What the scenes show (printed by the test, recomputed on every run): every map point has two observations but a handful; the groups
that shared (frame, keypoint) observations link never mix two physical points; there are about a third as many groups as map points.

The cull on exact keypoints.  With the true geometry every observation of every survivor is good (n_good == n_usable).  At the DEFAULT
parameters some survivors are culled all the same: a point seen in two frames only whose last frame lies mature_age = 3 or more frames
back needs mature_good = 3 good observations and has 2 (measured: 3 of 28 and 35 of 205 survivors).  That is the maturity rule doing
what include/vslam_fuse.h says, not a geometric rejection, so "the cull keeps every survivor" is asserted with the maturity rule
switched off (mature_good = min_good = 2), and at the defaults it is asserted that every culled survivor is such a point."""
import numpy as np
import pytest

import fuse_cases as fc
import pnp_cases as pc
import ref_fuse as rf
import ref_map


def _same(a, b, keys, name=""):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (name, k, a[k], b[k])


def test_hand_cases_of_the_fusion_in_both_forms():
    for name, c in fc.fuse_hand_cases().items():
        r = fc.fuse_reference(c)
        _same(r, rf.fuse_second(c["n"], c["offsets"], c["cam"], c["kp"], c["cam_stride"], c["kp_stride"], c.get("mask")), rf.FUSE_OUTS, name)
        assert np.array_equal(r["fuse_to"], c["expect"]), (name, r["fuse_to"])
    c = fc.fuse_hand_cases()
    r = fc.fuse_reference(c["two_shared_cells"])
    assert r["stats"].tolist() == [3, 1, 1, 3] and r["out_offsets"].tolist() == [0, 1, 3, 3]
    assert list(zip(r["out_cam"], r["out_kp"], r["out_src"])) == [(4, 4, 0), (0, 1, 1), (1, 2, 2)]
    r = fc.fuse_reference(c["duplicate_inside_a_row"])
    assert r["out_src"].tolist() == [0, 2, 4] and r["stats"].tolist() == [2, 0, 0, 3]
    r = fc.fuse_reference(c["chain_of_three"])
    assert r["out_src"].tolist() == [0, 1, 3, 5] and r["out_offsets"].tolist() == [0, 4, 4, 4]
    r = fc.fuse_reference(c["broken_decreasing"])
    assert not r["out_offsets"].any() and not r["stats"].any()


@pytest.mark.parametrize("n", [1, 2, 40, 257, 1200])
def test_random_items_of_the_fusion_in_both_forms(n):
    for seed in range(3):
        c = rf.random_fuse_item(1000 * n + seed, n, kp_stride=max(16, n // 2), S=n + 5)
        a = fc.fuse_reference(c)
        b = rf.fuse_second(c["n"], c["offsets"], c["cam"], c["kp"], c["cam_stride"], c["kp_stride"], c["mask"])
        _same(a, b, rf.FUSE_OUTS, (n, seed))
        if n >= 40:
            assert a["stats"][1] > 0 and a["stats"][2] > 0 and 0 < a["stats"][3] < a["out_src"].max() + 1 and (a["fuse_to"][:n] < 0).any()
        # what the rule promises, from the outputs alone
        rows = np.diff(a["out_offsets"])
        idx = np.arange(len(a["fuse_to"]))
        assert (rows[a["fuse_to"] != idx] == 0).all()
        cells = set()
        for s in np.flatnonzero(rows):
            row = list(zip(a["out_cam"][a["out_offsets"][s]:a["out_offsets"][s + 1]], a["out_kp"][a["out_offsets"][s]:a["out_offsets"][s + 1]]))
            assert len(set(row)) == len(row) and not cells & set(row), "a cell belongs to one group and appears once"
            assert (np.diff(a["out_src"][a["out_offsets"][s]:a["out_offsets"][s + 1]]) > 0).all(), "merged order is input order"
            cells |= set(row)


def test_hand_case_of_the_cull():
    c = fc.cull_hand_case()
    r = fc.cull_reference(c)
    assert np.array_equal(r["keep"], c["expect"]), r["keep"]
    assert np.array_equal(r["counts"], c["expect_counts"]), r["counts"]
    assert r["stats"].tolist() == [12, 5, 7, int(c["expect_counts"][:, 1].sum())]
    # an open disc, a first-observation-only count and an age taken from the first camera would each change an answer
    assert r["keep"][0] == 1 and r["keep"][1] == 0 and r["keep"][6] == 0 and r["keep"][8] == 1


@pytest.fixture(scope="module")
def scene_maps(oracle):
    """the two scenes through the reference's loop: [(scene, model, (offsets, frame, kp))]"""
    out = []
    for points in (60, 400):
        seed, ws = pc.first_world_scene(points)
        n = ws["n"]
        m = ref_map.PointMapModel(oracle, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H, n)
        m.first_frame(ws["xy"][0], ws["desc"][0], oracle.kdtree_build_frame(ws["xy"][0]))
        for f in range(1, 6):
            p = ws["pairs"][f - 1]
            m.step(ws["xy"][f], ws["desc"][f], oracle.kdtree_build_frame(ws["xy"][f]), None, p["matches"], np.asarray(p["F"], np.float32))
        out.append((seed, ws, m, m.observations()))
    return out


def _identity(ws, fr, kp):
    """the physical point behind every observation, from the scene's per-frame permutation"""
    inv = [np.argsort(q) for q in ws["perm"]]
    return np.array([inv[f][k] for f, k in zip(fr, kp)])


def test_scene_maps_fuse_into_one_group_per_physical_point(scene_maps):
    for seed, ws, m, (off, fr, kp) in scene_maps:
        n = ws["n"]
        r = rf.fuse_item(m.size, off, fr, kp, 6, n)
        _same(r, rf.fuse_second(m.size, off, fr, kp, 6, n), rf.FUSE_OUTS, seed)
        ident = _identity(ws, fr, kp)
        per_point = [set(ident[off[i]:off[i + 1]]) for i in range(m.size)]
        assert all(len(s) == 1 for s in per_point), "a map point observes one physical point"
        groups = {}
        for i in range(m.size):
            groups.setdefault(int(r["fuse_to"][i]), []).append(i)
        mixed = sum(len(set.union(*[per_point[i] for i in g])) > 1 for g in groups.values())
        holders = {}
        for i in range(m.size):
            for o in range(off[i], off[i + 1]):
                holders.setdefault((int(fr[o]), int(kp[o])), set()).add(int(r["fuse_to"][i]))
        split = sum(len(s) > 1 for s in holders.values())
        hist = np.bincount(np.diff(off))
        print(f"scene of {n} points (seed {seed}): {m.size} map points, {int(hist[2])} with two observations; {len(groups)} groups, "
              f"{int(r['stats'][1])} with more than one member, up to {max(len(g) for g in groups.values())} members; entries {len(fr)} -> {int(r['stats'][3])}")
        assert mixed == 0, "every group holds one physical point"
        assert split == 0, "every map point linked by a shared (frame, keypoint) is in one group"
        assert r["stats"][1] > 0 and len(groups) < m.size and r["stats"][3] < len(fr)
        assert hist[2] >= 0.9 * m.size


def _true_geometry(ws, m, off, fr, kp, r):
    """world points and cameras of the scene itself: the survivors' rows, NaN for the absorbed"""
    sc = ws["scene"]
    first = _identity(ws, fr, kp)[off[:-1]]
    pts = np.ones((m.size, 4), np.float32)
    pts[:, :3] = sc["points"][first]
    pts = rf.nan_rows(pts, np.flatnonzero(r["fuse_to"] != np.arange(m.size)))
    R = np.stack([ws["Rwc"][f].T.reshape(9) for f in range(6)])
    T = np.stack([-(ws["Rwc"][f].T @ sc["centres"][f]) for f in range(6)])
    return pts, R, T


def test_cull_on_the_fused_scene_maps(scene_maps):
    for seed, ws, m, (off, fr, kp) in scene_maps:
        n = ws["n"]
        r = rf.fuse_item(m.size, off, fr, kp, 6, n)
        pts, R, T = _true_geometry(ws, m, off, fr, kp, r)
        xy = np.stack(ws["xy"])
        survivors = int((r["fuse_to"] == np.arange(m.size)).sum())

        def cull(xy_, **kw):
            return rf.cull_item(pts, m.size, r["out_offsets"], r["out_cam"], r["out_kp"], R, T, 6, xy_, pc.SCENE_K, **kw)
        flat = cull(xy, mature_good=2)
        assert flat["stats"].tolist() == [survivors, survivors, 0, int(r["stats"][3])], "exact keypoints: every observation good, every survivor kept"
        dflt = cull(xy)
        culled = np.flatnonzero(dflt["keep"] == 0)
        assert (dflt["counts"][culled] == [2, 2]).all() and all(r["out_cam"][r["out_offsets"][i + 1] - 1] + 3 < 6 for i in culled)
        rng = np.random.default_rng(seed)
        noisy = xy.copy()
        bad = rng.permutation(n)[:n // 5]
        noisy[3, bad] = rng.uniform(0, [pc.SCENE_W, pc.SCENE_H], (len(bad), 2)).astype(np.float32)
        a, b = cull(noisy, mature_good=2), cull(noisy)
        print(f"scene of {n} points: {survivors} survivors; exact keypoints: kept {flat['stats'][1]} (maturity off), {dflt['stats'][1]} at the defaults; "
              f"a fifth of frame 3 replaced: kept / culled {a['stats'][1]} / {a['stats'][2]} (maturity off), {b['stats'][1]} / {b['stats'][2]} at the defaults")
        assert b["stats"][1] > 0 and b["stats"][2] > 0, "at the defaults the noisy frame leaves some points kept and some culled"
        assert b["stats"][2] >= dflt["stats"][2] and b["stats"][3] < dflt["stats"][3] and a["stats"][3] < flat["stats"][3] and a["stats"][1] > 0
        assert (a["keep"][r["fuse_to"] != np.arange(m.size)] == -1).all(), "an absorbed point (NaN row, empty row) takes no part"
