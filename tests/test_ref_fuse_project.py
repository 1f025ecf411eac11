"""tests/ref_fuse_project.py against its second formulation (one search per camera over all the points with rows emptied, holders
from a dictionary), on the hand cases whose answers are written out and under every plant, and on the maps that the reference's loop
builds from exact scenes: pnp_cases.first_world_scene (60 and 400 points, six frames) through ref_map.PointMapModel with the oracle,
once as they are and once as a revisit ("two passes": cameras 6 .. 11 repeat cameras 0 .. 5 with freshly permuted keypoint indices, every
map point is in the item twice, the copy's observations in the second pass, so the copies share no keypoint).  CPU only.

What the scenes show (printed by the test, recomputed on every run), with the scenes' true geometry and the default search
parameters: one geometric round behind the fusion by shared observations leaves exactly one live point per physical point -- 21 and
139, in both the six-frame and the two-pass items --, no group mixes two physical points and no found pair names a keypoint of
another physical point.  With 0.5 px of keypoint noise and up to 20 flipped descriptor bits the two conditions hold; the live count is
printed only.

The cases named in fuse_project_cases.INERT (n <= 0 and the broken CSRs) try no pair at all, so no plant can change them; every other
hand case changes under at least one plant."""
import numpy as np
import pytest

import fuse_project_cases as fpc
import pnp_cases as pc
import ref_fuse as rf
import ref_fuse_project as rfp
import ref_map
import ref_search as rs

KEYS = rfp.OUTS + ("n_found", "stats")


def _same(a, b, name=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (name, k, a[k], b[k])


def test_hand_cases_in_both_forms_and_their_written_answers():
    for name, c in fpc.hand_cases().items():
        r = rfp.reference(c)
        _same(r, rfp.second(c), name)
        assert fpc.found_of(r) == c["expect"], (name, fpc.found_of(r))
        if c["expect_stats"] is not None:
            assert np.array_equal(r["stats"], c["expect_stats"]), (name, r["stats"])


def test_every_hand_case_changes_under_a_plant_and_every_plant_is_caught():
    caught = {p: [] for p in rfp.PLANTS}
    for name, c in fpc.hand_cases().items():
        r = rfp.reference(c)
        for p in rfp.PLANTS:
            q = rfp.reference(c, plant=p)
            if any(not np.array_equal(r[k], q[k]) for k in KEYS):
                caught[p].append(name)
        assert name in fpc.INERT or any(name in v for v in caught.values()), name
    for name in fpc.INERT:
        assert not any(name in v for v in caught.values()) and not rfp.reference(fpc.hand_cases()[name])["stats"].any()
    assert "already_seen" in caught["skip_off"] and "holder_smaller" in caught["holder_largest"] and "holder_smaller" in caught["held_taken"]
    assert "order_c_then_i" in caught["order_ic"] and "found_stride_one_short" in caught["order_ic"]


def test_random_items_in_both_forms():
    for name, c in fpc.random_cases().items():
        r = rfp.reference(c)
        _same(r, rfp.second(c), name)
        s = r["stats"]
        print(f"{name}: tried {s[0]}, visible {s[1]}, proposing {s[2]}, found {s[3]}, with a holder {s[4]}")
        if c["n"] >= 255:
            assert s[0] >= s[1] > s[2] >= s[3] >= s[4] > 0, (name, s)
            assert len(set(zip(r["found_cam"], r["found_kp"]))) == s[3], "one point per keypoint"
            order = list(zip(r["found_cam"], r["found_point"]))
            assert order == sorted(order) and len(set(order)) == len(order)
            for p in rfp.PLANTS if "c9" in name else ():
                assert s[3] > s[4], (name, s)
                q = rfp.reference(c, plant=p)
                assert any(not np.array_equal(r[k], q[k]) for k in KEYS), (name, p)
        short = rfp.reference(dict(c, found_stride=max(int(s[3]) - 1, 1)))
        m = short["n_found"]
        assert m == min(max(int(s[3]) - 1, 1), int(s[3])) and short["stats"][5] == m and np.array_equal(short["stats"][:5], s[:5])
        assert all(np.array_equal(short[k], r[k][:m]) for k in rfp.OUTS)


# ------------------------------------------------------------------------------------------------ the scenes
def _scene_map(oracle, points):
    seed, ws = pc.first_world_scene(points)
    n = ws["n"]
    m = ref_map.PointMapModel(oracle, pc.SCENE_K, pc.SCENE_W, pc.SCENE_H, n)
    m.first_frame(ws["xy"][0], ws["desc"][0], oracle.kdtree_build_frame(ws["xy"][0]))
    for f in range(1, 6):
        p = ws["pairs"][f - 1]
        m.step(ws["xy"][f], ws["desc"][f], oracle.kdtree_build_frame(ws["xy"][f]), None, p["matches"], np.asarray(p["F"], np.float32))
    off, fr, kp = m.observations()
    return seed, ws, m.size, np.asarray(off, np.int32), np.asarray(fr, np.int32), np.asarray(kp, np.int32)


def scene_item(ws, size, off, fr, kp, two_passes=False, noise=None):
    """The item of one scene map with the scene's true geometry: -> (item dict as random_item's, ident_kp [cams](n,): the physical
    point behind every keypoint, ident_pt (points,): the physical point behind every map point).  noise: (rng, px, bits) moves every
    keypoint by N(0, px) and flips fewer than `bits` bits of every keypoint descriptor."""
    sc, n = ws["scene"], ws["n"]
    inv = [np.argsort(q) for q in ws["perm"]]
    xy, desc = [a.copy() for a in ws["xy"]], [d.copy() for d in ws["desc"]]
    R = [ws["Rwc"][f].T.reshape(9) for f in range(6)]
    T = [-(ws["Rwc"][f].T @ sc["centres"][f]) for f in range(6)]
    ident_pt = np.array([inv[fr[off[i]]][kp[off[i]]] for i in range(size)])
    off, fr, kp = off[:size + 1].copy(), fr[:off[size]].copy(), kp[:off[size]].copy()
    if two_passes:
        rng = np.random.default_rng(4242)
        again = [rng.permutation(n) for _ in range(6)]                  # keypoint k of frame f is keypoint again[f][k] of frame 6 + f
        for f in range(6):
            a, d = np.zeros_like(xy[f]), np.zeros_like(desc[f])
            a[again[f]], d[again[f]] = xy[f], desc[f]
            xy.append(a)
            desc.append(d)
            q = np.zeros(n, np.int64)
            q[again[f]] = inv[f]
            inv.append(q)
        R, T = R + R, T + T
        fr2, kp2 = fr + 6, np.array([again[f][k] for f, k in zip(fr, kp)], np.int32)
        off = np.concatenate([off, off[1:] + off[size]]).astype(np.int32)
        fr, kp = np.concatenate([fr, fr2]).astype(np.int32), np.concatenate([kp, kp2]).astype(np.int32)
        ident_pt = np.concatenate([ident_pt, ident_pt])
    obs_desc = np.stack([desc[f][k] for f, k in zip(fr, kp)])          # before any noise: what the map recorded
    if noise is not None:
        rng, px, bits = noise
        for f in range(len(xy)):
            xy[f] = (xy[f] + rng.normal(0, px, xy[f].shape)).astype(np.float32)
            desc[f] = np.stack([rs.flip_bits(rng, d, bits) for d in desc[f]])
    pts = np.ones((len(ident_pt), 4), np.float32)
    pts[:, :3] = sc["points"][ident_pt]
    item = dict(points=pts, n=len(pts), offsets=off, cam=fr, kp=kp, obs_desc=obs_desc, R=np.stack(R), T=np.stack(T), n_cams=len(R), xy=np.stack(xy),
                desc=np.stack(desc), n_kp=np.full(len(R), n, np.int32), cam_mask=None, K=pc.SCENE_K, width=pc.SCENE_W, height=pc.SCENE_H)
    return item, inv, ident_pt


def one_round(item, ident_kp, ident_pt):
    """fuse_item, then one geometric round on the survivors with true geometry, then the fusion over the lists with the extras
    appended -> (live after the fusion, live after the round, found, links, new observations, mixed groups, wrong pairs)"""
    P, Cs, Kp = item["n"], len(item["R"]), item["xy"].shape[1]
    O = len(item["cam"])
    first = rf.fuse_item(P, item["offsets"], item["cam"], item["kp"], Cs, Kp)
    idx = np.arange(P)
    live0 = int((first["fuse_to"] == idx).sum())
    merged = dict(item, points=rf.nan_rows(item["points"], np.flatnonzero(first["fuse_to"] != idx)), offsets=first["out_offsets"],
                  cam=first["out_cam"], kp=first["out_kp"], obs_desc=item["obs_desc"][first["out_src"]])
    r = rfp.reference(merged)
    extras = np.stack([r["found_point"], r["found_cam"], r["found_kp"]], 1)
    o2, f2, k2, _ = rfp.merge_extras(P, item["offsets"], item["cam"], item["kp"], extras, O + len(extras))
    after = rf.fuse_item(P, o2, f2, k2, Cs, Kp, first["fuse_to"])
    live1 = int((after["fuse_to"] == idx).sum())
    groups = {}
    for i in range(P):
        groups.setdefault(int(after["fuse_to"][i]), set()).add(int(ident_pt[i]))
    mixed = sum(len(g) > 1 for g in groups.values())
    wrong = sum(int(ident_kp[c][k]) != int(ident_pt[i]) for i, c, k in extras)
    links = int((r["found_holder"] >= 0).sum())
    return live0, live1, len(extras), links, len(extras) - links, mixed, wrong


@pytest.mark.parametrize("points,physical", [(60, 21), (400, 139)])
def test_one_round_on_the_scene_maps_leaves_one_point_per_physical_point(oracle, points, physical):
    seed, ws, size, off, fr, kp = _scene_map(oracle, points)
    for label, two in (("six frames", False), ("two passes", True)):
        item, ident_kp, ident_pt = scene_item(ws, size, off, fr, kp, two_passes=two)
        live0, live1, found, links, fresh, mixed, wrong = one_round(item, ident_kp, ident_pt)
        print(f"{label}, {points} (seed {seed}): {item['n']} map points, {len(set(ident_pt))} physical; live after the fusion {live0}, after one "
              f"geometric round {live1}; found {found} = {links} links + {fresh} new observations; mixed groups {mixed}, wrong pairs {wrong}")
        assert mixed == 0, "no group mixes two physical points"
        assert wrong == 0, "no found pair names a keypoint of another physical point"
        assert len(set(ident_pt)) == physical
        assert live1 == physical, "one live point per physical point after one round"
        assert live1 < live0
    item, ident_kp, ident_pt = scene_item(ws, size, off, fr, kp, two_passes=True, noise=(np.random.default_rng(seed), 0.5, 21))
    live0, live1, found, links, fresh, mixed, wrong = one_round(item, ident_kp, ident_pt)
    print(f"two passes, {points}, 0.5 px and up to 20 bits of noise: live {live0} -> {live1} ({physical} physical); found {found} = {links} links + "
          f"{fresh} new observations; mixed groups {mixed}, wrong pairs {wrong}")
    assert mixed == 0 and wrong == 0


def test_merge_extras_appends_in_order_and_admits_a_prefix():
    off, fr, kp = np.array([0, 2, 2, 3, 3], np.int32), np.array([0, 1, 4], np.int32), np.array([5, 6, 7], np.int32)
    extras = [(2, 8, 1), (0, 9, 2), (0, 7, 3), (1, 6, 4)]
    o, f, k, s = rfp.merge_extras(3, off, fr, kp, extras, 16)
    assert o.tolist() == [0, 4, 5, 7, 7] and f.tolist() == [0, 1, 9, 7, 6, 4, 8] and k.tolist() == [5, 6, 2, 3, 4, 7, 1]
    assert s.tolist() == [0, 1, 17, 18, 19, 2, 16]
    o, f, k, s = rfp.merge_extras(3, off, fr, kp, extras, 5)      # room for two
    assert o.tolist() == [0, 3, 3, 5, 5] and s.tolist() == [0, 1, 6, 2, 5]
    o, f, k, s = rfp.merge_extras(3, off, fr, kp, extras, 3)      # room for none
    assert o.tolist() == off.tolist() and s.tolist() == [0, 1, 2]
