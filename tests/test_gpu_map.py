"""The device-resident PointMap (vslam_map_* / vslam_track_sequences) against tests/ref_map.py, the plain Python restatement
of the reference's loop: BIT-EXACT on every array of the view -- points, colours, sizes, per-frame map_point_ids, R_t, pose --
and on the observation lists in the reference's push order.  The model's numeric stages are the CPU oracle's, so nothing here
has a tolerance."""
import numpy as np
import pytest
import torch

import ref_map
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu

MAXC, KP, HYP, THR = 400, 448, 256, 10.0     # kp_stride above every frame's count
TRACKS, FRAMES = 3, 6
# (seed, width, height, row padding in bytes): the second has a width that is no multiple of 4 and padded rows
SHAPES = [(2, 320, 240, 0), (3, 322, 200, 10)]


def _K(w, h):
    return np.array([[525, 0, w // 2], [0, 525, h // 2], [0, 0, 1]], np.float32)     # src/vslam.cpp:32


def _seeds(seed):
    return (np.arange(TRACKS * (FRAMES - 1), dtype=np.uint32).reshape(TRACKS, FRAMES - 1) * 7919 + seed * 100003).astype(np.uint32)


_MODELS = {}


def _scene(oracle, shape, **caps):
    """(bgr (T, F, H, W, 3), seeds, [model per track]) -- the models are cached per (shape, capacities)."""
    seed, w, h, _ = shape
    key = (shape, tuple(sorted(caps.items())))
    if key not in _MODELS:
        bgr = synth.sequences_numpy(seed, TRACKS, FRAMES, w, h)
        seeds = _seeds(seed)
        pat = synth.brief_pattern()
        ca, sa = synth.keypoint_rotation()
        models = [ref_map.run_track(oracle, bgr[t], seeds[t], _K(w, h), MAXC, ca, sa, pat, HYP, THR, kp_stride=KP, **caps)
                  for t in range(TRACKS)]
        _MODELS[key] = (bgr, seeds, models)
    return _MODELS[key]


def _device_bgr(bgr, pad):
    T, Fr, H, W, _ = bgr.shape
    if not pad:
        return torch.from_numpy(bgr).cuda(), None
    rows = np.full((T, Fr, H, 3 * W + pad), 0xA5, np.uint8)
    rows[..., :3 * W] = bgr.reshape(T, Fr, H, 3 * W)
    return torch.from_numpy(rows).cuda(), W


def _track(ctx, pmap, shape, bgr, seeds, out=None):
    _, w, h, pad = shape
    d_bgr, width = _device_bgr(bgr, pad)
    pat = torch.from_numpy(synth.brief_pattern()).cuda()
    ca, sa = synth.keypoint_rotation()
    d_seeds = torch.from_numpy(seeds.view(np.int32).copy()).cuda()
    return ctx.track_sequences(pmap, d_bgr, MAXC, ca, sa, pat, d_seeds, HYP, THR, _K(w, h), out=out, width=width)


def _state(pmap):
    off, fr, pt = pmap.observations()
    v = pmap.view()
    v["offsets"], v["obs_frames"], v["obs_points"] = off.cpu().numpy(), fr.cpu().numpy(), pt.cpu().numpy()
    return v


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare(v, models, frames, tracks=None):
    for t, m in enumerate(models):
        if tracks is not None and t not in tracks:
            continue
        tag = f"track {t}"
        print(f"{tag}: size {m.size}, observations {sum(len(x) for x in m.frame_ids)}, stats {m.stats}")
        assert v["sizes"][t] == m.size, tag
        assert np.array_equal(_bits(v["points"][t, :m.size]), _bits(m.points[:m.size])), tag
        assert not v["points"][t, m.size:].any(), tag
        assert np.array_equal(v["colors"][t, :m.size], np.array(m.colors, np.uint8).reshape(-1, 3)), tag
        for f in range(frames):
            fr = m.frames[f]
            assert np.array_equal(v["map_point_ids"][t, f], fr.map_point_ids), (tag, f)
            assert np.array_equal(_bits(v["R_t"][t, f]), _bits(fr.R_t).reshape(16)), (tag, f)
            assert np.array_equal(_bits(v["pose"][t, f]), _bits(fr.pose).reshape(16)), (tag, f)
        offs, ofr, opt = m.observations()
        total = int(offs[-1])
        assert v["n_obs"][t] == total, tag
        assert np.array_equal(v["offsets"][t, :m.size + 1], offs), tag
        assert (v["offsets"][t, m.size:] == total).all(), tag
        assert np.array_equal(v["obs_frames"][t, :total], ofr), tag
        assert np.array_equal(v["obs_points"][t, :total], opt), tag
        assert np.array_equal(v["obs_counts"][t, :m.size], np.diff(offs)), tag


def _needs(models):
    return max(m.size for m in models), max(sum(len(x) for x in m.frame_ids) for m in models)


@pytest.mark.parametrize("shape", SHAPES, ids=["320x240", "322x200_padded"])
def test_track_sequences_bit_exact(ctx, oracle, shape):
    bgr, seeds, models = _scene(oracle, shape)
    # non-vacuity, on the model's side: the scenes exercise every branch of the bookkeeping
    st = [m.stats for m in models]
    assert sum(s["propagation_pushes"] for s in st) >= 1 and sum(s["association_claims"] for s in st) >= 1
    assert max(len(x) for m in models for x in m.frame_ids) >= 3
    assert sum(s["colors_outside"] for s in st) >= 1 and sum(s["colors_inside"] for s in st) >= 1
    assert any(all(g > 0 for g in s["growth"][i:i + 3]) for s in st for i in range(len(s["growth"]) - 2))
    M, O = _needs(models)
    pmap = capi.PointMap(ctx, TRACKS, FRAMES, KP, M + 5, O + 7)
    try:
        _track(ctx, pmap, shape, bgr, seeds)
        ctx.synchronize()
        _compare(_state(pmap), models, FRAMES)
    finally:
        pmap.close()


def test_capacity_is_reported_and_nothing_partial(ctx, oracle):
    shape = SHAPES[0]
    bgr, seeds, full = _scene(oracle, shape)
    M, O = _needs(full)
    for caps in (dict(map_capacity=M - 1, obs_capacity=O + 7), dict(map_capacity=M + 5, obs_capacity=O - 1)):
        _, _, models = _scene(oracle, shape, **caps)
        assert 1 <= sum(m.overflowed > 0 for m in models) < TRACKS, "one short: some track overflows, some do not"
        pmap = capi.PointMap(ctx, TRACKS, FRAMES, KP, caps["map_capacity"], caps["obs_capacity"])
        try:
            _track(ctx, pmap, shape, bgr, seeds)
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
                ctx.synchronize()
            _compare(_state(pmap), models, FRAMES)
            ctx.synchronize()                       # the word was cleared
            # the SAME map after the dropped steps: reset + rerun is exact again (no per-step state survives a reset)
            pmap.reset()
            ctx.synchronize()
            empty = pmap.view()
            assert not empty["sizes"].any() and not empty["n_obs"].any() and (empty["map_point_ids"] == -1).all()
            assert not empty["points"].any() and not empty["colors"].any() and not empty["obs_counts"].any()
            _track(ctx, pmap, shape, bgr, seeds)
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
                ctx.synchronize()
            _compare(_state(pmap), models, FRAMES)
        finally:
            pmap.close()
    # max_frames one short: the last step does nothing to any track
    _, _, models = _scene(oracle, shape, max_frames=FRAMES - 1)
    pmap = capi.PointMap(ctx, TRACKS, FRAMES - 1, KP, M + 5, O + 7)
    try:
        _track(ctx, pmap, shape, bgr, seeds)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            ctx.synchronize()
        _compare(_state(pmap), models, FRAMES - 1)
    finally:
        pmap.close()
    # the same context, a map that fits: exact again
    pmap = capi.PointMap(ctx, TRACKS, FRAMES, KP, M + 5, O + 7)
    try:
        _track(ctx, pmap, shape, bgr, seeds)
        ctx.synchronize()
        _compare(_state(pmap), full, FRAMES)
    finally:
        pmap.close()


def _frame_batches(out, f):
    """Frame f / pair f - 1 -> f of every track as [tracks][...] batches, from the flattened outputs of track_sequences."""
    def per_frame(a):
        return a.view(TRACKS, FRAMES, *a.shape[1:])[:, f].contiguous()

    def per_pair(a):
        full = torch.cat([a, torch.zeros_like(a[:1])])      # tracks * frames - 1 slots -> tracks * frames
        return full.view(TRACKS, FRAMES, *a.shape[1:])[:, f - 1].contiguous()
    frame = {k: per_frame(out[k]) for k in ("xy", "desc", "nodes", "n")}
    pair = {k: per_pair(out[k]) for k in ("matches", "best", "F")} if f > 0 else None
    return frame, pair


def test_reset_rerun_and_interleaved_maps_identical(ctx, oracle):
    shape = SHAPES[0]
    _, w, h, _ = shape
    bgr, seeds, models = _scene(oracle, shape)
    M, O = _needs(models)
    a = capi.PointMap(ctx, TRACKS, FRAMES, KP, M + 5, O + 7)
    b = capi.PointMap(ctx, TRACKS, FRAMES, KP, M + 5, O + 7)
    try:
        out = _track(ctx, a, shape, bgr, seeds)
        ctx.synchronize()
        first = _state(a)
        _track(ctx, a, shape, bgr, seeds)          # resets the map itself
        ctx.synchronize()
        second = _state(a)
        for k in first:
            assert np.array_equal(np.asarray(first[k]), np.asarray(second[k])), k
        # vslam_map_step on two maps of one context, interleaved step by step, from the same per-frame batches
        a.reset(); b.reset()
        d_bgr = torch.from_numpy(bgr).cuda()
        last, _ = _frame_batches(out, 0)
        for f in range(1, FRAMES):
            cur, pair = _frame_batches(out, f)
            img = d_bgr[:, f].contiguous()
            a.step(last, cur, pair, img, _K(w, h))
            b.step(last, cur, pair, img, _K(w, h))
            last = cur
        ctx.synchronize()
        sa, sb = _state(a), _state(b)
        for k in first:
            assert np.array_equal(np.asarray(sa[k]), np.asarray(first[k])), k
            assert np.array_equal(np.asarray(sb[k]), np.asarray(first[k])), k
    finally:
        a.close(); b.close()


def test_map_step_directed(ctx, oracle):
    """vslam_map_step fed hand-edited ids and matches, with tracks of different sizes in one call: track 0 -- last-frame ids
    0 (never propagated), 1, 2 and a duplicate, two matches onto one m.second (the later wins the id, both push, a map point
    pushed twice in one step); track 1 -- no RANSAC winner; track 2 -- untouched data; track 3 -- an empty map and then n = 0
    keypoints.  (A current-frame keypoint HOLDING id 0: test_sixteen_candidate_flag_and_id_zero_through_map_step.)"""
    shape = SHAPES[0]
    _, w, h, _ = shape
    T = 4
    bgr, seeds, _ = _scene(oracle, shape)
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    K = _K(w, h)
    src = [0, 1, 2, 0]                                           # which scene track feeds each map track
    feats = [[oracle.extract_features(bgr[s][f], MAXC, ca, sa, pat) for f in range(3)] for s in src]
    refs = [[oracle.match_features(feats[t][f]["xy"], feats[t][f]["desc"], feats[t][f + 1]["xy"], feats[t][f + 1]["desc"],
                                   int(seeds[src[t]][f]), HYP, THR) for f in range(2)] for t in range(T)]
    models = [ref_map.PointMapModel(oracle, K, w, h, KP) for _ in range(T)]
    for t in range(T):
        models[t].first_frame(feats[t][0]["xy"], feats[t][0]["desc"], feats[t][0]["nodes"], bgr[src[t]][0])
    pmap = capi.PointMap(ctx, T, 3, KP, 2 * MAXC, 8 * MAXC)

    def batch(f, edit=None):
        fr = dict(xy=np.zeros((T, KP, 2), np.float32), desc=np.zeros((T, KP, 32), np.uint8), nodes=np.full((T, KP), -1, np.int32),
                  n=np.zeros(T, np.int32))
        for t in range(T):
            ft = feats[t][f]
            n = 0 if (edit and edit.get("empty") == t) else ft["n"]
            fr["xy"][t, :n], fr["desc"][t, :n], fr["nodes"][t, :n], fr["n"][t] = ft["xy"][:n], ft["desc"][:n], ft["nodes"][:n], n
        return {k: torch.from_numpy(v).cuda() for k, v in fr.items()}

    def pair_batch(matches, Fs, winners):
        p = dict(matches=np.zeros((T, KP, 2), np.int32), best=np.zeros((T, 4), np.int32), F=np.zeros((T, 9), np.float32))
        for t in range(T):
            k = len(matches[t])
            p["matches"][t, :k] = matches[t]
            p["best"][t] = (winners[t], k, 0, k)
            p["F"][t] = Fs[t]
        return {k: torch.from_numpy(v).cuda() for k, v in p.items()}

    try:
        # step 1: plain, except track 1 (no winner) -- track 3's map stays empty through it by having no matches kept
        m1 = [refs[t][0]["matches"] for t in range(T)]
        m1[3] = m1[3][:0]
        win = [0, -1, 0, 0]
        img = torch.from_numpy(np.stack([bgr[s][1] for s in src])).cuda()
        pmap.step(batch(0), batch(1), pair_batch(m1, [refs[t][0]["F"] for t in range(T)], win), img, K)
        for t in range(T):
            ft = feats[t][1]
            models[t].step(ft["xy"], ft["desc"], ft["nodes"], bgr[src[t]][1], m1[t], refs[t][0]["F"], has_model=win[t] >= 0)
        ctx.synchronize()
        v = pmap.view()
        assert v["sizes"][1] == 0 and v["sizes"][3] == 0 and v["sizes"][0] == models[0].size > 8
        # hand-edit frame 1's ids of track 0 on both sides: ids 0, 1, 2 and a duplicate on the first matches' keypoints
        m2 = [refs[t][1]["matches"].copy() for t in range(T)]
        k0 = m2[0][:4, 0]
        ids1 = models[0].frames[1].map_point_ids
        ids1[k0] = (0, 1, 2, 2)
        m2[0][2, 1] = m2[0][1, 1]                       # matches 1 and 2 onto one m.second: match 2's id wins
        row = np.ascontiguousarray(ids1, np.int32)
        a = pmap.arrays()
        ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, capi.C.c_void_p(a.d_map_point_ids + 4 * (0 * 3 + 1) * KP),
                                          capi.C.c_void_p(row.ctypes.data), capi.C.c_size_t(4 * KP)))
        win = [0, 0, 0, 0]
        img = torch.from_numpy(np.stack([bgr[s][2] for s in src])).cuda()
        pmap.step(batch(1), batch(2, edit=dict(empty=3)), pair_batch(m2[:3] + [m2[3][:0]], [refs[t][1]["F"] for t in range(T)], win),
                  img, K)
        for t in range(3):
            ft = feats[t][2]
            models[t].step(ft["xy"], ft["desc"], ft["nodes"], bgr[src[t]][2], m2[t], refs[t][1]["F"])
        models[3].step(np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32), bgr[src[3]][2],
                       np.zeros((0, 2), np.int32), refs[3][1]["F"])
        ctx.synchronize()
        f2 = models[0].frames[2]
        assert f2.map_point_ids[m2[0][1, 1]] == 2               # the later of the two matches won
        assert models[0].frame_ids[1][2:3] == [2] and models[0].frame_ids[2][2:4] == [2, 2]   # every such match pushed
        assert models[0].stats["propagation_pushes"] == 3       # and the match whose last id was 0 did not
        _compare(_state(pmap), models, 3)
    finally:
        pmap.close()


def _batches(T, feats, f):
    fr = dict(xy=np.zeros((T, KP, 2), np.float32), desc=np.zeros((T, KP, 32), np.uint8), nodes=np.full((T, KP), -1, np.int32),
              n=np.zeros(T, np.int32))
    for t in range(T):
        ft = feats[t][f]
        n = ft["n"]
        fr["xy"][t, :n], fr["desc"][t, :n], fr["nodes"][t, :n], fr["n"][t] = ft["xy"], ft["desc"], ft["nodes"], n
    return {k: torch.from_numpy(v).cuda() for k, v in fr.items()}


def _pair_batches(T, refs, f):
    p = dict(matches=np.zeros((T, KP, 2), np.int32), best=np.zeros((T, 4), np.int32), F=np.zeros((T, 9), np.float32))
    for t in range(T):
        k = len(refs[t][f]["matches"])
        p["matches"][t, :k] = refs[t][f]["matches"]
        p["best"][t] = (0, k, 0, k)
        p["F"][t] = refs[t][f]["F"]
    return {k: torch.from_numpy(v).cuda() for k, v in p.items()}


def test_sixteen_candidate_flag_and_id_zero_through_map_step(ctx, oracle):
    """The association's 16-candidate cap still raises VSLAM_ERR_CAPACITY when it is reached through vslam_map_step, and the step
    is published all the same.  Track 0's third frame is edited by hand: 25 keypoints carrying map point I's descriptor are
    laid on a half-pixel grid around the pixel map point I projects to (25 acceptable hits within radius 2), and keypoint 0 is
    moved onto map point 0's projection with map point 0's descriptor, so that a current-frame keypoint HOLDS id 0 -- which the
    association treats as taken (>= 0) and the reprojection filter, reading ids at match index 0, does not (> 0).  Track 1 is
    untouched data."""
    shape = SHAPES[0]
    _, w, h, _ = shape
    T = 2
    bgr, seeds, _ = _scene(oracle, shape)
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    K = _K(w, h)
    feats = [[oracle.extract_features(bgr[t][f], MAXC, ca, sa, pat) for f in range(3)] for t in range(T)]
    refs = [[oracle.match_features(feats[t][f]["xy"], feats[t][f]["desc"], feats[t][f + 1]["xy"], feats[t][f + 1]["desc"],
                                   int(seeds[t][f]), HYP, THR) for f in range(2)] for t in range(T)]
    models = [ref_map.PointMapModel(oracle, K, w, h, KP) for _ in range(T)]
    for t in range(T):
        models[t].first_frame(feats[t][0]["xy"], feats[t][0]["desc"], feats[t][0]["nodes"], bgr[t][0])
        ft = feats[t][1]
        models[t].step(ft["xy"], ft["desc"], ft["nodes"], bgr[t][1], refs[t][0]["matches"], refs[t][0]["F"])
    # where the map points of track 0 land in frame 2 (float64 is enough: it only places the hand-made keypoints)
    m0 = models[0]
    R, tv = oracle.extract_Rt(refs[0][1]["F"], K)
    c2 = oracle.camera_matrix(K, R, tv).astype(np.float64)
    proj = m0.points[:m0.size].astype(np.float64) @ c2.T
    q = proj[:, :2] / proj[:, 2:3]
    inside = (q[:, 0] > 8) & (q[:, 0] < w - 8) & (q[:, 1] > 8) & (q[:, 1] < h - 8)
    assert inside[0], "map point 0 must project into the frame for the id-0 case"
    far = np.hypot(q[:, 0] - q[0, 0], q[:, 1] - q[0, 1]) > 10
    I = int(np.nonzero(inside & far & (np.arange(m0.size) > 0))[0][0])
    ft = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in feats[0][2].items()}
    n = ft["n"]
    assert n > 60
    grid = np.array([(dx, dy) for dx in (-1, -.5, 0, .5, 1) for dy in (-1, -.5, 0, .5, 1)], np.float32)
    ft["xy"][n - 25:n] = q[I].astype(np.float32) + grid
    ft["desc"][n - 25:n] = feats[0][0]["desc"][m0.frame_point_ids[I][0]]
    ft["xy"][0] = q[0].astype(np.float32)
    ft["desc"][0] = feats[0][0]["desc"][m0.frame_point_ids[0][0]]
    ft["nodes"] = oracle.kdtree_build_frame(ft["xy"])
    feats[0][2] = ft
    M, O = 4 * MAXC, 12 * MAXC
    pmap = capi.PointMap(ctx, T, 3, KP, M, O)
    try:
        for f in (1, 2):
            img = torch.from_numpy(np.stack([bgr[t][f] for t in range(T)])).cuda()
            pmap.step(_batches(T, feats, f - 1), _batches(T, feats, f), _pair_batches(T, refs, f - 1), img, K)
            if f == 1:
                ctx.synchronize()
        for t in range(T):
            g = feats[t][2]
            models[t].step(g["xy"], g["desc"], g["nodes"], bgr[t][2], refs[t][1]["matches"], refs[t][1]["F"])
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            ctx.synchronize()
        f2 = m0.frames[2]
        assert len(refs[0][1]["matches"]) > 0 and f2.map_point_ids[0] == 0        # a keypoint holds id 0, at a match index
        assert m0.frame_ids[0][-1] == 2 and m0.frame_point_ids[0][-1] == 0        # ... claimed by map point 0 in frame 2
        assert n - 25 <= m0.frame_point_ids[I][-1] < n and m0.frame_ids[I][-1] == 2   # map point I took one of its 25 hits
        _compare(_state(pmap), models, 3)                                          # the step was published, exactly
    finally:
        pmap.close()


def test_pipeline_ticket_reports_map_overflow(oracle):
    shape = SHAPES[0]
    bgr, seeds, full = _scene(oracle, shape)
    M, O = _needs(full)
    pipe = capi.Pipeline(0, n_ctx=2)
    try:
        statuses = []
        for cap in (M - 1, M + 5):
            ticket, c = pipe.acquire()
            pmap = capi.PointMap(c, TRACKS, FRAMES, KP, cap, O + 7)
            _track(c, pmap, shape, bgr, seeds)
            pipe.commit(ticket)
            statuses.append(pipe.wait_status(ticket)[0])
            if cap > M:
                _compare(_state(pmap), full, FRAMES)
            pmap.close()
        assert statuses == [-4, 0]                    # VSLAM_ERR_CAPACITY on the short map's ticket only
    finally:
        pipe.close()
