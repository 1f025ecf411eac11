"""What a call may find in its workspace.  Every stage takes its scratch from the context's grow-only arena, whose slots
are never cleared: a call runs on whatever the last user of a slot left there.  The rule: what a call writes is a function of its
arguments (and of the resident maps / worlds it is handed), never of the workspace.  Held here on the session's context, bit for bit:

  * every entry point that takes device memory (include/vslam_amd.h through tests/entry_calls.py, the five newer headers through
    tests/header_calls.py) runs FOUR times on the same arguments: as the suite's history left the arena; behind
    Context.workspace_fill(0); behind the same entry point on a second, same-shaped scene; behind another entry point (one that
    shares a slot with it where there is one, the next of a fixed shuffled order otherwise).  The return code, every compared output
    and in-out tensor and the state a Call exposes are equal across the four; entry_calls.run() holds the error word of
    vslam_ctx_synchronize to 0 behind every one of them.  Call.scratch outputs stay excluded, as everywhere.
  * the forms of a stage that the small scene does not reach (FORMS below), the same way, where the second stale predecessor is the
    same entry point at a LARGER shape: the real call then works in the front part of blocks whose rest holds the larger call's data.
  * the batch sizes at which a launch shape changes (vs_stream_segments, the corner pool's slots, the padded item grid), against the
    oracle for every copy of eight distinct frames.

Only zeros and in-range stale data are ever put into the workspace: a stale count of four billion is nothing a caller can meet.
The zeroed runs come first (test_zeroed_workspace); an entry point goes on to the stale runs only when its zeroed run held.
Nothing here has a tolerance."""
import os
import random
import re

import numpy as np
import pytest
import torch

import alignment_contract as ac
import entry_calls as ec
import header_calls as hc
from entry_calls import Call, Dbl, Fl, Hst, I, P
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = capi.Context
DEFAULTS = {OPT.OPT_CORNER_LIST_CAP: 0, OPT.OPT_RANSAC_ALL_SUMS: 0}
i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8

# Entry points with device-pointer arguments that are not held, and why: only what entry_calls.NOT_LAUNCHED already excuses.
NOT_HELD = {
    "vslam_dev_free": "takes back an allocation: no workspace",
    "vslam_copy_h2d": "hipMemcpy: no workspace",
    "vslam_copy_d2h": "hipMemcpy: no workspace",
    "vslam_upload_async": "hipMemcpyAsync: no workspace",
    "vslam_download_async": "hipMemcpyAsync: no workspace",
    "vslam_pipeline_submit_pairs": "runs on the pipeline's own contexts (a pipeline makes contexts and streams); the wrapper around vslam_frontend_pairs, which is held",
    "vslam_pipeline_submit_pairs_pose": "the same wrapper around vslam_frontend_pairs_pose, which is held",
    "vslam_pipeline_submit_sequence": "the same wrapper around vslam_frontend_sequence, which is held",
    "vslam_multi_frontend_pairs": "host images; one context per device inside vslam_multi",
    "vslam_multi_frontend_pairs_resident": "one host thread and context per device inside vslam_multi, around vslam_frontend_pairs, which is held",
    "vslam_gather_records": "needs an RCCL communicator; no workspace",
    "vslam_gather_records_v": "needs an RCCL communicator; no workspace",
}
HELD = ec.ENTRIES + hc.ENTRIES

# The stale predecessor from another entry point: one that writes a slot the entry point reads where there is one (the search and the
# match share corr_keys / corr_prop; the image stages extract.* / gf.* / stage.*; vslam_match_features and vslam_ransac_* the mf.* and
# ransac.* blocks; the renderers render.keys; ...), the others follow a fixed shuffled order (_other_entry).
SHARES_A_SLOT_WITH = {
    "vslam_search_projection": "vslam_match_points", "vslam_match_points": "vslam_search_projection",
    "vslam_world_search": "vslam_world_relocalise", "vslam_world_relocalise": "vslam_pnp_ransac", "vslam_pnp_ransac": "vslam_world_relocalise",
    "vslam_extract_features": "vslam_good_features", "vslam_good_features": "vslam_extract_features", "vslam_gaussian7": "vslam_extract_features",
    "vslam_min_eigen": "vslam_good_features", "vslam_orb_describe": "vslam_extract_features", "vslam_bgr2gray": "vslam_extract_features",
    "vslam_match_features": "vslam_ransac_fundamental", "vslam_ransac_fundamental": "vslam_match_features",
    "vslam_ransac_evaluate": "vslam_match_features", "vslam_ransac_solve": "vslam_match_features", "vslam_ransac_sets": "vslam_frontend_pairs",
    "vslam_match_knn2_ratio": "vslam_match_features",
    "vslam_frontend_pairs": "vslam_frontend_sequence", "vslam_frontend_sequence": "vslam_frontend_pairs_pose",
    "vslam_frontend_pairs_pose": "vslam_track_sequences", "vslam_track_sequences": "vslam_frontend_pairs",
    "vslam_map_step": "vslam_associate_map_points", "vslam_associate_map_points": "vslam_map_step",
    "vslam_reprojection_filter": "vslam_frontend_pairs_pose", "vslam_refine_pairs": "vslam_frontend_pairs_pose",
    "vslam_render_points": "vslam_map_render", "vslam_map_render": "vslam_world_render", "vslam_world_render": "vslam_render_points",
    "vslam_adjust_windows": "vslam_world_adjust", "vslam_world_adjust": "vslam_adjust_windows",
    "vslam_fuse_points": "vslam_world_fuse", "vslam_world_fuse": "vslam_fuse_points",
    "vslam_cull_points": "vslam_world_cull", "vslam_world_cull": "vslam_cull_points",
    "vslam_world_observations": "vslam_world_fuse", "vslam_map_observation_descriptors": "vslam_world_observations",
    "vslam_map_observations": "vslam_world_observations", "vslam_resect_poses": "vslam_world_search", "vslam_world_step_resect": "vslam_resect_poses",
    "vslam_extract_features_grid": "vslam_extract_features",
}


def _other_entry(entry):
    if entry in SHARES_A_SLOT_WITH:
        return SHARES_A_SLOT_WITH[entry]
    order = sorted(HELD)
    random.Random(20261020).shuffle(order)
    return order[(order.index(entry) + 1) % len(order)]


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


# ----------------------------------------------------------------------------------------------------------------- the runs
class Held:
    """One call held: `real`, its stale predecessors [(label, Call, options)], the context options it runs under, and `check(ctx, got)`,
    which asserts that the run reached the form it is there for."""

    def __init__(self, real, preds, opts=None, check=None):
        self.real, self.preds, self.opts, self.check = real, preds, dict(opts or {}), check


def _run(ctx, call, opts):
    try:
        for o, v in opts.items():
            ctx.set_option(o, v)
        rc, msg, got, _ = ec.run(ctx, call)
    finally:
        for o in opts:
            ctx.set_option(o, DEFAULTS[o])
    return rc, msg, ec.canonical(call.entry, got)


def _hold_equal(name, what, first, got):
    assert got[0] == first[0], (name, what, "return code", got[0], got[1])
    diff = ec._same(first[2], got[2])
    assert set(first[2]) == set(got[2]) and not diff, f"{name}: {what}: differs from the first run in {diff}"


FIRST = {}      # name -> the first run, for the entries whose zeroed run held


def hold_zeroed(ctx, name, h):
    first = _run(ctx, h.real, h.opts)
    assert first[0] == 0, (name, first[1])
    if h.check:
        h.check(ctx, first[2])
    ctx.workspace_fill(0)
    _hold_equal(name, "behind a zeroed workspace", first, _run(ctx, h.real, h.opts))
    FIRST[name] = first


def hold_stale(ctx, name, h):
    assert name in FIRST, f"{name}: the zeroed run has not held (test_zeroed_workspace runs first); the stale runs are not made"
    for label, pred, opts in h.preds:
        rc, msg, _ = _run(ctx, pred, opts)
        assert rc == 0, (name, label, msg)
        _hold_equal(name, "behind " + label, FIRST[name], _run(ctx, h.real, h.opts))


# ------------------------------------------------------------------------------------------------- the calls of the six headers
class Table:
    def __init__(self):
        self.held, self.closers = {}, []


def _world_calls(ctx, tab):
    """The entry points that work on a world attached to a map: two maps of the same two exact scenes (test_gpu_pnp._scene_map), the
    tracks the other way round in the second, each fused once; every run starts from the state the fusion left (put back by `before`)."""
    import pnp_cases as pc
    from test_gpu_fuse import _xy_all
    from test_gpu_pnp import SCENE_KP, _put, _scene_map
    both = [pc.first_world_scene(60)[1], pc.first_world_scene(400)[1]]
    polish, resect = capi.ResectParams.make(ctx.lib), capi.ResectParams.make(ctx.lib)
    sides = []
    for scenes, f_cur, seed0, noise in ((both, 5, 1, 0), (both[::-1], 3, 50, 9)):
        a, wa, _ = _scene_map(ctx, scenes)
        tab.closers += [a.close, wa.close]
        wa.fuse(a)
        ctx.synchronize()
        start = a.view()
        fv = capi.C.c_void_p()
        ctx._check(ctx.lib.vslam_world_fusion_view(wa.handle, capi.C.byref(fv), capi.C.c_void_p(0)))

        def before(ctx=ctx, wa=wa, start=start, fv=fv):
            w = wa.arrays()
            for ptr, key in ((w.d_Twc, "world_Twc"), (w.d_pose, "world_pose"), (w.d_scale, "world_scale"), (w.d_links, "world_links"),
                             (w.d_carry, "world_carry"), (w.d_carry_index, "world_carry_index"), (w.d_world_points, "world_points"),
                             (fv.value, "world_fuse_to")):
                _put(ctx, ptr, start[key])
        T = len(scenes)
        xy, desc = np.zeros((T, SCENE_KP, 2), np.float32), np.zeros((T, SCENE_KP, 32), np.uint8)
        for t, ws in enumerate(scenes):
            xy[t, :ws["n"]], desc[t, :ws["n"]] = ws["xy"][f_cur], ws["desc"][f_cur]
        cur = dict(xy=_t(xy), desc=_t(desc), n=_t(np.array([ws["n"] for ws in scenes], np.int32)))
        xy_all = _xy_all(scenes)[0]
        if noise:
            xy_all[:, 2:] += np.random.default_rng(noise).uniform(-30, 30, xy_all[:, 2:].shape).astype(np.float32)
        xy_all = _t(xy_all)
        reloc = {"d_xy_cur": cur["xy"], "d_desc_cur": cur["desc"], "d_n_cur": cur["n"], "d_seeds": torch.arange(seed0, seed0 + T, dtype=i32).cuda()}
        K = pc.SCENE_K
        calls = [hc.world_search(wa, a, cur, K, pc.SCENE_W, pc.SCENE_H, resect, before, a.view),
                 hc.world_relocalise(wa, a, reloc, K, polish, before, a.view),
                 hc.world_adjust(wa, a, xy_all, 6, K, 8, before, a.view),
                 hc.world_fuse(wa, a, before, a.view), hc.world_cull(wa, a, xy_all, 6, K, before, a.view),
                 hc.world_observations(wa, a).replaced(before=before), hc.map_observation_descriptors(a).replaced(before=before)]
        sides.append({c.entry: c for c in calls})
    return sides


def _step_resect_calls(ctx, tab):
    import ref_resect as rr
    from test_gpu_resect import FRAMES, KM, KP, _args, _pair_batch
    out = []
    for seeds in ((1, 2), (3, 4)):
        scenes = [rr.scene_inputs(seeds[0], outliers=0.0), rr.scene_inputs(seeds[1], outliers=0.2)]
        world = capi.World(ctx, 2, FRAMES, KP)
        world.set_resection()
        tab.closers.append(world.close)
        led = [_pair_batch([sc["pairs"][f] for sc in scenes]) for f in range(3)]

        def before(world=world, led=led):      # two steps in front, so that the third resects against a carry
            world.reset()
            for b in led[:2]:
                world.step(*_args(b))
        out.append(hc.world_step_resect(world, led[2], KM, before, world.view))
    return out


def _item_calls(ctx):
    """-> [{entry: Call}] twice: the batched entry points of the newer headers on the items their own tests use, and a second seed"""
    import pnp_cases as pc
    import ref_adjust as ra
    import ref_fuse as rf
    import ref_pnp as rp
    import ref_resect as rr
    import ref_search as rs
    from test_gpu_adjust import _batch as adjust_batch, _item as adjust_item
    from test_gpu_fuse import _cull_batch
    from test_gpu_pnp import _match_tensors, _tensors
    from test_gpu_resect import _batch as resect_batch
    from test_gpu_search import _cuda
    planted = [rs.planted_scene(s) for s in (1, 2)]
    sb = rs.batch_of(planted)
    structs = (capi.PnpParams.make(ctx.lib), capi.ResectParams.make(ctx.lib))
    fuse = [rf.random_fuse_item(61, 600, kp_stride=300), rf.random_fuse_item(62, 600, kp_stride=300)]
    O = max(len(it["cam"]) for it in fuse)
    cull = [rf.random_cull_item(71, 600, 6), rf.random_cull_item(72, 600, 6)]
    cb = _cull_batch(cull)
    sides = []
    for i in range(2):
        pnp = pc.case(rp.planted(300, 0.5, 5 + i), seed=5 + i)
        rP, rx, rn, rR, rT = resect_batch([rr.item(257, 13 + 4 * i, 0.2, 0.3)], 300)
        pr = ra.problem(24 + 3 * i, 8, 257, outliers=0.2, noise_px=0.3)
        it = fuse[i]
        fb = rf.batch_fuse([dict(it, cam=np.concatenate([it["cam"], np.zeros(O - len(it["cam"]), np.int32)]),
                                 kp=np.concatenate([it["kp"], np.zeros(O - len(it["kp"]), np.int32)]))])
        calls = [hc.search_projection(_cuda({k: v[i:i + 1] for k, v in sb.items()}), planted[0]["K"], 640, 480),
                 hc.match_points(_match_tensors(pc.match_case(2 + 4 * i, 300, (1, 4), 257), 900)),
                 hc.pnp_ransac(_tensors(pnp), pnp["K"], *structs),
                 hc.resect_poses(rP, rx, rn, rR, rT, rr.kmat()),
                 hc.adjust_windows(adjust_batch([adjust_item(pr)], 8, 300, 2400), ra.kmat()),
                 hc.fuse_points({k: _t(v) for k, v in fb.items()}, 6, 300),
                 hc.cull_points({k: _t(v[i:i + 1]) for k, v in cb.items()}, cull[i]["K"])]
        sides.append({c.entry: c for c in calls})
    return sides


# -------------------------------------------------------------------------------------------------------------------- FORMS
def _gray(seed, frames, w, h):
    return np.ascontiguousarray(synth.frames_numpy(seed, (frames + 1) // 2, w, h)[:frames, :, :, 1])


def _gf(g, maxc, kp):
    g = _t(g)
    F_, H_, W_ = g.shape
    return Call("vslam_good_features", [P("d_gray"), I(F_), I(W_), I(H_), I(maxc), Dbl(0.01), Dbl(3.0), I(kp), P("d_xy"), P("d_n")],
                ins={"d_gray": g}, outs={"d_xy": ((F_, kp, 2), f32), "d_n": ((F_,), i32)})


def _plateaus(h, w, cell, blobs):
    """test_good_features_tiny_max_corners_forces_slow_path's frames at any size: a checkerboard, blobs beside each other, noise"""
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy // cell) + (xx // cell)) % 2 * 200 + 20).astype(np.uint8)
    spots = np.full((h, w), 30, np.uint8)
    for cy, cx in blobs:
        spots[cy:cy + 3, cx:cx + 3] = 220
    return np.stack([board, spots, _gray(77 + cell, 1, w, h)[0]])


def _refine(c, Kp):
    import ref_refine as rr
    xy1, xy2, matches, best, R, t, P4 = c
    argv = [P("d_xy1"), P("d_xy2"), P("d_matches"), P("d_best"), I(1), I(Kp), Hst("h_K"), Fl(rr.GATE_SQ), I(rr.MAX_ITERATIONS), P("d_R"), P("d_t"),
            P("d_c2"), P("d_points4d"), P("d_stats")]
    return Call("vslam_refine_pairs", argv,
                ins={"d_xy1": _t(xy1[None], np.float32), "d_xy2": _t(xy2[None], np.float32), "d_matches": _t(matches[None], np.int32),
                     "d_best": _t(np.asarray(best)[None], np.int32)},
                inouts={"d_R": _t(np.asarray(R).reshape(1, 9), np.float32), "d_t": _t(np.asarray(t).reshape(1, 3), np.float32),
                        "d_points4d": _t(P4[None], np.float32)},
                outs={"d_c2": ((1, 12), f32), "d_stats": ((1, 4), f64)}, hosts={"h_K": np.ascontiguousarray(rr.KMAT, np.float32).reshape(9).copy()})


def _forms(ctx, scene, decoy, calls, decoys):
    import pnp_cases as pc
    import ref_fuse as rf
    import ref_pnp as rp
    import ref_refine as rr
    from test_gpu_fuse import _chain
    from test_gpu_pnp import _tensors
    forms = {}
    cap40 = {OPT.OPT_CORNER_LIST_CAP: 40}

    def same_form(real, second, larger, opts=None, check=None):
        return Held(real, [("the same call on a second seed", second, opts or {}), ("a larger shape of the same entry point", larger, opts or {})],
                    opts, check)

    def pool_ran(ctx, got):
        st = ctx.corner_stats()
        assert 1 <= st["frames_overflowed"] <= st["pool_sets"] == 4, st     # frames that list more than 40 pixels are redone from the pool
        assert (np.frombuffer(got["d_n"].tobytes(), np.int32) > 0).all()

    def corners(ctx, got):
        assert (np.frombuffer(got["d_n"].tobytes(), np.int32) > 0).all()
    forms["good_features: the pool fallback (corner list cap 40)"] = same_form(
        _gf(_gray(35, 4, 128, 96), 60, 64), _gf(_gray(47, 4, 128, 96), 60, 64), _gf(_gray(35, 4, 160, 120), 60, 64), cap40, pool_ran)
    forms["good_features: the plain pipeline (61 columns)"] = same_form(
        _gf(_gray(35, 4, 61, 48), 20, 32), _gf(_gray(47, 4, 61, 48), 20, 32), _gf(_gray(35, 4, 63, 90), 20, 32), check=corners)
    forms["good_features: padded rows (131 columns)"] = same_form(
        _gf(_gray(35, 4, 131, 96), 60, 64), _gf(_gray(47, 4, 131, 96), 60, 64), _gf(_gray(35, 4, 150, 110), 60, 64), check=corners)
    blobs = [(30, 40), (30, 44), (34, 40), (80, 100), (80, 103), (60, 20)]
    forms["good_features: the per-pixel state map (3 corners on plateaus)"] = same_form(
        _gf(_plateaus(120, 160, 8, blobs), 3, 3), _gf(_plateaus(120, 160, 10, [(y + 7, x + 5) for y, x in blobs]), 3, 3),
        _gf(_plateaus(150, 200, 8, blobs), 3, 3))

    def full(n):
        def check(ctx, got):
            assert n - 2 <= np.frombuffer(got["d_stats"].tobytes(), np.float64)[0] <= n       # the pair is full to the seam
        return check
    seam = {n: _refine(rr.case(rr.SHAPE_SEEDS[(4096, n)], 4096, n), 4096) for n in (3200, 3201)}
    large = _refine(rr.case(rr.SHAPE_SEEDS[(8160, 8160)], 8160, 8160), 8160)
    forms["refine_pairs: n = 3200, the point state in LDS"] = same_form(seam[3200], seam[3201], large, check=full(3200))
    forms["refine_pairs: n = 3201, the point state in the arena"] = same_form(seam[3201], _refine(rr.case(771, 4096, 3201), 4096), large,
                                                                             check=full(3201))
    # VSLAM_OPT_RANSAC_ALL_SUMS on, and off behind a call that had it on; the larger shape is both scenes as one batch of four
    mf, dmf = calls["vslam_match_features"], decoys["vslam_match_features"]
    both = mf.replaced(argv=[I(2 * ec.PAIRS) if i == 6 else a for i, a in enumerate(mf.argv)],
                       ins={k: torch.cat([v, dmf.ins[k]]).contiguous() for k, v in mf.ins.items()},
                       outs={k: ((2 * s[0],) + tuple(s[1:]), dt) for k, (s, dt) in mf.outs.items()})
    sums = {OPT.OPT_RANSAC_ALL_SUMS: 1}
    forms["match_features: every hypothesis scored (ALL_SUMS)"] = same_form(mf, dmf, both, sums)
    forms["match_features: behind calls that scored every hypothesis"] = Held(
        mf, [("the second scene with ALL_SUMS on", dmf, sums), ("a batch of four with ALL_SUMS on", both, sums)])

    def fuse(c):
        b = rf.batch_fuse([c])
        return hc.fuse_points({k: (_t(v) if k != "mask" or c.get("mask") is not None else None) for k, v in b.items()}, c["cam_stride"], c["kp_stride"])

    def one_group(n):
        def check(ctx, got):
            assert np.frombuffer(got["d_stats"].tobytes(), np.int32).tolist() == [n, 1, n - 1, n + 1]      # several rounds on the cells
        return check
    ends = [x for pair in zip(range(150), range(299, 149, -1)) for x in pair]
    forms["fuse_points: a chain of 300, index 0 at the far end"] = same_form(
        fuse(_chain(list(range(299, -1, -1)))), fuse(_chain(ends)), fuse(_chain(list(range(699, -1, -1)))), check=one_group(300))

    def crowd(n, col):
        return dict(n=n, offsets=np.arange(0, 2 * n + 2, 2, dtype=np.int32), cam=np.tile([1, 0], n).astype(np.int32),
                    kp=np.stack([np.full(n, col), np.arange(n)], 1).reshape(-1).astype(np.int32), cam_stride=2, kp_stride=n, mask=None)
    forms["fuse_points: 1000 points in one cell"] = same_form(fuse(crowd(1000, 7)), fuse(crowd(1000, 9)), fuse(crowd(1500, 7)),
                                                              check=one_group(1000))

    # most hypotheses without a pose (collinear points: the empty pose slots still walk the count loop), behind calls
    # that left a pose with inliers in every slot
    def pnp(c):
        return hc.pnp_ransac(_tensors(c), c["K"], capi.PnpParams.make(ctx.lib, **c["params"]), None)

    def no_pose(ctx, got):
        assert np.frombuffer(got["d_winner"].tobytes(), np.int32)[0] == -1
    forms["pnp_ransac: collinear points, no hypothesis has a pose"] = same_form(
        pnp(pc.hand_cases()["collinear"][0]), pnp(pc.case(rp.planted(40, 0.5, 7), seed=7)),
        pnp(pc.case(rp.planted(300, 0.5, 8), seed=8, hypotheses=256)), check=no_pose)
    return forms


FORM_NAMES = ["good_features: the pool fallback (corner list cap 40)", "good_features: the plain pipeline (61 columns)",
              "good_features: padded rows (131 columns)", "good_features: the per-pixel state map (3 corners on plateaus)",
              "refine_pairs: n = 3200, the point state in LDS", "refine_pairs: n = 3201, the point state in the arena",
              "match_features: every hypothesis scored (ALL_SUMS)", "match_features: behind calls that scored every hypothesis",
              "fuse_points: a chain of 300, index 0 at the far end", "fuse_points: 1000 points in one cell",
              "pnp_ransac: collinear points, no hypothesis has a pose"]


@pytest.fixture(scope="module")
def table(ctx):
    assert torch.cuda.current_stream() == torch.cuda.default_stream()      # the session's context and stream: none is made here
    tab = Table()
    scene = ec.build_scene(ctx, ec.SEED)
    decoy = ec.decoy_scene(ctx)
    tab.closers += [lambda: ec.close_scene(scene), lambda: ec.close_scene(decoy)]
    real, other = ec.build_calls(ctx, scene), ec.build_calls(ctx, decoy)
    for side, more in zip((real, other), zip(_item_calls(ctx), _world_calls(ctx, tab), ({c.entry: c} for c in _step_resect_calls(ctx, tab)))):
        for m in more:
            side.update(m)
    for entry in HELD:
        tab.held[entry] = Held(real[entry], [("the same entry point on the second scene", other[entry], {}),
                                             ("another entry point, " + _other_entry(entry), real[_other_entry(entry)], {})])
    tab.held.update(_forms(ctx, scene, decoy, real, other))
    yield tab
    for close in tab.closers:
        close()


def test_every_entry_point_with_device_memory_is_held_or_accounted_for():
    """all six headers: an entry point with a device-pointer argument (d_*, or a struct that carries one) is in HELD or in NOT_HELD"""
    declared = {e for e, _, r in ac.CONTRACT if r != ac.HOST}
    newer = set()
    for header in ("vslam_search.h", "vslam_pnp.h", "vslam_resect.h", "vslam_adjust.h", "vslam_fuse.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for m in re.finditer(r"\b(vslam_[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
            if re.search(r"[A-Za-z0-9_]\s*\*\s*d_\w+", m.group(2)):      # a pointer to device memory (`type **d_x` hands a view out)
                newer.add(m.group(1))
    assert newer == set(hc.ENTRIES), sorted(newer ^ set(hc.ENTRIES))
    assert len(HELD) == len(set(HELD)) and not set(HELD) & set(NOT_HELD)
    assert set(HELD) | set(NOT_HELD) == declared | newer, sorted((set(HELD) | set(NOT_HELD)) ^ (declared | newer))
    assert set(NOT_HELD) <= set(ec.NOT_LAUNCHED), "only what entry_calls.NOT_LAUNCHED already excuses"
    assert all(_other_entry(e) in HELD and _other_entry(e) != e for e in HELD)
    assert sorted(FORM_NAMES) == sorted(set(FORM_NAMES))


def test_workspace_slots_and_fill(ctx, table):
    slots = ctx.workspace_slots()
    print("\n".join(f"{name:28s} {size:>12d}" for name, size in sorted(slots.items())))
    assert sum(slots.values()) == ctx.workspace_bytes() and "ctx.errflag" in slots and "gf.counts" in slots
    need = capi.C.c_size_t()
    small = capi.C.create_string_buffer(8)
    assert ctx.lib.vslam_ctx_workspace_slots(ctx.handle, small, capi.C.c_size_t(8), capi.C.byref(need)) == 0
    assert len(small.value) == 7 and need.value > 8, "cut to the buffer, NUL-terminated, the whole size reported"
    assert ctx.lib.vslam_ctx_workspace_slots(ctx.handle, None, capi.C.c_size_t(8), capi.C.byref(need)) == -1
    assert ctx.lib.vslam_ctx_workspace_slots(ctx.handle, small, capi.C.c_size_t(8), None) == -1
    for bad in (-1, 256):
        assert ctx.lib.vslam_ctx_workspace_fill(ctx.handle, capi.C.c_int(bad)) == -1
    assert ctx.lib.vslam_ctx_workspace_fill(None, capi.C.c_int(0)) == -1
    ctx.workspace_fill(0)
    ctx.synchronize()
    assert ctx.workspace_slots() == slots, "a fill allocates nothing"


@pytest.mark.parametrize("name", HELD + FORM_NAMES)
def test_zeroed_workspace(ctx, table, name):
    hold_zeroed(ctx, name, table.held[name])


@pytest.mark.parametrize("name", HELD + FORM_NAMES)
def test_stale_workspace(ctx, table, name):
    hold_stale(ctx, name, table.held[name])


# ------------------------------------------------------------------------------------- batch sizes where the launch shape changes
BW, BH = 64, 136          # one column strip per frame
SEAMS = (46, 68, 92)      # rows where a segment of 46 (3 per frame) or 68 (2 per frame) rows ends
BATCHES = (9, 80, 2047, 2048)
BMAXC = 32


def stream_segments(h, frames, strips):
    """vs_stream_segments (vslam_amd/csrc/ctx.h)"""
    segs = (h + 45) // 90 if h >= 135 else 1
    if frames * strips * segs < 4096:
        segs = max(1, min(-(-4096 // (frames * strips)), max(h // 24, 1)))
    return segs


def pool_slots(frames):
    """pool.slots of vs_launch_good_features (vslam_amd/csrc/select.hip), two-tier rows"""
    return frames if frames < 4 else min(max(frames // 16, 4), 64)


def test_the_batches_sit_on_the_seams_of_the_launch_formulas():
    """The numbers the batch tests are built on, computed from copies of the two formulas, and the formulas themselves still as copied:
    a change of either fails here instead of silently moving the tests off the seam."""
    assert [stream_segments(BH, f, 1) for f in BATCHES] == [5, 5, 3, 2]
    assert -(-BH // 3) == SEAMS[0] and BH // 2 == SEAMS[1] and 2 * SEAMS[0] == SEAMS[2]
    assert [pool_slots(f) for f in (3, 4, 80, 2048)] == [3, 4, 5, 64]
    assert -(-9 // 8) * 8 == 16                                   # vs_xcd_grid pads 9 items to 16
    src = lambda f: re.sub(r"\s+", " ", open(os.path.join(ROOT, "vslam_amd", "csrc", f)).read())
    ctx_h, select = src("ctx.h"), src("select.hip")
    for text in ("int segs = h >= 135 ? (h + 45) / 90 : 1;", "if (waves < 4096) {", "const int most = h / 24 > 1 ? h / 24 : 1;",
                 "const long long want = (4096 + (long long)frames * strips - 1) / ((long long)frames * strips);",
                 "static inline int vs_xcd_grid(int items, int per_item) { return vs_div_up(items, 8) * 8 * per_item; }"):
        assert text in ctx_h, text
    assert "pool.slots = two_tier ? (frames < 4 ? frames : (frames / 16 < 4 ? 4 : (frames / 16 > 64 ? 64 : frames / 16))) : 0;" in select


def _seam_frames():
    """8 distinct frames of 64 x 136: bright blocks on weak noise whose corners lie on rows 44..48, 66..70 and 90..94"""
    rng = np.random.default_rng(2026)
    frames = (96 + rng.integers(0, 9, (8, BH, BW))).astype(np.uint8)
    for k in range(8):
        for j, seam in enumerate(SEAMS):
            top = seam - 2 + (k + j) % 5                           # 44 .. 48 around the first seam, and so on
            x0 = 21 + 10 * ((k + j) % 2) + ((k >> 1) + j) % 2        # a corner in column 31 or 32: what a 31-pixel border leaves of 64
            frames[k, top:top + 9, x0:x0 + 11] = 200 + 5 * ((k + j) % 4)
            frames[k, top - 12:top - 1, (5 * k + 17 * j) % 50:(5 * k + 17 * j) % 50 + 8] = 30 + 7 * k
    return frames


@pytest.fixture(scope="module")
def seam_refs(oracle):
    frames = _seam_frames()
    bgr = np.ascontiguousarray(np.repeat(frames[..., None], 3, 3))
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    ex = [oracle.extract_features(bgr[k], BMAXC, ca, sa, pat) for k in range(8)]
    gf = [oracle.good_features(frames[k], BMAXC) for k in range(8)]
    assert all(oracle.bgr2gray(bgr[k]).tobytes() == frames[k].tobytes() for k in range(8))
    for k in range(8):     # corners on the seams' rows, in every frame
        rows = gf[k][:, 1]
        assert all(((rows >= s - 2) & (rows <= s + 2)).any() for s in SEAMS), (k, sorted(rows.tolist()))

    def padded(rows, shape, dtype):
        out = np.zeros((8,) + shape, dtype)
        for k, r in enumerate(rows):
            out[k, :len(r)] = r
        return _t(out)
    return dict(frames=frames, bgr=bgr, pat=pat, ca=ca, sa=sa,
                eig=_t(np.stack([oracle.min_eigen(frames[k]) for k in range(8)])), blur=_t(np.stack([oracle.gaussian7(frames[k]) for k in range(8)])),
                gf_n=_t(np.array([len(g) for g in gf], np.int32)), gf_xy=padded(gf, (BMAXC, 2), np.float32),
                ex_n=_t(np.array([e["n"] for e in ex], np.int32)), ex_nd=_t(np.array([e["n_detected"] for e in ex], np.int32)),
                ex_xy=padded([e["xy"] for e in ex], (BMAXC, 2), np.float32), ex_desc=padded([e["desc"] for e in ex], (BMAXC, 32), np.uint8),
                ex_nodes=padded([e["nodes"] for e in ex], (BMAXC,), np.int32))


def _rows_equal(got, n, want, idx):
    """rows [0, n[f]) of got[f] equal those of want[idx[f]] (rows past the count keep the caller's bits: not the stage's business)"""
    used = (torch.arange(got.shape[1], device=got.device)[None, :] < n[:, None]).reshape(got.shape[:2] + (1,) * (got.dim() - 2))
    return bool(((got == want[idx]) | ~used).all())


@pytest.mark.parametrize("frames", BATCHES)
def test_every_copy_equals_the_oracle_at_every_batch_size(ctx, seam_refs, frames):
    """min_eigen, gaussian7, good_features and extract_features on the 8 frames tiled to 9 (an item grid padded to 16), 80, 2047 (3 row
    segments of 46 rows) and 2048 frames (2 of 68): every copy of a frame gives the oracle's result for that frame, bit for bit, and so
    the batch sizes agree with each other."""
    r = seam_refs
    idx = torch.arange(frames, device="cuda") % 8
    gray = _t(r["frames"])[idx].contiguous()
    assert torch.equal(ctx.min_eigen(gray).view(i32), r["eig"].view(i32)[idx]), "min_eigen"
    assert torch.equal(ctx.gaussian7(gray), r["blur"][idx]), "gaussian7"
    xy, n = ctx.good_features(gray, BMAXC)
    assert torch.equal(n, r["gf_n"][idx]) and _rows_equal(xy.view(i32), n, r["gf_xy"].view(i32), idx), "good_features"
    out = ctx.extract_features(_t(r["bgr"])[idx].contiguous(), BMAXC, r["ca"], r["sa"], _t(r["pat"]))
    ctx.synchronize()
    assert torch.equal(out["n"], r["ex_n"][idx]) and torch.equal(out["n_detected"], r["ex_nd"][idx]), "extract_features: counts"
    assert int(r["ex_n"].min()) > 0
    for k, want in (("xy", r["ex_xy"].view(i32)), ("desc", r["ex_desc"]), ("nodes", r["ex_nodes"])):
        got = out[k].view(i32) if k == "xy" else out[k]
        assert _rows_equal(got, out["n"], want, idx), "extract_features: " + k


@pytest.mark.parametrize("frames,flat", [(80, 40), (2048, 200)])
def test_flat_frames_take_no_slot_of_the_corner_pool(ctx, oracle, frames, flat):
    """At the default list bound (16 x 32 + 4096 of 8704 pixels) a constant frame lists every interior pixel and overflows its list; the
    selection sees that it is constant and gives it no corners without a pool slot.  Many more flat frames than the pool has slots (40
    for 5, 200 for 64) among textured ones, and one frame that is constant but for ONE pixel, which is no flat frame: it goes through the
    pool and equals the oracle like every textured frame.  No CAPACITY is reported."""
    tex = _gray(91, 8, BW, BH)
    almost = np.full((BH, BW), 90, np.uint8)
    almost[BH - 1, BW - 1] = 91                                     # the last byte a scan reaches
    refs = [oracle.good_features(tex[k], BMAXC) for k in range(8)] + [oracle.good_features(almost, BMAXC)]
    where = [(i * frames) // flat + 1 for i in range(flat)]
    gray = tex[np.arange(frames) % 8]
    gray[where] = 90
    gray[where[1]] = almost
    xy, n = ctx.good_features(_t(gray), BMAXC)
    status = ctx.lib.vslam_ctx_synchronize(ctx.handle)
    st = ctx.corner_stats()
    print(f"{frames} frames, {flat} flat: vslam_ctx_synchronize {status}, {st}")
    assert status == 0 and st["pool_sets"] == pool_slots(frames) and st["frames_overflowed"] == 1, (status, st)
    xy, n = xy.cpu().numpy(), n.cpu().numpy()
    for f in range(frames):
        ref = refs[8] if f == where[1] else (np.zeros((0, 2), np.float32) if f in where else refs[f % 8])
        assert n[f] == len(ref) and np.array_equal(xy[f, :n[f]].view(np.uint32), ref.view(np.uint32)), f


def test_flat_frames_through_the_fused_front_end(ctx, oracle):
    """vslam_extract_features forms the gray image inside the detector: 6 constant frames of 8 (the pool has 4 slots) have no keypoints
    and take no slot; the two textured frames equal the oracle."""
    bgr = synth.frames_numpy(91, 4, 160, 120)
    flat = [0, 1, 3, 4, 6, 7]
    bgr[flat] = 90
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    out = ctx.extract_features(_t(bgr), 60, ca, sa, _t(pat), kp_stride=64)
    status = ctx.lib.vslam_ctx_synchronize(ctx.handle)
    st = ctx.corner_stats()
    print(status, st)
    assert status == 0 and st["frames_overflowed"] == 0, (status, st)
    n = out["n"].cpu().numpy()
    assert not n[flat].any() and not out["n_detected"].cpu().numpy()[flat].any()
    for f in (2, 5):
        ref = oracle.extract_features(bgr[f], 60, ca, sa, pat)
        assert n[f] == ref["n"] > 0 and np.array_equal(out["xy"][f, :n[f]].cpu().numpy(), ref["xy"])
        assert np.array_equal(out["desc"][f, :n[f]].cpu().numpy(), ref["desc"])


@pytest.mark.parametrize("frames,textured", [(80, 5), (2048, 60)])
def test_the_corner_pool_at_5_and_64_slots(ctx, oracle, frames, textured):
    """VSLAM_OPT_CORNER_LIST_CAP = 40: every textured frame overflows its list and is redone from a pool slot (5 slots for 80 frames, 64
    for 2048); the other frames are flat.  Every textured frame equals the oracle and no CAPACITY is reported.

    This is the test that found the one bug of this file: a flat frame lists every interior pixel (tier 1's bound carries an absolute
    margin, and nothing on a constant image raises the threshold from -inf), so it overflowed any bounded list and took a pool ticket
    like a textured frame -- 80 tickets for 5 slots, 2048 for 64, VSLAM_ERR_CAPACITY, and the frames that lost the race got no corners.
    The selection now tells a constant frame by its gray bytes before it files it (select.hip; HISTORY.md)."""
    assert pool_slots(frames) in (5, 64) and textured <= pool_slots(frames)
    tex = _gray(91, 8, BW, BH)
    refs = [oracle.good_features(tex[k], BMAXC) for k in range(8)]
    assert all(len(r) > 8 for r in refs)
    where = [(i * frames) // textured + 3 for i in range(textured)]
    gray = np.full((frames, BH, BW), 90, np.uint8)
    for i, f in enumerate(where):
        gray[f] = tex[i % 8]
    try:
        ctx.set_option(OPT.OPT_CORNER_LIST_CAP, 40)
        xy, n = ctx.good_features(_t(gray), BMAXC)
        status = ctx.lib.vslam_ctx_synchronize(ctx.handle)           # reads and clears the error word
        st = ctx.corner_stats()
    finally:
        ctx.set_option(OPT.OPT_CORNER_LIST_CAP, 0)
    print(f"{frames} frames, {textured} textured: vslam_ctx_synchronize {status}, {st}")
    assert status == 0, (capi.ERRORS.get(status, status), st)
    assert st["pool_sets"] == pool_slots(frames) and st["frames_overflowed"] == textured, st
    xy, n = xy.cpu().numpy(), n.cpu().numpy()
    flat = np.ones(frames, bool)
    flat[where] = False
    assert not n[flat].any(), "a flat frame has no corners"
    for i, f in enumerate(where):
        ref = refs[i % 8]
        assert n[f] == len(ref) and np.array_equal(xy[f, :n[f]].view(np.uint32), ref.view(np.uint32)), (f, i % 8)
