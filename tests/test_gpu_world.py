"""The world frame on the device (vslam_world_* / vslam_map_attach_world) against tests/ref_world.py, BIT FOR BIT: Twc, scale,
links, the f32 poses, the carry, lifted points and the rows a lift must leave alone.  The f64 square root is the one operation
the project had not relied on bit-exactly before; test_device_sqrt_is_correctly_rounded holds it to the host's on 4096 values,
so nothing here has a tolerance."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import ref_world as rw
import world_cases as wc
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = capi.C
K = wc.K
CASES = wc.cases()
NAMES = sorted(CASES)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _step_batch(steps, kp):
    """one step of T scripts -> cuda tensors [T][...]"""
    T = len(steps)
    b = dict(matches=np.full((T, kp, 2), 3, np.int32), best=np.zeros((T, 4), np.int32), X=np.full((T, kp, 4), 0.5, np.float32),
             R=np.zeros((T, 9), np.float32), t=np.zeros((T, 3), np.float32), n_last=np.zeros(T, np.int32), n_cur=np.zeros(T, np.int32))
    for i, st in enumerate(steps):
        n = len(st["matches"])
        b["matches"][i, :n], b["X"][i, :n] = st["matches"], st["X"]
        b["best"][i] = (0 if st["winner"] else -1, n, 0, n)
        b["R"][i], b["t"][i], b["n_last"][i], b["n_cur"][i] = st["R"], st["t"], st["n_last"], st["n_cur"]
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}


def _poke(ctx, world, track, carry, valid):
    a = world.arrays()
    kp = world.kp_stride
    c = np.ascontiguousarray(carry, np.float64)
    idx = np.where(valid, 0, -1).astype(np.int32)
    ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, C.c_void_p(a.d_carry + 24 * track * kp), C.c_void_p(c.ctypes.data), C.c_size_t(c.nbytes)))
    ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, C.c_void_p(a.d_carry_index + 4 * track * kp), C.c_void_p(idx.ctypes.data),
                                      C.c_size_t(idx.nbytes)))


def _run_scripts(ctx, scripts, kp=K, min_links=8, frames=5):
    """the scripts as one batch through vslam_world_step / _lift -> (view, [lifted (T, kp, 4) per step])"""
    T = len(scripts)
    world = capi.World(ctx, T, frames, kp, min_links)
    lifted = []
    try:
        for f in range(1, len(scripts[0]) + 1):
            steps = [s[f - 1] for s in scripts]
            for i, st in enumerate(steps):
                if st["poke"] is not None:
                    _poke(ctx, world, i, *st["poke"])
            b = _step_batch(steps, kp)
            world.step(b["matches"], b["best"], b["X"], b["R"], b["t"], b["n_last"], b["n_cur"])
            lo = torch.tensor([1 if len(st["matches"]) > 2 else 0 for st in steps], dtype=torch.int32).cuda()
            hi = torch.tensor([len(st["matches"]) for st in steps], dtype=torch.int32).cuda()
            out = torch.full((T, kp, 4), 7.0, dtype=torch.float32).cuda()
            lifted.append((world.lift(f, b["X"], lo, hi, out).cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()))
        ctx.synchronize()
        return world.view(), lifted
    finally:
        world.close()


def _hold_to_reference(view, lifted, scripts, slot_of=None, min_links=8, kp=K):
    for i, script in enumerate(scripts):
        ref = rw.World(kp, min_links)
        for f, st in enumerate(script, 1):
            if st["poke"] is not None:
                ref.carry, ref.valid = st["poke"][0].copy(), st["poke"][1].copy()
            ref.step(st["matches"], st["X"], st["R"], st["t"], st["n_last"], st["n_cur"], winner=st["winner"])
            tag = (i, f)
            assert np.array_equal(_u64(view["Twc"][i, f]), _u64(ref.Twc[f])), tag
            assert np.array_equal(_u32(view["pose"][i, f]), _u32(ref.Twc[f].astype(np.float32))), tag
            assert _u64(view["scale"][i, f]) == _u64(ref.scale[f]), tag
            assert view["links"][i, f] == ref.links[f], tag
            got, lo, hi = lifted[f - 1]
            want = np.full((kp, 4), 7.0, np.float32)
            X = np.full((kp, 4), 0.5, np.float32)
            X[:len(st["X"])] = st["X"]
            ref.lift(f, X, int(lo[i]), int(hi[i]), want)
            assert np.array_equal(_u32(got[i]), _u32(want)), tag      # lifted rows and the untouched ones
        assert np.array_equal(view["carry_index"][i] >= 0, ref.valid), i
        assert np.array_equal(_u64(view["carry"][i][ref.valid]), _u64(ref.carry[ref.valid])), i
    assert view["frames"] == len(scripts[0]) + 1


@pytest.mark.parametrize("group", range(4))
def test_hand_worked_cases_bit_exact(ctx, group):
    names = [NAMES[(3 * group + j) % len(NAMES)] for j in range(3)]
    scripts = [CASES[n]["steps"] for n in names]
    view, lifted = _run_scripts(ctx, scripts)
    for i, n in enumerate(names):      # the hand-worked numbers, on the device's own output
        assert view["scale"][i, 1] == CASES[n]["expect"]["scale"] and view["links"][i, 1] == CASES[n]["expect"]["links"], n
        assert view["links"][i, 3] == -1, n
    _hold_to_reference(view, lifted, scripts)


def _selection_one_track_linked_neighbours_empty(ctx, kp):
    rng = np.random.default_rng(5)
    m = np.stack([rng.permutation(kp), rng.permutation(kp)], 1)
    X = np.stack([rng.uniform(-2, 2, kp), rng.uniform(-2, 2, kp), rng.uniform(1, 9, kp)], 1)
    carry = X * rng.uniform(0.5, 2.0, (kp, 1)) * 1.7
    full = wc.step(m, X, wc.RZ90, [0.6, 0, 0.8], n_last=kp, n_cur=kp, poke=(carry, np.ones(kp, bool)))
    none = wc.step(m, X, wc.RZ90, [0.6, 0, 0.8], n_last=kp, n_cur=kp, poke=(np.zeros((kp, 3)), np.zeros(kp, bool)))
    follow = wc.step(m[:, ::-1], X[::-1], wc.I9, [0, 1, 0], n_last=kp, n_cur=kp)
    scripts = [[none, follow], [full, follow], [none, follow]]
    view, lifted = _run_scripts(ctx, scripts, kp=kp, frames=3)
    assert view["links"][:, 1].tolist() == [0, kp, 0] and view["links"][:, 2].tolist() == [kp, kp, kp]
    _hold_to_reference(view, lifted, scripts, kp=kp)


def test_selection_at_8160_one_track_linked_neighbours_empty(ctx):
    _selection_one_track_linked_neighbours_empty(ctx, 8160)


def test_selection_at_max_kp_one_track_linked_neighbours_empty(ctx):
    """kp_stride = VSLAM_MAX_KP = 16384 (include/vslam_amd.h), the most the ABI takes: 128 KB of keys in the step kernel's LDS
    beside its 1040 static bytes, every match slot used (full permutations), links == kp."""
    _selection_one_track_linked_neighbours_empty(ctx, 16384)


def test_device_sqrt_is_correctly_rounded(ctx):
    """4096 tracks, one link each (min_links = 1): s = sqrt(q), q = c^2 / 1, against numpy's correctly rounded square root."""
    T, kp = 4096, 8
    rng = np.random.default_rng(9)
    c = np.concatenate([rng.uniform(0.5, 2.0, T - 64), 2.0 ** rng.uniform(-400, 400, 64)])
    world = capi.World(ctx, T, 2, kp, 1)
    try:
        carry = np.zeros((T, kp, 3)); carry[:, 0, 2] = c
        idx = np.full((T, kp), -1, np.int32); idx[:, 0] = 0
        a = world.arrays()
        ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, C.c_void_p(a.d_carry), C.c_void_p(carry.ctypes.data), C.c_size_t(carry.nbytes)))
        ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, C.c_void_p(a.d_carry_index), C.c_void_p(idx.ctypes.data), C.c_size_t(idx.nbytes)))
        st = wc.step([[0, 1]], [[0, 0, 1]], n_last=kp, n_cur=kp)
        b = _step_batch([st] * T, kp)
        world.step(b["matches"], b["best"], b["X"], b["R"], b["t"], b["n_last"], b["n_cur"])
        ctx.synchronize()
        v = world.view()
    finally:
        world.close()
    q = (c * c) / 1.0
    assert (v["links"][:, 1] == 1).all()
    bad = np.flatnonzero(_u64(v["scale"][:, 1]) != _u64(np.sqrt(q)))
    print(f"sqrt: {len(bad)} of {T} differ from the correctly rounded value")
    assert len(bad) == 0


def test_one_track_same_bits_in_any_slot_batch_and_run(ctx):
    script = CASES["ties"]["steps"]
    other = CASES["odd_L9"]["steps"]
    runs = []
    for scripts, slot in (([script], 0), ([other, other, script], 2), ([other] * 5 + [script] + [other], 5), ([script], 0)):
        view, lifted = _run_scripts(ctx, scripts)
        runs.append({k: np.asarray(view[k])[slot] for k in ("Twc", "pose", "scale", "links", "carry", "carry_index")}
                    | {f"lift{f}": lifted[f][0][slot] for f in range(4)})
    for r in runs[1:]:
        for k in runs[0]:
            assert np.array_equal(np.asarray(runs[0][k]).view(np.uint8), np.asarray(r[k]).view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ errors
def test_errors_shape_mismatch_null_pointer_and_step_beyond_max_frames(ctx):
    pmap = capi.PointMap(ctx, 3, 5, K, 64, 256)
    bad = [capi.World(ctx, 3, 5, K + 1), capi.World(ctx, 2, 5, K), capi.World(ctx, 3, 4, K)]
    world = capi.World(ctx, 3, 2, K)
    try:
        for w in bad:
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                pmap.attach_world(w)
        assert pmap.world is None
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            capi.World(ctx, 3, 5, K, min_links=0)
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            capi.World(ctx, 1, 2, 16385)
        b = _step_batch([CASES["ties"]["steps"][1]] * 3, K)
        args = [b["matches"], b["best"], b["X"], b["R"], b["t"], b["n_last"], b["n_cur"]]
        for i in range(len(args)):
            with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
                world.step(*[None if j == i else x for j, x in enumerate(args)])
        lo = torch.zeros(3, dtype=torch.int32).cuda()
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            world.lift(1, b["X"], lo, lo)                    # no pair recorded yet
        assert ctx.lib.vslam_world_view(world.handle, C.c_void_p(0)) == -1
        assert ctx.lib.vslam_map_attach_world(C.c_void_p(0), world.handle) == -1
        world.step(*args)
        ctx.synchronize()
        before = world.view()
        world.step(*args)                                    # max_frames = 2: no slot
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_CAPACITY"):
            ctx.synchronize()
        after = world.view()
        for k in before:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), k
        with pytest.raises(capi.VslamError, match="VSLAM_ERR_INVALID"):
            world.lift(2, b["X"], lo, lo)
        ctx.synchronize()
    finally:
        pmap.close()
        for w in bad + [world]:
            w.close()


# ------------------------------------------------------------------------------------------------ attached to a map
MAXC, KP, HYP, THR = 400, 448, 256, 10.0          # the smallest shape of tests/test_gpu_map.py
TRACKS, FRAMES, W, H = 3, 6, 320, 240
MCAP, OCAP = FRAMES * MAXC, 4 * FRAMES * MAXC


def _Kmat():
    return np.array([[525, 0, W // 2], [0, 525, H // 2], [0, 0, 1]], np.float32)


def _track(ctx, pmap, d_bgr):
    pat = torch.from_numpy(synth.brief_pattern()).cuda()
    ca, sa = synth.keypoint_rotation()
    seeds = (np.arange(TRACKS * (FRAMES - 1), dtype=np.uint32).reshape(TRACKS, FRAMES - 1) * 7919 + 200006).astype(np.uint32)
    d_seeds = torch.from_numpy(seeds.view(np.int32).copy()).cuda()
    return ctx.track_sequences(pmap, d_bgr, MAXC, ca, sa, pat, d_seeds, HYP, THR, _Kmat())


def _frame_batches(out, f):
    def per_frame(a):
        return a.view(TRACKS, FRAMES, *a.shape[1:])[:, f].contiguous()

    def per_pair(a):
        full = torch.cat([a, torch.zeros_like(a[:1])])
        return full.view(TRACKS, FRAMES, *a.shape[1:])[:, f - 1].contiguous()
    frame = {k: per_frame(out[k]) for k in ("xy", "desc", "nodes", "n")}
    pair = {k: per_pair(out[k]) for k in ("matches", "best", "F")} if f > 0 else None
    return frame, pair


def _same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(np.atleast_1d(a[k]).view(np.uint8), np.atleast_1d(b[k]).view(np.uint8)), k


@pytest.fixture(scope="module")
def sequences():
    return torch.from_numpy(synth.sequences_numpy(2, TRACKS, FRAMES, W, H)).cuda()


@pytest.mark.parametrize("refit,refine", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["plain", "pose_refit", "pose_refine", "pose_refit_refine"])
def test_attached_world_equals_separate_step_and_lift(ctx, sequences, refit, refine):
    a = capi.PointMap(ctx, TRACKS, FRAMES, KP, MCAP, OCAP)
    b = capi.PointMap(ctx, TRACKS, FRAMES, KP, MCAP, OCAP)
    c = capi.PointMap(ctx, TRACKS, FRAMES, KP, MCAP, OCAP)
    wa, wc_ = a.attach_world(), c.attach_world()
    wd = capi.World(ctx, TRACKS, FRAMES, KP)
    try:
        front = _track(ctx, b, sequences)                         # the front end's outputs with both options off
        ctx.synchronize()
        ctx.set_option(ctx.OPT_POSE_REFIT, refit)
        ctx.set_option(ctx.OPT_POSE_REFINE, refine)
        out = _track(ctx, a, sequences)
        ctx.synchronize()
        sa = a.view()
        print(f"sizes {sa['sizes'].tolist()}, links {sa['world_links'].tolist()}, scale {np.round(sa['world_scale'], 4).tolist()}")
        assert sa["world_frames"] == FRAMES and int(sa["sizes"].min()) > 8 and int(sa["world_links"][:, 2:].max()) >= 8, \
            "the scenes have to triangulate and link"
        _track(ctx, b, sequences)
        ctx.synchronize()
        sb = b.view()
        _same(sa, sb, keys=list(sb))                              # the map's own arrays: the same with and without a world
        # by hand: c with its world attached; b followed by a separate world step + lift on the same inputs
        b.reset()
        Km = _Kmat()
        acc = torch.zeros((TRACKS, MCAP, 4), dtype=torch.float32).cuda()
        # VSLAM_OPT_POSE_REFIT is a property of vslam_track_sequences, not of vslam_map_step: by hand, the front end's F is
        # refitted before the steps
        own = [t_ * FRAMES + f for t_ in range(TRACKS) for f in range(FRAMES - 1)]
        for k in ("xy", "desc", "nodes", "n"):
            assert torch.equal(out[k], front[k]), k
        for k in ("matches", "best"):
            assert torch.equal(out[k][own], front[k][own]), k
        assert torch.equal(out["F"][own], front["F"][own]) == (not refit), "the refit moves F, and nothing else does"
        last, _ = _frame_batches(front, 0)
        for f in range(1, FRAMES):
            cur, pair = _frame_batches(front, f)
            if refit:
                pair["F"], _ = ctx.refit_fundamental(last["xy"], cur["xy"], pair["matches"], pair["best"], pair["F"], want_stats=False)
                assert torch.equal(pair["F"].view(torch.int32), _frame_batches(out, f)[1]["F"].view(torch.int32)), f
            img = sequences[:, f].contiguous()
            c.step(last, cur, pair, img, Km)
            lo = torch.from_numpy(b.view()["sizes"]).cuda()
            b.step(last, cur, pair, img, Km)
            R, t, c2 = ctx.extract_Rt(pair["F"], pair["best"], Km)
            pts = ctx.triangulate(last["xy"], cur["xy"], pair["matches"], pair["best"], Km, c2)
            if refine:
                ctx.refine_pairs(last["xy"], cur["xy"], pair["matches"], pair["best"], Km, R, t, pts, gate_sq=16.0, max_iterations=20,
                                 want_stats=False)
            wd.step(pair["matches"], pair["best"], pts, R, t, last["n"], cur["n"])
            vb = b.view()
            wd.lift(f, torch.from_numpy(vb["points"]).cuda(), lo, torch.from_numpy(vb["sizes"]).cuda(), acc)
            last = cur
        ctx.synchronize()
        _same(sa, c.view())                                       # vslam_track_sequences = stepping by hand, world included
        vd = wd.view()
        for k in ("Twc", "pose", "scale", "links", "carry", "carry_index", "frames"):
            assert np.array_equal(np.atleast_1d(vd[k]).view(np.uint8), np.atleast_1d(sa["world_" + k]).view(np.uint8)), k
        assert np.array_equal(_u32(acc.cpu().numpy()), _u32(sa["world_points"]))
        for t_ in range(TRACKS):                                  # lifted where the map has points, zero elsewhere
            assert not sa["world_points"][t_, sa["sizes"][t_]:].any() and (sa["world_points"][t_, :sa["sizes"][t_], 3] == 1).all()
        if refine:                                                # the world saw the adjusted values
            ctx.set_option(ctx.OPT_POSE_REFINE, 0)
            _track(ctx, a, sequences)
            ctx.synchronize()
            assert not np.array_equal(a.view()["world_Twc"], sa["world_Twc"])
        if refit:                                                 # and the refitted F
            ctx.set_option(ctx.OPT_POSE_REFIT, 0)
            ctx.set_option(ctx.OPT_POSE_REFINE, 0)
            _track(ctx, a, sequences)
            ctx.synchronize()
            assert not np.array_equal(a.view()["world_Twc"], sa["world_Twc"])
            ctx.set_option(ctx.OPT_POSE_REFINE, refine)           # the render below runs as the steps above did
        # vslam_world_render = vslam_render_points over the world's arrays
        view = capi.View.look_at((-3, -2, -6), (0, 0, 4), (0, 1, 0), 160, 120, lib=ctx.lib, point_size=2)
        wa_arr = wc_.view()
        cv = c.view()
        got = wc_.render(c, view, 160, 120, depth=True)
        want = ctx.render_points(torch.from_numpy(wa_arr["points"]).cuda(), torch.from_numpy(cv["colors"]).cuda(),
                                 torch.from_numpy(cv["sizes"]).cuda(), view, 160, 120, pose=torch.from_numpy(wa_arr["pose"]).cuda(),
                                 frames=FRAMES, depth=True)
        ctx.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
        assert int((got[0] != 0).sum()) > 0, "something is drawn"
        one = wc_.render(c, view, 160, 120, tracks=(1, 1))
        assert torch.equal(one[0], got[0][1])
        # vslam_map_reset resets both
        c.reset()
        ctx.synchronize()
        e = c.view()
        assert e["frames"] == 1 and e["world_frames"] == 1 and not e["world_points"].any() and not e["sizes"].any()
        assert (e["world_carry_index"] == -1).all() and (e["world_scale"] == 1).all() and (e["world_links"] == 0).all()
        assert np.array_equal(e["world_Twc"], np.tile(np.eye(4).reshape(16), (TRACKS, FRAMES, 1)))
    finally:
        ctx.set_option(ctx.OPT_POSE_REFIT, 0)
        ctx.set_option(ctx.OPT_POSE_REFINE, 0)
        a.close(); b.close(); c.close()
        wa.close(); wc_.close(); wd.close()


# ------------------------------------------------------------------------------------------------ C++ surface
@pytest.fixture(scope="module")
def world_demo(tmp_path_factory):
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("world_demo") / "world_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "world_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    return exe


def test_cpp_world_matches_the_c_entry_points(ctx, world_demo, tmp_path):
    """tests/native/world_demo.cpp, mode 0: vslam::World (include/vslam/World.h) stepped by hand on a script of
    tests/world_cases.py gives the bits of vslam_world_step / _lift."""
    script = [dict(st, poke=None) for st in CASES["odd_L9"]["steps"][1:]]      # the carry builds up through the steps
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", 0, K, len(script)))
        for st in script:
            n = len(st["matches"])
            f.write(struct.pack("4i", 1 if st["winner"] else 0, n, st["n_last"], st["n_cur"]))
            f.write(st["R"].tobytes()); f.write(st["t"].tobytes())
            f.write(np.ascontiguousarray(st["matches"], np.int32).tobytes()); f.write(np.ascontiguousarray(st["X"], np.float32).tobytes())
    subprocess.run([world_demo, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    frames = len(script) + 1
    view, lifted = _run_scripts(ctx, [script], frames=frames)
    off = 0
    Twc = np.frombuffer(buf, np.float64, frames * 16, off).reshape(frames, 16); off += frames * 128
    pose = np.frombuffer(buf, np.float32, frames * 16, off).reshape(frames, 16); off += frames * 64
    scale = np.frombuffer(buf, np.float64, frames, off); off += frames * 8
    links = np.frombuffer(buf, np.int32, frames, off); off += frames * 4
    assert np.array_equal(_u64(Twc), _u64(view["Twc"][0])) and np.array_equal(_u32(pose), _u32(view["pose"][0]))
    assert np.array_equal(_u64(scale), _u64(view["scale"][0])) and np.array_equal(links, view["links"][0])
    assert links.tolist() == [0, 0, -1, 0] and not np.array_equal(Twc[1], Twc[0])
    for f in range(len(script)):
        got = np.frombuffer(buf, np.float32, K * 4, off).reshape(K, 4); off += K * 16
        want, lo, hi = lifted[f]
        assert np.array_equal(_u32(got[int(lo[0]):int(hi[0])]), _u32(want[0][int(lo[0]):int(hi[0])])), f
        assert not got[int(hi[0]):].any(), f
    assert off == len(buf)


def test_cpp_pointmap_world_points_and_poses_match_the_c_entry_points(ctx, world_demo, tmp_path):
    """mode 1: the reference's loop over include/vslam/PointMap.h with vslam::map_attach_world; world_points() / world_poses()
    after sync_to_host() are the bits vslam_track_sequences leaves in an attached world for the same frames."""
    w, h, maxc, hyp, frames = 320, 240, 400, 256, 5
    bgr = synth.sequences_numpy(2, 1, frames, w, h)
    seeds = (np.arange(frames - 1, dtype=np.uint32) * 7919 + 5).astype(np.uint32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("6i", 1, w, h, maxc, hyp, frames))
        f.write(seeds.tobytes())
        f.write(bgr[0].tobytes())
    subprocess.run([world_demo, fin, fout], check=True, timeout=120)
    buf = open(fout, "rb").read()
    size = struct.unpack_from("i", buf, 0)[0]
    pts = np.frombuffer(buf, np.float32, size * 4, 4).reshape(size, 4)
    wpts = np.frombuffer(buf, np.float32, size * 4, 4 + 16 * size).reshape(size, 4)
    n_poses = struct.unpack_from("i", buf, 4 + 32 * size)[0]
    poses = np.frombuffer(buf, np.float32, n_poses * 16, 8 + 32 * size).reshape(n_poses, 16)
    pmap = capi.PointMap(ctx, 1, frames, maxc, frames * maxc, 4 * frames * maxc)
    world = pmap.attach_world()
    try:
        pat = torch.from_numpy(synth.brief_pattern()).cuda()
        ca, sa = synth.keypoint_rotation()
        Km = np.array([[525, 0, w // 2], [0, 525, h // 2], [0, 0, 1]], np.float32)
        ctx.track_sequences(pmap, torch.from_numpy(bgr).cuda(), maxc, ca, sa, pat,
                            torch.from_numpy(seeds.view(np.int32).reshape(1, -1).copy()).cuda(), hyp, 10.0, Km)
        ctx.synchronize()
        v = pmap.view()
    finally:
        pmap.close()
        world.close()
    assert size == v["sizes"][0] > 8 and n_poses == frames
    assert np.array_equal(_u32(pts), _u32(v["points"][0, :size]))
    assert np.array_equal(_u32(wpts), _u32(v["world_points"][0, :size])) and not np.array_equal(wpts, pts)
    assert np.array_equal(_u32(poses), _u32(v["world_pose"][0]))
