"""The device renderer (vslam_render_points / vslam_map_render, include/vslam_amd.h "the view of the map") against
tests/ref_render.py: BIT-EXACT -- the BGR bytes, and the depth plane as u32 bit patterns; no tolerance and no excluded pixel.
tests/test_ref_render.py holds the reference itself to definitions and asserts that the random scenes are not trivial."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import ref_render
import render_scenes
from vslam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD_BYTE = 0xA5

# the constants of tests/test_gpu_map.py, restated
MAXC, KP, HYP, THR = 400, 448, 256, 10.0
TRACKS, FRAMES = 3, 6
SHAPES = [(2, 320, 240, 0), (3, 322, 200, 10)]


def c_view(v):
    """ref_render.View -> capi.View (the struct handed to the library)."""
    out = capi.View()
    for i in range(16):
        out.mv[i] = float(v.mv[i])
    out.fu, out.fv, out.u0, out.v0 = float(v.fu), float(v.fv), float(v.u0), float(v.v0)
    out.z_near, out.z_far, out.point_size, out.flags = float(v.z_near), float(v.z_far), v.point_size, v.flags
    out.box_w, out.box_h_ratio, out.box_z_ratio = (float(b) for b in v.box)
    for i in range(3):
        out.background_bgr[i] = v.background[i]
        out.frustum_bgr[i] = v.frustum[i]
    return out


def ref_view(v):
    """capi.View -> ref_render.View."""
    return ref_render.View(np.array(list(v.mv), np.float32), v.fu, v.fv, v.u0, v.v0, v.z_near, v.z_far, v.point_size, v.flags,
                           (v.box_w, v.box_h_ratio, v.box_z_ratio), tuple(v.background_bgr), tuple(v.frustum_bgr))


def _outputs(T, W, H, pad):
    bgr = torch.full((T, H, 3 * W + pad), PAD_BYTE, dtype=torch.uint8, device="cuda")
    depth = torch.full((T, H, W), -7.0, dtype=torch.float32, device="cuda")
    return bgr, depth


def _check(bgr, depth, ref_bgr, ref_depth, W, tag):
    bgr, depth = bgr.cpu().numpy(), depth.cpu().numpy()
    T, H = bgr.shape[:2]
    assert (bgr[..., 3 * W:] == PAD_BYTE).all(), f"{tag}: row padding was written"
    got = bgr[..., :3 * W].reshape(T, H, W, 3)
    for t in range(T):
        print(f"{tag} track {t}: {int(np.isfinite(ref_depth[t]).sum())} covered pixels, "
              f"{int((got[t] != ref_bgr[t]).any(-1).sum())} colour / {int((depth[t].view(np.uint32) != ref_depth[t].view(np.uint32)).sum())} depth mismatches")
    assert np.array_equal(depth.view(np.uint32), ref_depth.view(np.uint32)), tag
    assert np.array_equal(got, ref_bgr), tag


def _render_scene(ctx, s, view, frames=None, depth=True):
    W, H = s["width"], s["height"]
    T = len(s["sizes"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(s[k])).cuda() for k in ("points", "colors", "sizes", "pose")}
    bgr, dep = _outputs(T, W, H, s["pad"])
    ctx.render_points(dev["points"], dev["colors"], dev["sizes"], c_view(view), W, H, pose=dev["pose"],
                      frames=s["frames"] if frames is None else frames, depth=True, row_stride=3 * W + s["pad"], out=(bgr, dep if depth else None))
    ctx.synchronize()
    return bgr, dep


@pytest.mark.parametrize("name", sorted(render_scenes.SCENES))
def test_raw_arrays_bit_exact(ctx, name):
    """Several tracks of different sizes (0 included), points behind the eye and beyond z_far, NaN and infinite coordinates,
    exact depth ties between colours, squares across every image edge, frusta through the near and the far plane; widths 320,
    322 and 1277 with rows padded by 10 bytes; point sizes 1, 3, 4 and 15."""
    s = render_scenes.make(name)
    W, H = s["width"], s["height"]
    ref_bgr, ref_depth = ref_render.render(s["points"], s["colors"], s["sizes"], s["pose"], s["frames"], s["view"], W, H)
    bgr, dep = _render_scene(ctx, s, s["view"])
    _check(bgr, dep, ref_bgr, ref_depth, W, name)


@pytest.mark.parametrize("flags", [0, ref_render.AS_REFERENCE, ref_render.AS_REFERENCE | ref_render.FRUSTA], ids=["points_only", "as_reference", "as_reference_frusta"])
def test_raw_arrays_modes(ctx, flags):
    s = render_scenes.make("322x200_s1_padded")
    W, H = s["width"], s["height"]
    view = s["view"].replace(flags=flags, point_size=3, background=(3, 200, 77), frustum=(1, 2, 250))
    ref_bgr, ref_depth = ref_render.render(s["points"], s["colors"], s["sizes"], s["pose"], s["frames"], view, W, H)
    assert np.isfinite(ref_depth).sum() >= 1000
    bgr, dep = _render_scene(ctx, s, view)
    _check(bgr, dep, ref_bgr, ref_depth, W, f"flags {flags}")


def test_tie_goes_to_the_lower_index(ctx):
    """Two points at one place with different colours, at every point size: the lower index wins whichever comes first in
    memory order of the atomics; and a frustum sample never beats a point at the same depth bits (its order index is higher)."""
    W, H = 64, 48
    pts = np.zeros((1, 4, 4), np.float32)
    pts[0, :, :3] = [(0.05, 0.02, 2.0), (0.05, 0.02, 2.0), (-0.3, 0.1, 3.0), (-0.3, 0.1, 3.0)]
    cols = np.array([[[10, 20, 30], [200, 210, 220], [1, 2, 3], [4, 5, 6]]], np.uint8)
    for size in (1, 3, 4, 15):
        view = ref_render.View(np.eye(4, dtype=np.float32).reshape(16), 60, 60, W // 2, H // 2, point_size=size, flags=0)
        ref_bgr, ref_depth = ref_render.render(pts, cols, [4], None, 0, view, W, H)
        assert set(map(tuple, ref_bgr[0][np.isfinite(ref_depth[0])])) == {(10, 20, 30), (1, 2, 3)}
        bgr, dep = _outputs(1, W, H, 0)
        ctx.render_points(torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda(), torch.tensor([4], dtype=torch.int32, device="cuda"),
                          c_view(view), W, H, depth=True, row_stride=3 * W, out=(bgr, dep))
        ctx.synchronize()
        _check(bgr, dep, ref_bgr, ref_depth, W, f"size {size}")


def test_two_renders_are_identical(ctx):
    s = render_scenes.make("320x240_s3")
    a = [x.cpu().numpy() for x in _render_scene(ctx, s, s["view"])]
    b = [x.cpu().numpy() for x in _render_scene(ctx, s, s["view"])]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    # without the depth plane: the same image
    c, _ = _render_scene(ctx, s, s["view"], depth=False)
    assert np.array_equal(a[0], c.cpu().numpy())


def test_view_helpers_match_reference(ctx):
    for w, h in ((640, 480), (1277, 95)):
        v, r = capi.View.default(w, h), ref_render.default_view(w, h)
        g = ref_view(v)
        assert np.array_equal(g.mv.view(np.uint32), r.mv.view(np.uint32))
        assert (g.fu, g.fv, g.u0, g.v0, g.z_near, g.z_far, g.point_size, g.flags, g.box, g.background, g.frustum) == \
               (r.fu, r.fv, r.u0, r.v0, r.z_near, r.z_far, r.point_size, r.flags, r.box, r.background, r.frustum)


# ------------------------------------------------------------------ tracked maps
def _K(w, h):
    return np.array([[525, 0, w // 2], [0, 525, h // 2], [0, 0, 1]], np.float32)     # src/vslam.cpp:32


def _track(ctx, shape):
    seed, w, h, pad = shape
    bgr = synth.sequences_numpy(seed, TRACKS, FRAMES, w, h)
    seeds = (np.arange(TRACKS * (FRAMES - 1), dtype=np.uint32).reshape(TRACKS, FRAMES - 1) * 7919 + seed * 100003).astype(np.uint32)
    if pad:
        rows = np.full((TRACKS, FRAMES, h, 3 * w + pad), PAD_BYTE, np.uint8)
        rows[..., :3 * w] = bgr.reshape(TRACKS, FRAMES, h, 3 * w)
        d_bgr, width = torch.from_numpy(rows).cuda(), w
    else:
        d_bgr, width = torch.from_numpy(bgr).cuda(), None
    pmap = capi.PointMap(ctx, TRACKS, FRAMES, KP, FRAMES * MAXC, 6 * FRAMES * MAXC)
    pat = torch.from_numpy(synth.brief_pattern()).cuda()
    ca, sa = synth.keypoint_rotation()
    ctx.track_sequences(pmap, d_bgr, MAXC, ca, sa, pat, torch.from_numpy(seeds.view(np.int32).copy()).cuda(), HYP, THR, _K(w, h), width=width)
    ctx.synchronize()
    return pmap


def _map_view(v, W, H, **fields):
    """A look_at view placed from the map's median point: from behind and above the first camera, far enough to see the bulk
    of the points and the frusta at the origin."""
    pts = np.concatenate([v["points"][t, :v["sizes"][t], :3] for t in range(len(v["sizes"]))]).astype(np.float64)
    pts = pts[np.isfinite(pts).all(1)]
    med = np.median(pts, axis=0)
    spread = float(np.median(np.abs(pts - med))) + 1.0
    eye = -2.0 * spread * (med / (np.linalg.norm(med) + 1e-9)) + np.array([0.4 * spread, -0.6 * spread, 0.0])
    return capi.View.look_at(eye, med, (0, -1, 0), W, H, fu=0.6 * W, fv=0.6 * W, z_near=0.05, z_far=1e6, **fields)


@pytest.mark.parametrize("shape", SHAPES, ids=["320x240", "322x200_padded"])
def test_tracked_maps_bit_exact(ctx, shape):
    W, H, pad = 322, 241, 10
    pmap = _track(ctx, shape)
    try:
        before = pmap.view()
        assert (before["sizes"] > 50).all() and before["frames"] == FRAMES
        cases = [("frusta", dict(point_size=3), None), ("no_frusta", dict(point_size=3, flags=0), None),
                 ("as_reference", dict(point_size=5, flags=capi.RENDER_AS_REFERENCE | capi.RENDER_FRUSTA), None),
                 ("subset", dict(point_size=3), (1, 2))]
        for tag, fields, tracks in cases:
            view = _map_view(before, W, H, **fields)
            lo, count = tracks or (0, TRACKS)
            sl = slice(lo, lo + count)
            ref_bgr, ref_depth = ref_render.render(before["points"][sl], before["colors"][sl], before["sizes"][sl], before["pose"][sl],
                                                   before["frames"], ref_view(view), W, H)
            for t in range(count):
                nonbg = int((ref_bgr[t] != np.array(ref_view(view).background, np.uint8)).any(-1).sum())
                print(f"{tag} track {lo + t}: {nonbg} non-background pixels in the reference image")
                assert nonbg >= 200
            bgr, dep = _outputs(count, W, H, pad)
            pmap.render(view, W, H, tracks=tracks, depth=True, row_stride=3 * W + pad, out=(bgr, dep))
            ctx.synchronize()
            _check(bgr, dep, ref_bgr, ref_depth, W, tag)
        after = pmap.view()
        for k in before:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), f"the render wrote to the map's {k}"
        # the convenience form: new tensors, no padding
        view = _map_view(before, W, H, point_size=3)
        img = pmap.render(view, W, H)
        assert img.shape == (TRACKS, H, W, 3) and img.dtype == torch.uint8
        ref_bgr, _ = ref_render.render(before["points"], before["colors"], before["sizes"], before["pose"], FRAMES, ref_view(view), W, H)
        assert np.array_equal(img.cpu().numpy(), ref_bgr)
    finally:
        pmap.close()


# ------------------------------------------------------------------ errors
def test_invalid_arguments_leave_the_output_untouched(ctx):
    W, H, T, M = 32, 24, 2, 16
    pts = torch.zeros((T, M, 4), dtype=torch.float32, device="cuda")
    cols = torch.zeros((T, M, 3), dtype=torch.uint8, device="cuda")
    sizes = torch.full((T,), M, dtype=torch.int32, device="cuda")
    pose = torch.zeros((T, 2, 16), dtype=torch.float32, device="cuda")
    good = capi.View.default(W, H)
    bgr, dep = _outputs(T, W, H, 0)
    lib, C = ctx.lib, capi.C

    def call(points=pts, colors=cols, sz=sizes, tracks=T, stride=M, po=pose, frames=2, pstride=2, view=good, w=W, h=H, row=3 * W,
             out=bgr, handle=None):
        return lib.vslam_render_points(ctx.handle if handle is None else handle, capi._ptr(points), capi._ptr(colors), capi._ptr(sz),
                                       C.c_int(tracks), C.c_int(stride), capi._ptr(po), C.c_int(frames), C.c_int(pstride),
                                       C.byref(view) if view is not None else C.c_void_p(0), C.c_int(w), C.c_int(h), C.c_int(row),
                                       capi._ptr(out), capi._ptr(dep))
    bad = dict(null_ctx=dict(handle=C.c_void_p(0)), null_points=dict(points=None), null_colors=dict(colors=None), null_sizes=dict(sz=None),
               null_view=dict(view=None), null_out=dict(out=None), null_pose_with_frusta=dict(po=None),
               tracks_0=dict(tracks=0), tracks_neg=dict(tracks=-1), stride_0=dict(stride=0), width_0=dict(w=0), height_neg=dict(h=-3),
               frames_neg=dict(frames=-1), pose_stride_short=dict(pstride=1), row_stride_short=dict(row=3 * W - 1),
               point_size_0=dict(view=good.copy(point_size=0)), point_size_16=dict(view=good.copy(point_size=16)),
               z_near_0=dict(view=good.copy(z_near=0.0)), z_near_neg=dict(view=good.copy(z_near=-1.0)),
               z_near_nan=dict(view=good.copy(z_near=float("nan"))), z_near_inf=dict(view=good.copy(z_near=float("inf"), z_far=float("inf"))),
               z_far_below_near=dict(view=good.copy(z_near=2.0, z_far=1.0)))
    for tag, kw in bad.items():
        assert call(**kw) == -1, tag                                     # VSLAM_ERR_INVALID
    assert call(w=16385, row=3 * 16385) == -4 and call(h=16385) == -4    # VSLAM_ERR_CAPACITY, nothing queued either
    pmap = capi.PointMap(ctx, 3, 2, 8, 16, 32)
    try:
        def map_call(lo, count, m=None, view=good, out=bgr):
            return lib.vslam_map_render(ctx.handle, pmap.handle if m is None else m, C.c_int(lo), C.c_int(count),
                                        C.byref(view) if view is not None else C.c_void_p(0), C.c_int(W), C.c_int(H), C.c_int(3 * W),
                                        capi._ptr(out), capi._ptr(dep))
        for lo, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (0, -1), (2 ** 31 - 1, 2)):
            assert map_call(lo, count) == -1, (lo, count)
        assert map_call(0, 1, m=C.c_void_p(0)) == -1 and map_call(0, 1, view=None) == -1 and map_call(0, 1, out=None) == -1
        assert map_call(0, 2, view=good.copy(point_size=16)) == -1
        ctx.synchronize()
        assert (bgr == PAD_BYTE).all() and (dep == -7.0).all(), "a rejected call wrote to its output"
        assert call() == 0 and map_call(1, 2) == 0                      # and the good calls are good
        ctx.synchronize()
        assert not (bgr == PAD_BYTE).all()
    finally:
        pmap.close()


# ------------------------------------------------------------------ the C++ surface
def test_display_demo_matches_python_call(ctx, tmp_path):
    """tests/native/display_demo.cpp: Display::render of host-side arrays and vslam::render_map of a device map built through
    include/vslam/PointMap.h give the bytes of the Python call on the same arrays (and of the reference)."""
    from vslam_amd import build
    build.build_host()
    exe = str(tmp_path / "display_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "display_demo.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "vslam_amd")], check=True)
    W, H = 322, 200
    s = render_scenes.make("322x200_s1_padded")
    n = 3100
    pts, cols, pose = s["points"][3, :n], s["colors"][3, :n], s["pose"][3, :s["frames"]]
    view = c_view(s["view"].replace(point_size=3))
    w, h, maxc, hyp, frames = 320, 240, 400, 256, 5
    video = synth.sequences_numpy(2, 1, frames, w, h)[0]
    seeds = (np.arange(frames - 1, dtype=np.uint32) * 7919 + 5).astype(np.uint32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("2i", W, H))
        f.write(bytes(view))
        f.write(struct.pack("i", n)); f.write(pts.tobytes()); f.write(cols.tobytes())
        f.write(struct.pack("i", len(pose))); f.write(pose.tobytes())
        f.write(struct.pack("5i", w, h, maxc, hyp, frames)); f.write(seeds.tobytes()); f.write(video.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=180)
    buf = open(fout, "rb").read()
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a
    shot = take(np.uint8, W * H * 3).reshape(H, W, 3)
    seen = take(np.uint8, W * H * 3).reshape(H, W, 3)
    size = int(take(np.int32, 1)[0])
    mp = take(np.float32, 4 * size).reshape(1, size, 4)
    mc = take(np.uint8, 3 * size).reshape(1, size, 3)
    nf = int(take(np.int32, 1)[0])
    mpose = take(np.float32, 16 * nf).reshape(1, nf, 16)
    assert off == len(buf) and size > 50 and nf == frames

    def python_call(p, c, sz, po):
        img = ctx.render_points(torch.from_numpy(p.copy()).cuda(), torch.from_numpy(c.copy()).cuda(),
                                torch.tensor([sz], dtype=torch.int32, device="cuda"), view, W, H, pose=torch.from_numpy(po.copy()).cuda())
        ctx.synchronize()
        return img.cpu().numpy()[0]
    # 1. Display::render(ds)
    assert np.array_equal(shot, python_call(pts[None], cols[None], n, pose[None]))
    ref_bgr, _ = ref_render.render(pts[None], cols[None], [n], pose[None], len(pose), ref_view(view), W, H)
    assert np.array_equal(shot, ref_bgr[0]) and (shot != 0).any(-1).sum() >= 1000
    # 2. vslam::render_map of the device map == the Python call on what sync_to_host() copied out of it
    assert np.array_equal(seen, python_call(mp, mc, size, mpose))
    ref_bgr, _ = ref_render.render(mp, mc, [size], mpose, nf, ref_view(view), W, H)
    assert np.array_equal(seen, ref_bgr[0]) and (seen != 0).any(-1).sum() >= 50       # the frusta at the origin, at least
