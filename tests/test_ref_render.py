"""tests/ref_render.py -- the numpy restatement of the renderer's contract (include/vslam_amd.h, "the view of the map") that the
GPU test compares against bit for bit -- held to definitions of its own: a sequential painter written in scalar Python from
the header's text, the properties a rasterised line has to have, look_at's geometry, the reference-mode colour table, and the
non-triviality of every scene the GPU test renders.  No GPU."""
import math
import struct

import numpy as np
import pytest

import ref_render
import render_scenes


# ------------------------------------------------------------------ a sequential painter, scalar Python floats (IEEE double)
def _f64(v):
    return float(np.float32(v))


def _xf(M, p):
    return tuple(((_f64(M[4 * i]) * p[0] + _f64(M[4 * i + 1]) * p[1]) + _f64(M[4 * i + 2]) * p[2]) + _f64(M[4 * i + 3]) for i in range(3))


def _mix(a, b, t):
    return a * (1.0 - t) + b * t


def _f32_bits(x):
    try:
        return struct.unpack("<I", struct.pack("<f", x))[0]
    except OverflowError:
        return 0x7F800000


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan


def _segment_pixels(a, b, view, W, H):
    """[(x, y, f32 depth bits)] of one eye-space segment, sample by sample."""
    if not all(math.isfinite(v) for v in a + b):
        return []
    zn, zf = _f64(view.z_near), _f64(view.z_far)
    if (a[2] < zn and b[2] < zn) or (a[2] > zf and b[2] > zf):
        return []
    ends = []
    for p in (a, b):
        if p[2] < zn or p[2] > zf:
            plane = zn if p[2] < zn else zf
            t = (plane - a[2]) / (b[2] - a[2])
            p = (_mix(a[0], b[0], t), _mix(a[1], b[1], t), plane)
        ends.append(p)
    fu, fv, u0, v0 = (_f64(v) for v in (view.fu, view.fv, view.u0, view.v0))
    (Ua, Va, qa), (Ub, Vb, qb) = [(fu * p[0] / p[2] + u0, fv * p[1] / p[2] + v0, 1.0 / p[2]) for p in ends]
    if not all(math.isfinite(v) for v in (Ua, Va, qa, Ub, Vb, qb)):
        return []
    s0, s1 = 0.0, 1.0
    dU, dV = Ub - Ua, Vb - Va
    for p, q in ((-dU, Ua + 0.5), (dU, (W + 0.5) - Ua), (-dV, Va + 0.5), (dV, (H + 0.5) - Va)):
        if p == 0.0:
            if q < 0.0:
                return []
            continue
        r = q / p
        if p < 0.0:
            if r > s1:
                return []
            s0 = max(s0, r)
        else:
            if r < s0:
                return []
            s1 = min(s1, r)
    cUa, cVa, cqa = _mix(Ua, Ub, s0), _mix(Va, Vb, s0), _mix(qa, qb, s0)
    cUb, cVb, cqb = _mix(Ua, Ub, s1), _mix(Va, Vb, s1), _mix(qa, qb, s1)
    m = max(abs(cUb - cUa), abs(cVb - cVa))
    if not m <= 65536.0:
        return []
    n = max(1, math.ceil(m))
    out = []
    for k in range(n + 1):
        t = k / n
        x, y = math.floor(_mix(cUa, cUb, t)), math.floor(_mix(cVa, cVb, t))
        if 0 <= x < W and 0 <= y < H:
            out.append((x, y, _f32_bits(1.0 / _mix(cqa, cqb, t))))
    return out


def painter(points, colors, size, pose, frames, view, W, H):
    """Primitives visited one by one in order; per pixel the best (depth bits, order) so far is kept, a LATER primitive
    replacing it only when strictly smaller."""
    best = {}
    size = min(max(int(size), 0), len(points))
    n = (size + 3) // 4 if view.flags & ref_render.AS_REFERENCE else size
    zn, zf = _f64(view.z_near), _f64(view.z_far)
    fu, fv, u0, v0 = (_f64(v) for v in (view.fu, view.fv, view.u0, view.v0))
    s = view.point_size

    def put(x, y, bits, order):
        if (x, y) not in best or (bits, order) < best[(x, y)]:
            best[(x, y)] = (bits, order)
    for i in range(n):
        e = _xf(view.mv, tuple(_f64(c) for c in points[i][:3]))
        if not all(math.isfinite(c) for c in e) or not (zn <= e[2] <= zf):
            continue
        u, v = _div(fu * e[0], e[2]) + u0, _div(fv * e[1], e[2]) + v0
        if not (math.isfinite(u) and math.isfinite(v)) or abs(math.floor(u)) > 2 ** 30 or abs(math.floor(v)) > 2 ** 30:
            continue
        px, py = math.floor(u), math.floor(v)
        for y in range(py - (s - 1) // 2, py + s // 2 + 1):
            for x in range(px - (s - 1) // 2, px + s // 2 + 1):
                if 0 <= x < W and 0 <= y < H:
                    put(x, y, _f32_bits(e[2]), i)
    if view.flags & ref_render.FRUSTA:
        w = np.float32(view.box[0])
        h, z = np.float32(w * np.float32(view.box[1])), np.float32(w * np.float32(view.box[2]))
        O, PP, PM, MM, MP = (0.0, 0.0, 0.0), (w, h, z), (w, -h, z), (-w, -h, z), (-w, h, z)
        box = [(O, PP), (O, PM), (O, MM), (O, MP), (PP, PM), (MP, MM), (MP, PP), (MM, PM)]      # src/display.cpp:129-148
        for f in range(frames):
            for k, (A, B) in enumerate(box):
                a = _xf(view.mv, _xf(pose[f], tuple(float(c) for c in A)))
                b = _xf(view.mv, _xf(pose[f], tuple(float(c) for c in B)))
                for x, y, bits in _segment_pixels(a, b, view, W, H):
                    put(x, y, bits, n + 8 * f + k)
    bgr = np.empty((H, W, 3), np.uint8)
    bgr[:] = view.background
    depth = np.full((H, W), np.inf, np.float32)
    for (x, y), (bits, order) in best.items():
        depth[y, x] = np.array([bits], np.uint32).view(np.float32)[0]
        if order >= n:
            bgr[y, x] = view.frustum
        elif view.flags & ref_render.AS_REFERENCE:
            b, g, r = (int(c) for c in colors[order])
            bgr[y, x] = [ref_render.reference_channel(r), ref_render.reference_channel(g), ref_render.reference_channel(b)]
        else:
            bgr[y, x] = colors[order]
    return bgr, depth


def _small_scene(seed, W, H, n, frames, point_size, flags):
    rng = np.random.default_rng(seed)
    eye = rng.uniform(-1, 1, 3) + np.array([0, 0, -4.0])
    view = ref_render.View(ref_render.look_at(eye, rng.uniform(-.3, .3, 3), (0, 1, 0)), 0.8 * W, 0.8 * W, W // 2, H // 2,
                           z_near=0.3, z_far=7.5, point_size=point_size, flags=flags, background=(9, 8, 7), frustum=(200, 100, 50))
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = rng.uniform(-3, 3, (n, 3)) * np.array([1.5, 1.5, 2.0])
    pts[:, 3] = rng.uniform(-2, 2, n)
    pts[n // 2:n // 2 + n // 8] = pts[:n // 8]                     # depth ties
    pts[n - 6:n - 3, 0] = (np.nan, np.inf, -np.inf)
    cols = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    pose = np.stack([render_scenes._rigid(rng, 2.0) for _ in range(frames)])
    if frames:
        pose[0, 3:12:4] = (eye + 0.1).astype(np.float32)            # around the viewer: crosses the near plane
    return pts, cols, pose, view


@pytest.mark.parametrize("seed,point_size,flags", [(1, 1, 1), (2, 3, 1), (3, 4, 0), (4, 15, 1), (5, 2, 3), (6, 3, 2)])
def test_ref_render_equals_sequential_painter(seed, point_size, flags):
    W, H, frames = 97, 61, 4
    n = 1600 if flags & ref_render.AS_REFERENCE else 400          # reference mode submits a quarter of the points
    pts, cols, pose, view = _small_scene(seed, W, H, n, frames, point_size, flags)
    for size in (n, n - 3, 0):
        bgr, depth = ref_render.render(pts[None], cols[None], [size], pose[None], frames, view, W, H)
        pb, pd = painter(pts, cols, size, pose, frames, view, W, H)
        hit = np.isfinite(pd)
        print(f"seed {seed} size {size}: {int(hit.sum())} covered pixels")
        assert size == 0 or hit.sum() > 150
        assert np.array_equal(depth[0].view(np.uint32), pd.view(np.uint32))
        assert np.array_equal(bgr[0], pb)


# ------------------------------------------------------------------ lines
def _line_view(W, H, **kw):
    return ref_render.View(np.eye(4, dtype=np.float32).reshape(16), 100.0, 100.0, W / 2, H / 2, z_near=0.2, z_far=1e4, **kw)


def _dist_to_segment(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    L = dx * dx + dy * dy
    t = 0.0 if L == 0 else min(1.0, max(0.0, ((px - ax) * dx + (py - ay) * dy) / L))
    return math.hypot(px - (ax + t * dx), py - (ay + t * dy))


def test_line_properties():
    W, H = 160, 120
    view = _line_view(W, H)
    rng = np.random.default_rng(5)
    checked_inside = 0
    for it in range(400):
        a = rng.uniform(-3, 3, 3) * (1, 1, 0) + (0, 0, rng.uniform(0.5, 6))
        b = rng.uniform(-3, 3, 3) * (1, 1, 0) + (0, 0, rng.uniform(0.5, 6))
        if it % 4 == 0:
            b[2] = -rng.uniform(0.1, 5)                           # an end behind the eye
        if it % 7 == 0:
            a[:2] *= 1e4                                          # an end far off screen
        x, y, d, cost = ref_render.segment_samples(tuple(a), tuple(b), view, W, H)
        assert cost <= 2 * (W + H)
        if len(x) == 0:
            continue
        # the ideal segment on the screen: the projection of the part in front of the near plane (a projective map keeps lines)
        A, B = a.copy(), b.copy()
        for P in (A, B):
            if P[2] < 0.2:
                t = (0.2 - a[2]) / (b[2] - a[2])
                P[:] = a + t * (b - a)
        ia = (100 * A[0] / A[2] + W / 2, 100 * A[1] / A[2] + H / 2)
        ib = (100 * B[0] / B[2] + W / 2, 100 * B[1] / B[2] + H / 2)
        for px, py in zip(x, y):
            assert _dist_to_segment(px + 0.5, py + 0.5, *ia, *ib) <= 1.0, (it, px, py)
        # 8-connected: consecutive samples inside the image move by at most one pixel per axis (samples leave the image only
        # at the ends of the clipped run, the clip rectangle being half a pixel larger than the image)
        assert (np.abs(np.diff(x)) <= 1).all() and (np.abs(np.diff(y)) <= 1).all(), it
        for e, (u, v) in ((a, ia), (b, ib)):
            if e[2] >= 0.2 and 0 <= u < W and 0 <= v < H:
                assert ((x == math.floor(u)) & (y == math.floor(v))).any(), (it, "endpoint")
                checked_inside += 1
        assert (d > 0).all() and np.isfinite(d).all()
        lo, hi = min(A[2], B[2]), max(A[2], B[2])
        assert (d >= np.float32(lo) * (1 - 1e-6)).all() and (d <= np.float32(hi) * (1 + 1e-6)).all()
    assert checked_inside > 100


def test_line_depth_is_perspective_correct():
    """Along a segment the depth at a pixel is the eye z of the 3-D point that projects there: 1 / z, not z, is linear."""
    W, H = 200, 100
    view = _line_view(W, H)
    a, b = (-0.9, 0.1, 1.0), (3.5, -0.2, 8.0)
    x, y, d, _ = ref_render.segment_samples(a, b, view, W, H)
    assert len(x) > 80
    for px, dz in zip(x, d):
        # the point of the 3-D line whose projection has u = px + 0.5 (roughly the sample): solve for s on a + s (b - a)
        u = (px + 0.5 - W / 2) / 100
        s = (u * a[2] - a[0]) / ((b[0] - a[0]) - u * (b[2] - a[2]))
        z = a[2] + s * (b[2] - a[2])
        assert abs(float(dz) - z) <= 0.05 * z + 0.08, (px, dz, z)      # half a pixel of slack along a steep depth ramp


def test_degenerate_and_dropped_segments():
    W, H = 64, 48
    view = _line_view(W, H)
    x, y, d, cost = ref_render.segment_samples((0.01, 0.01, 2.0), (0.01, 0.01, 2.0), view, W, H)
    assert list(zip(x, y)) == [(32, 24), (32, 24)] and cost == 2              # a point-like segment: n = 1, both samples
    assert ref_render.segment_samples((0, 0, -1.0), (1, 1, -2.0), view, W, H)[3] == 0          # behind the eye
    assert ref_render.segment_samples((0, 0, 2e4), (1, 1, 3e4), view, W, H)[3] == 0            # beyond z_far
    assert ref_render.segment_samples((50.0, 0, 1.0), (50.0, 1, 2.0), view, W, H)[3] == 0      # off screen
    assert ref_render.segment_samples((math.nan, 0, 1.0), (0.0, 1, 2.0), view, W, H)[3] == 0
    assert ref_render.segment_samples((0, 0, 1.0), (0.0, math.inf, 2.0), view, W, H)[3] == 0


# ------------------------------------------------------------------ look_at, the default view
def test_look_at_is_orthonormal_right_handed_and_maps_eye_to_origin():
    rng = np.random.default_rng(3)
    for _ in range(50):
        eye, target = rng.uniform(-5, 5, 3), rng.uniform(-5, 5, 3)
        up = rng.normal(size=3)
        mv = ref_render.look_at(eye, target, up).astype(np.float64).reshape(4, 4)
        R, t = mv[:3, :3], mv[:3, 3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)
        assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-6)              # right-handed
        assert np.allclose(R @ eye + t, 0, atol=1e-5)                        # the eye is the origin
        f = (target - eye) / np.linalg.norm(target - eye)
        assert np.allclose(R @ f, (0, 0, 1), atol=1e-6)                      # looking down +z
        assert (R @ target + t)[2] > 0
        assert (R @ up)[1] <= 1e-6                                           # `up` points to -y on the screen (y is down)
        assert tuple(mv[3]) == (0, 0, 0, 1)
    with pytest.raises(ValueError):
        ref_render.look_at((1, 2, 3), (1, 2, 3), (0, 1, 0))
    with pytest.raises(ValueError):
        ref_render.look_at((0, 0, 0), (0, 2, 0), (0, 1, 0))


def test_default_view_is_the_reference_window():
    v = ref_render.default_view(641, 481)
    assert (v.fu, v.fv, v.u0, v.v0) == (420, 420, 320, 240)                  # src/display.cpp:25, W / 2 in integers
    assert v.z_near == np.float32(0.2) and v.z_far == 10000 and v.point_size == 1 and v.flags == ref_render.FRUSTA
    assert v.box == (1.0, 0.75, np.float32(0.6)) and v.background == (0, 0, 0) and v.frustum == (255, 0, 0)
    mv = v.mv.astype(np.float64).reshape(4, 4)
    assert np.allclose(mv[:3, :3] @ np.array([-2, 2, -2.0]) + mv[:3, 3], 0, atol=1e-6)
    origin = mv[:3, 3]
    assert abs(origin[0]) < 1e-6 and abs(origin[1]) < 1e-6 and origin[2] == pytest.approx(math.sqrt(12), abs=1e-6)


# ------------------------------------------------------------------ reference mode
def test_reference_colour_table_and_point_count():
    for c in range(256):
        signed = c - 256 if c >= 128 else c                                  # the byte as glColor3b's GLbyte
        expect = max(0, min(255, round((2 * signed + 1) / 255 * 255)))       # (2c + 1) / 255, clamped, in an 8-bit buffer
        assert ref_render.reference_channel(c) == expect, c
    assert [ref_render.reference_channel(c) for c in (0, 1, 127, 128, 255)] == [1, 3, 255, 0, 0]
    for size in range(10):
        assert ref_render.reference_point_count(size) == len(range(0, size, 4)) == math.ceil(size / 4)
    # through the renderer: one point in the middle, stored (b, g, r) = (10, 200, 100) -> output b = 2 * 100 + 1, g = 0, r = 21
    W, H = 9, 9
    view = _line_view(W, H, flags=ref_render.AS_REFERENCE)
    pts = np.zeros((1, 8, 4), np.float32)
    pts[0, :, 2] = 1.0
    pts[0, :, 0] = np.arange(8) * 0.01                                        # point i at column 4 + i
    cols = np.tile(np.array([10, 200, 100], np.uint8), (1, 8, 1))
    for size, drawn in ((8, 2), (5, 2), (4, 1), (1, 1), (0, 0)):
        bgr, depth = ref_render.render(pts, cols, [size], None, 0, view, W, H)
        assert int(np.isfinite(depth).sum()) == drawn
        for i in range(drawn):
            assert tuple(bgr[0, 4, 4 + i]) == (201, 0, 21)


# ------------------------------------------------------------------ the GPU test's scenes
@pytest.mark.parametrize("name", sorted(render_scenes.SCENES))
def test_gpu_scenes_are_not_trivial(name):
    s = render_scenes.make(name)
    W, H, view = s["width"], s["height"], s["view"]
    covered = twice = 0
    for t, size in enumerate(s["sizes"]):
        cov = ref_render.coverage(s["points"][t], size, s["pose"][t], s["frames"], view, W, H)
        print(f"{name} track {t}: size {size}, {int((cov > 0).sum())} covered, {int((cov > 1).sum())} reached twice or more")
        if size:
            assert (cov > 0).sum() >= 1000 and (cov > 1).sum() >= 50
        covered += int((cov > 0).sum())
        twice += int((cov > 1).sum())
    assert covered >= 1000 and twice >= 50
    # what the scene is there to exercise, on track 0
    P = s["points"][0].astype(np.float64)
    ex, ey, ez = ref_render.xf(view.mv, P[:, 0], P[:, 1], P[:, 2])
    assert (ez < 0).sum() > 50 and (ez > float(view.z_far)).sum() > 50 and (~np.isfinite(ez) | ~np.isfinite(ex) | ~np.isfinite(ey)).sum() >= 20
    bgr, depth = ref_render.render(s["points"][:1], s["colors"][:1], s["sizes"][:1], s["pose"][:1], s["frames"], view, W, H)
    # exact depth ties between different colours were decided by the index
    bits = np.float32(ez).view(np.uint32)
    tie_lo, tie_hi = np.arange(7, 27), np.arange(len(P) - 40, len(P) - 20)
    assert np.array_equal(bits[tie_lo], bits[tie_hi])
    vis = [i for i in tie_lo if np.isfinite(ez[i]) and float(view.z_near) <= ez[i] <= float(view.z_far)]
    assert vis
    # every image edge is touched by a square that continues outside
    with np.errstate(all="ignore"):
        pu = np.floor(float(view.fu) * ex / ez + float(view.u0))
        pv = np.floor(float(view.fv) * ey / ez + float(view.v0))
    ok = np.isfinite(ez) & (ez >= float(view.z_near)) & (ez <= float(view.z_far))
    lo, hi = (view.point_size - 1) // 2, view.point_size // 2
    if view.point_size > 1:
        inx, iny = (pu >= 0) & (pu < W), (pv >= 0) & (pv < H)
        assert (ok & iny & (pu - lo < 0) & (pu + hi >= 0)).any() and (ok & iny & (pu + hi >= W) & (pu - lo < W)).any()
        assert (ok & inx & (pv - lo < 0) & (pv + hi >= 0)).any() and (ok & inx & (pv + hi >= H) & (pv - lo < H)).any()
    # a frustum segment crosses the near plane, one frustum is wholly behind the eye, one straddles z_far
    zs = []
    for f in range(s["frames"]):
        for A, B in ref_render.SEGMENTS:
            a, b = ref_render.segment_eye(s["pose"][0, f], ref_render.box_corner(A, view), ref_render.box_corner(B, view), view)
            zs.append((f, a[2], b[2]))
    zn, zf = float(view.z_near), float(view.z_far)
    assert any(min(a, b) < zn <= max(a, b) for _, a, b in zs)
    assert any(max(a, b) < 0 for _, a, b in zs)
    assert any(min(a, b) <= zf < max(a, b) for _, a, b in zs)
    assert (bgr[0].reshape(-1, 3) == np.array(view.frustum, np.uint8)).all(axis=1).sum() > 30
