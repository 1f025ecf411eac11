"""numpy float64 restatement of the map renderer's contract (include/vslam_amd.h, "the view of the map"): what
vslam_render_points / vslam_map_render must produce bit for bit.  Written from the header's text, vectorised per primitive kind;
tests/test_ref_render.py holds it to a sequential painter and to the properties a line has to have, so that the GPU test
does not compare two copies of one mistake.

Every operation is a float64 numpy operation in the header's order (numpy never fuses a product into a sum), so the values are
the ones the kernels' `double` arithmetic produces with contraction off."""
import math

import numpy as np

FRUSTA, AS_REFERENCE = 1, 2
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
# draw_box's eight segments as (sign of w, sign of h, has z) per end, src/display.cpp:129-148
_O, _PP, _PM, _MM, _MP = (0, 0, 0), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1)
SEGMENTS = [(_O, _PP), (_O, _PM), (_O, _MM), (_O, _MP), (_PP, _PM), (_MP, _MM), (_MP, _PP), (_MM, _PM)]


class View:
    """vslam_view with numpy members."""

    def __init__(self, mv, fu, fv, u0, v0, z_near=0.2, z_far=10000.0, point_size=1, flags=FRUSTA, box=(1.0, 0.75, 0.6),
                 background=(0, 0, 0), frustum=(255, 0, 0)):
        self.mv = np.asarray(mv, np.float32).reshape(16).copy()
        self.fu, self.fv, self.u0, self.v0 = (np.float32(v) for v in (fu, fv, u0, v0))
        self.z_near, self.z_far = np.float32(z_near), np.float32(z_far)
        self.point_size, self.flags = int(point_size), int(flags)
        self.box = tuple(np.float32(v) for v in box)
        self.background = tuple(int(v) for v in background)
        self.frustum = tuple(int(v) for v in frustum)

    def replace(self, **kw):
        v = View(self.mv, self.fu, self.fv, self.u0, self.v0, self.z_near, self.z_far, self.point_size, self.flags, self.box,
                 self.background, self.frustum)
        for k, val in kw.items():
            assert hasattr(v, k), k
            setattr(v, k, val)
        return v


def look_at(eye, target, up):
    """vslam_view_look_at: (16,) float32."""
    e, t, u = (np.asarray(v, np.float64) for v in (eye, target, up))

    def normalize(v):
        return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    with np.errstate(all="ignore"):
        f = normalize(t - e)
        r = normalize(cross(f, u))
        d = cross(f, r)
    R = np.stack([r, d, f])
    if not np.isfinite(R).all():
        raise ValueError("degenerate look_at")
    tr = -((R[:, 0] * e[0] + R[:, 1] * e[1]) + R[:, 2] * e[2])
    mv = np.zeros(16, np.float64)
    mv.reshape(4, 4)[:3, :3] = R
    mv.reshape(4, 4)[:3, 3] = tr
    mv[15] = 1.0
    return mv.astype(np.float32)


def default_view(width, height):
    """vslam_view_default."""
    return View(look_at((-2, 2, -2), (0, 0, 0), (0, 1, 0)), 420, 420, width // 2, height // 2)


def reference_channel(c):
    """[OpenGL, from memory] glColor3b of a stored byte, as an 8-bit framebuffer holds it."""
    return 2 * c + 1 if c < 128 else 0


_REF_LUT = np.array([reference_channel(c) for c in range(256)], np.uint8)


def reference_point_count(size):
    """Vertices draw_points_colors submits: for (i = 0; i < size; i += 4)."""
    return (size + 3) // 4


def xf(M, x, y, z):
    """Rows 0..2 of the row-major 4 x 4 M (16 float32) applied to (x, y, z, 1), float64, left to right."""
    M = np.asarray(M, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return tuple(((M[4 * i] * x + M[4 * i + 1] * y) + M[4 * i + 2] * z) + M[4 * i + 3] for i in range(3))


def mix(a, b, t):
    return a * (1.0 - t) + b * t


def _keys(depth32, order):
    return (depth32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order.astype(np.uint64)


def point_samples(points, n, view, width, height):
    """(pixel index, key) arrays of the map points 0 .. n - 1 of one track."""
    P = np.asarray(points, np.float32)[:n].astype(np.float64)
    with np.errstate(all="ignore"):
        ex, ey, ez = xf(view.mv, P[:, 0], P[:, 1], P[:, 2])
        zn, zf = np.float64(view.z_near), np.float64(view.z_far)
        ok = np.isfinite(ex) & np.isfinite(ey) & np.isfinite(ez) & (ez >= zn) & (ez <= zf)
        pu = np.floor(np.float64(view.fu) * ex / ez + np.float64(view.u0))
        pv = np.floor(np.float64(view.fv) * ey / ez + np.float64(view.v0))
        ok &= (np.abs(pu) <= 2.0 ** 30) & (np.abs(pv) <= 2.0 ** 30)      # NaN compares false
    idx = np.nonzero(ok)[0]
    px, py = pu[idx].astype(np.int64), pv[idx].astype(np.int64)
    key = _keys(ez[idx].astype(np.float32), idx)
    s = view.point_size
    lo, hi = (s - 1) // 2, s // 2
    pix, keys = [], []
    for dy in range(-lo, hi + 1):
        for dx in range(-lo, hi + 1):
            x, y = px + dx, py + dy
            m = (x >= 0) & (x < width) & (y >= 0) & (y < height)
            pix.append((y[m] * width + x[m]))
            keys.append(key[m])
    if not pix:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    return np.concatenate(pix), np.concatenate(keys)


def box_corner(sign, view):
    """A corner of draw_box in camera coordinates: h and z are float32 products, as the reference forms them."""
    w = view.box[0]
    h = np.float32(w * view.box[1])
    z = np.float32(w * view.box[2])
    return (np.float64(sign[0]) * np.float64(w), np.float64(sign[1]) * np.float64(h), np.float64(sign[2]) * np.float64(z))


def segment_eye(pose, A, B, view):
    """Both ends of a camera-space segment in eye space."""
    a = xf(view.mv, *xf(pose, *A))
    b = xf(view.mv, *xf(pose, *B))
    return a, b


def segment_samples(a, b, view, width, height):
    """(x, y, depth32) of the samples of the eye-space segment a -> b that fall inside the image, and how many samples were
    stepped (the cost)."""
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), 0)
    a = tuple(np.float64(v) for v in a)
    b = tuple(np.float64(v) for v in b)
    if not all(math.isfinite(v) for v in a + b):
        return none
    zn, zf = np.float64(view.z_near), np.float64(view.z_far)
    if (a[2] < zn and b[2] < zn) or (a[2] > zf and b[2] > zf):
        return none

    def zclip(p):
        for plane, out in ((zn, p[2] < zn), (zf, p[2] > zf)):
            if out:
                t = (plane - a[2]) / (b[2] - a[2])
                return (mix(a[0], b[0], t), mix(a[1], b[1], t), plane)
        return p
    ends = [zclip(a), zclip(b)]
    fu, fv, u0, v0 = (np.float64(v) for v in (view.fu, view.fv, view.u0, view.v0))
    with np.errstate(all="ignore"):
        proj = [(fu * p[0] / p[2] + u0, fv * p[1] / p[2] + v0, np.float64(1.0) / p[2]) for p in ends]
    if not all(math.isfinite(v) for p in proj for v in p):
        return none
    (Ua, Va, qa), (Ub, Vb, qb) = proj
    s0, s1 = np.float64(0.0), np.float64(1.0)
    dU, dV = Ub - Ua, Vb - Va
    for p, q in ((-dU, Ua + 0.5), (dU, (width + 0.5) - Ua), (-dV, Va + 0.5), (dV, (height + 0.5) - Va)):
        if p == 0:
            if q < 0:
                return none
        else:
            r = q / p
            if p < 0:
                if r > s1:
                    return none
                s0 = max(s0, r)
            else:
                if r < s0:
                    return none
                s1 = min(s1, r)
    ca = (mix(Ua, Ub, s0), mix(Va, Vb, s0), mix(qa, qb, s0))
    cb = (mix(Ua, Ub, s1), mix(Va, Vb, s1), mix(qa, qb, s1))
    m = max(abs(cb[0] - ca[0]), abs(cb[1] - ca[1]))
    if not m <= 65536.0:
        return none
    n = max(1, int(math.ceil(m)))
    t = np.arange(n + 1, dtype=np.float64) / np.float64(n)
    U, V, q = mix(ca[0], cb[0], t), mix(ca[1], cb[1], t), mix(ca[2], cb[2], t)
    pu, pv = np.floor(U), np.floor(V)
    inside = (pu >= 0) & (pu < width) & (pv >= 0) & (pv < height)
    depth = (1.0 / q[inside]).astype(np.float32)
    return pu[inside].astype(np.int64), pv[inside].astype(np.int64), depth, n + 1


def track_keys(points, colors, size, pose, frames, view, width, height):
    """The key plane (height * width,) uint64 of one track and the number of points submitted."""
    size = int(min(max(int(size), 0), len(points)))
    n = reference_point_count(size) if view.flags & AS_REFERENCE else size
    plane = np.full(width * height, EMPTY, np.uint64)
    pix, keys = point_samples(points, n, view, width, height)
    np.minimum.at(plane, pix, keys)
    if view.flags & FRUSTA:
        for f in range(frames):
            for s, (A, B) in enumerate(SEGMENTS):
                a, b = segment_eye(np.asarray(pose[f]).reshape(16), box_corner(A, view), box_corner(B, view), view)
                x, y, d, _ = segment_samples(a, b, view, width, height)
                order = np.full(len(x), n + 8 * f + s, np.int64)
                np.minimum.at(plane, y * width + x, _keys(d, order))
    return plane, n


def resolve(plane, n, colors, view, width, height):
    """(bgr (height, width, 3) uint8, depth (height, width) float32) of a key plane."""
    bgr = np.empty((width * height, 3), np.uint8)
    bgr[:] = np.array(view.background, np.uint8)
    hit = plane != EMPTY
    order = (plane & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pt = hit & (order < n)
    c = np.asarray(colors, np.uint8).reshape(-1, 3)[order[pt]]
    if view.flags & AS_REFERENCE:
        c = _REF_LUT[c][:, ::-1]           # output B <- stored R, G <- G, R <- stored B
    bgr[pt] = c
    bgr[hit & ~pt] = np.array(view.frustum, np.uint8)
    depth = np.full(width * height, np.inf, np.float32)
    depth[hit] = (plane[hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return bgr.reshape(height, width, 3), depth.reshape(height, width)


def render(points, colors, sizes, pose, frames, view, width, height):
    """points (T, M, 4) f32, colors (T, M, 3) u8, sizes (T,), pose (T, >= frames, 16) f32 or None ->
    (bgr (T, H, W, 3) uint8, depth (T, H, W) float32)."""
    T = len(sizes)
    bgr = np.empty((T, height, width, 3), np.uint8)
    depth = np.empty((T, height, width), np.float32)
    for t in range(T):
        plane, n = track_keys(points[t], colors[t], sizes[t], None if pose is None else pose[t], frames, view, width, height)
        bgr[t], depth[t] = resolve(plane, n, colors[t], view, width, height)
    return bgr, depth


def coverage(points, size, pose, frames, view, width, height):
    """(height, width) int32: how many distinct primitives reach each pixel of one track."""
    size = int(min(max(int(size), 0), len(points)))
    n = reference_point_count(size) if view.flags & AS_REFERENCE else size
    cnt = np.zeros(width * height, np.int32)
    pix, _ = point_samples(points, n, view, width, height)     # a point reaches a pixel at most once
    np.add.at(cnt, pix, 1)
    if view.flags & FRUSTA:
        for f in range(frames):
            for A, B in SEGMENTS:
                a, b = segment_eye(np.asarray(pose[f]).reshape(16), box_corner(A, view), box_corner(B, view), view)
                x, y, _, _ = segment_samples(a, b, view, width, height)
                cnt[np.unique(y * width + x)] += 1
    return cnt.reshape(height, width)
