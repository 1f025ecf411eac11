"""A definitional restatement of the grid ORB/FAST extractor, extract_features(Frame&, nrows, ncols) (src/Frame.cpp:16-51),
written from ORB's published definition (Rublee et al. 2011: oFAST = FAST-9/16 + Harris ranking over a scale pyramid,
intensity-centroid orientation; rBRIEF = BRIEF tests steered by that angle), OpenCV's documented ORB parameters
(ORB::create(500, 1.2f, 8, 31, 0, 2, HARRIS_SCORE, 31, 20 / 5): nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel,
WTA_K, scoreType, patchSize, fastThreshold) and src/Frame.cpp itself -- not from oracle/.  It holds oracle/vso_orb.cpp and the
device to definitions, where the bit-exact tests only show that those two agree with each other.

It follows tests/ref64.py's conventions: each stage takes as input the u8 / f32 values that the stage under test sees (the
pyramid levels are the oracle's, themselves held to float64 bilinear by resize_errors; the angle that steers a descriptor is
the one reported), computes in float64 or exactly in integers, returns every value with the bound it can be trusted to and a
*decided* flag for every outcome that sits on a boundary.  Only decided outcomes are asserted.

  scale             ORB::create takes scaleFactor as a float; src/Frame.cpp passes 1.2f, so scale_l = (float)pow((double)1.2f, l)
                    (not (float)1.2^l: the two differ in the last bit from level 3 on)
  level size        cvRound(cols * (1.f / scale_l)), pinned.  Where cols / 1.2f^l lies within the expression's float error of
                    x.5 (cols / 1.2^l is exactly x.5 there: cols = 3 mod 6 at level 1, 108 * odd at level 3, ...) the
                    rounding is implementation-defined and the size undecided.
  budget            500 (1 - f) / (1 - f^8), f = 1 / 1.2f, geometric, the remainder on the last level; 2x for the FAST pass
  FAST              9 contiguous of the 16 radius-3 circle pixels all darker than v - t or all brighter than v + t; score =
                    the largest t that still holds; strict 3x3 non-max suppression.  Integer-exact: always decided.
  border filter     31 <= x < w - 31 and 31 <= y < h - 31 on each level (a level with w or h <= 62 is emptied)
  retainBest(n)     a set rule: everything whose response is >= the n-th largest, ties at the cut all kept
  Harris            k = 0.04, 7 x 7 block centred on the point, 3 x 3 Sobel, scale 1 / (4 * 7 * 255): a, b, c exact integers;
                    bound C_HARRIS * EPS * (|ab| + c^2 + k (a + b)^2) * scale^4 on the f32 response
  angle             degrees(atan2(m01, m10)) mod 360 from the exact integer moments over the radius-15 disc;
                    bound ATAN_BOUND degrees (fastAtan2 is a polynomial, measured against atan2 in the CPU tests)
  coordinates       x = sx + x_l * 1.2f^l, bound C_XY * EPS * |x|; the octave exact
  fallback          the threshold-5 result when the threshold-20 count (after its ties) is below 500
  descriptor        256 steered tests on the 7 x 7 Gaussian-blurred level (samples outside the level read the unblurred
                    reflect-101 frame, which the in-place blur of the level does not touch) at round(pt / scale_l); a bit is
                    undecided when one of its rotated offsets lies within C_ROT * EPS * (|fx| + |fy|) * (2 + |angle in rad|)
                    of x.5, a row when its centre lies within C_CENTRE * EPS * |c| of x.5.
The constants carry a margin of at least 4x over what the oracle and the device reach (the CPU tests print the ratios).
"""
import math
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -23
NFEATURES, NLEVELS, EDGE, HALF = 500, 8, 31, 15
SCALE = float(np.float32(1.2))      # ORB::create(500, 1.2f, ...): the float scaleFactor, widened
HARRIS_K, HARRIS_BLOCK = 0.04, 7
C_HARRIS = 16.0
C_XY = 8.0
C_ROT = 4.0
C_CENTRE = 8.0
ATAN_BOUND = 0.04      # degrees; fastAtan2's largest error over the reachable moment range is printed by test_fast_atan2_bound

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


# ------------------------------------------------------------------------------------------------ pyramid geometry
def level_size(n, l, scale=SCALE):
    """(pinned, exact, decided): pinned = cvRound(n * (1.f / (float)scale^l)) in f32 with round-half-even; exact = the
    rounded real quotient n / scale^l; decided when that quotient is further from x.5 than the f32 expression's three
    roundings (3 * 2^-24 relative, taken as 4 EPS) can move it."""
    inv = np.float32(1.0) / np.float32(scale ** l)
    pinned = int(np.rint(np.float64(np.float32(np.float32(n) * inv))))
    q = Fraction(n) / Fraction(scale) ** l
    dist = abs(q - (math.floor(q) + Fraction(1, 2)))
    decided = float(dist) > 4 * EPS * float(q)
    exact = math.floor(q + Fraction(1, 2)) if decided else None
    return pinned, exact, decided


def level_sizes(w, h, nlevels=NLEVELS):
    return [(level_size(w, l)[0], level_size(h, l)[0]) for l in range(nlevels)]


def level_budget(nfeatures=NFEATURES, nlevels=NLEVELS):
    f = 1.0 / SCALE
    nd = nfeatures * (1 - f) / (1 - f ** nlevels)
    out = []
    for _ in range(nlevels - 1):
        out.append(int(np.floor(nd + 0.5)))
        nd *= f
    out.append(max(nfeatures - sum(out), 0))
    return out


def bilinear(src, dw, dh):
    """float64 bilinear, source position (d + 0.5) s - 0.5 clamped to the image on each axis."""
    src = np.asarray(src, np.float64)
    sh, sw = src.shape

    def axis(dn, sn):
        p = np.clip((np.arange(dn) + 0.5) * (sn / dn) - 0.5, 0, sn - 1)
        i0 = np.minimum(np.floor(p).astype(np.int64), max(sn - 2, 0))
        fr = p - i0
        return i0, np.minimum(i0 + 1, sn - 1), fr

    y0, y1, fy = axis(dh, sh)
    x0, x1, fx = axis(dw, sw)
    rows = src[y0] * (1 - fy)[:, None] + src[y1] * fy[:, None]
    return rows[:, x0] * (1 - fx) + rows[:, x1] * fx


RESIZE_BOUND = 1.5   # 255/512 per axis for the Q8 coefficients + the final rounding


def resize_errors(levels):
    """max |levels[l] - bilinear(levels[l - 1])| for l >= 1 (0 for a level too small to say anything)."""
    return [float(np.abs(levels[l].astype(np.float64) - bilinear(levels[l - 1], levels[l].shape[1], levels[l].shape[0])).max())
            if levels[l].size and levels[l - 1].size else 0.0 for l in range(1, len(levels))]


# ------------------------------------------------------------------------------------------------------ FAST-9/16
def fast_arc_score(img):
    """best[y, x] = max over the 16 arcs of 9 of min(v - p) or min(p - v) (-1 outside y, x in [3, n - 3))."""
    g = np.asarray(img, np.int16)
    h, w = g.shape
    best = np.full((h, w), -1, np.int16)
    if h < 7 or w < 7:
        return best
    v = g[3:h - 3, 3:w - 3]
    d = np.stack([v - g[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])
    for sgn in (1, -1):
        e = sgn * d
        m2 = np.minimum(e, np.roll(e, -1, axis=0))
        m4 = np.minimum(m2, np.roll(m2, -2, axis=0))
        m8 = np.minimum(m4, np.roll(m4, -4, axis=0))
        m9 = np.minimum(m8, np.roll(e, -8, axis=0))
        best[3:h - 3, 3:w - 3] = np.maximum(best[3:h - 3, 3:w - 3], m9.max(axis=0))
    return best


def fast(img, t, best=None):
    """FAST-9/16 with strict 3x3 NMS: (x, y, score) in raster order, score = best - 1."""
    if best is None:
        best = fast_arc_score(img)
    score = np.where(best > t, best.astype(np.int32) - 1, 0)
    h, w = score.shape
    if h < 3 or w < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = score[1:-1, 1:-1]
    ok = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= c > score[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    ys, xs = np.nonzero(ok)
    return xs + 1, ys + 1, c[ys, xs]


def border_mask(x, y, w, h, border=EDGE):
    if w <= 2 * border or h <= 2 * border:
        return np.zeros(len(x), bool)
    return (x >= border) & (x < w - border) & (y >= border) & (y < h - border)


# ------------------------------------------------------------------------------------------- Harris, retainBest, angle
def harris_abc(img, x, y, block=HARRIS_BLOCK):
    """Exact integer a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the block centred on (x, y), 3x3 Sobel."""
    g = np.asarray(img, np.int64)
    r = block // 2
    offs = np.arange(-r, r + 1)
    yy = y[:, None, None] + offs[None, :, None]
    xx = x[:, None, None] + offs[None, None, :]

    def at(dy, dx):
        return g[yy + dy, xx + dx]

    ix = 2 * (at(0, 1) - at(0, -1)) + (at(-1, 1) - at(-1, -1)) + (at(1, 1) - at(1, -1))
    iy = 2 * (at(1, 0) - at(-1, 0)) + (at(1, -1) - at(-1, -1)) + (at(1, 1) - at(-1, 1))
    return (ix * ix).sum((1, 2)), (iy * iy).sum((1, 2)), (ix * iy).sum((1, 2))


def harris_response(a, b, c, block=HARRIS_BLOCK, k=HARRIS_K):
    """(response, bound) in float64 from exact a, b, c."""
    s4 = (1.0 / (4 * block * 255.0)) ** 4
    a = a.astype(np.float64); b = b.astype(np.float64); c = c.astype(np.float64)
    r = (a * b - c * c - k * (a + b) ** 2) * s4
    return r, C_HARRIS * EPS * (np.abs(a * b) + c * c + k * (a + b) ** 2) * s4


def retain_best(resp, n, bound=None, key=None):
    """retainBest(n) as a set rule.  Returns (keep mask, decided).  Candidates sharing a key (equal exact inputs) get equal
    f32 responses, so they move as one group; with bounds the cut is decided when the group holding the n-th largest
    response is separated, by more than the bounds, from every group above and every group below it."""
    m = len(resp)
    if n < 0 or m <= n:
        return np.ones(m, bool), True
    if n == 0:
        return np.zeros(m, bool), True
    resp = np.asarray(resp, np.float64)
    if bound is None:
        thr = np.sort(resp)[::-1][n - 1]
        return resp >= thr, True
    if key is None:
        key = resp
    ukey, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ng = len(ukey)
    gr = np.zeros(ng); ge = np.zeros(ng); gc = np.zeros(ng, np.int64)
    gr[inv] = resp; np.maximum.at(ge, inv, bound); np.add.at(gc, inv, 1)
    order = np.argsort(-gr, kind="stable")
    cum = np.cumsum(gc[order])
    g = int(np.searchsorted(cum, n))          # first group whose cumulative count reaches n
    keep_g = np.zeros(ng, bool)
    keep_g[order[:g + 1]] = True
    lo = gr[order[g]] - ge[order[g]]
    hi = gr[order[g]] + ge[order[g]]
    above, below = order[:g], order[g + 1:]
    decided = bool((len(above) == 0 or (gr[above] - ge[above]).min() > hi) and
                   (len(below) == 0 or (gr[below] + ge[below]).max() < lo))
    return keep_g[inv], decided


def umax_reference(half=HALF):
    """The centroid disc's half widths: round(sqrt(r^2 - v^2)) below r / sqrt 2, the rest by the disc's symmetry u <-> v
    (umax[v] = the largest u whose own half width reaches v)."""
    vmin = int(np.ceil(half * np.sqrt(2.0) / 2))
    u = [int(np.floor(np.sqrt(half * half - v * v) + 0.5)) for v in range(vmin)]
    for v in range(vmin, half + 1):
        u.append(max(uu for uu in range(len(u)) if u[uu] >= v))
    return np.array(u, np.int64)


def disc_offsets(umax):
    half = len(umax) - 1
    uu, vv = np.meshgrid(np.arange(-half, half + 1), np.arange(-half, half + 1))
    inside = np.abs(uu) <= np.asarray(umax)[np.abs(vv)]
    return uu[inside], vv[inside]


_DISC = disc_offsets(umax_reference())


def ic_moments(img, x, y):
    """Exact integer (m01, m10) over the radius-15 disc centred on (x, y)."""
    g = np.asarray(img, np.int64)
    du, dv = _DISC
    vals = g[y[:, None] + dv[None, :], x[:, None] + du[None, :]]
    return (vals * dv).sum(1), (vals * du).sum(1)


def angle_deg(m01, m10):
    return np.mod(np.degrees(np.arctan2(np.asarray(m01, np.float64), np.asarray(m10, np.float64))), 360.0)


def angle_diff(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


# ---------------------------------------------------------------------------------------------------- ORB::detect
def detect(levels, t, nfeatures=NFEATURES):
    """ORB::detect on one image given its pyramid levels (u8, as the stage sees them).  Returns a list of per-level dicts:
      x, y        level coordinates of the candidates that reach Harris (after the border filter and the first cut)
      keep        the second cut's set on them;  decided  whether that cut is decided
      resp, rb    Harris response and bound;  angle  degrees in [0, 360)
      n_fast      FAST corners inside the border (the list the first cut sees);  n_first  the list the second cut sees
    and count_range (lo, hi) of the final count (lo == hi when every level is decided)."""
    budget = level_budget(nfeatures, len(levels))
    out, lo, hi = [], 0, 0
    for l, img in enumerate(levels):
        h, w = img.shape
        x, y, s = fast(img, t)
        bm = border_mask(x, y, w, h)
        x, y, s = x[bm], y[bm], s[bm]
        n_fast = len(x)
        k1, _ = retain_best(s, 2 * budget[l])
        x, y = x[k1], y[k1]
        a, b, c = harris_abc(img, x, y)
        resp, rb = harris_response(a, b, c)
        key = np.stack([np.minimum(a, b), np.maximum(a, b), c * c], 1)
        keep, dec = retain_best(resp, budget[l], rb, key)
        m01, m10 = ic_moments(img, x, y)
        out.append(dict(level=l, x=x, y=y, keep=keep, decided=dec, resp=resp, rb=rb, angle=angle_deg(m01, m10),
                        n_fast=n_fast, n_first=len(x)))
        kk = int(keep.sum())
        lo += kk if dec else min(kk, budget[l])
        hi += kk if dec else len(x)
    return dict(levels=out, count_range=(lo, hi))


def detect_with_fallback(levels, nfeatures=NFEATURES):
    """src/Frame.cpp:33-36: the threshold-20 result unless it holds fewer than nfeatures, then the threshold-5 result.
    Returns (result, fallback, decided)."""
    r20 = detect(levels, 20, nfeatures)
    lo, hi = r20["count_range"]
    if lo >= nfeatures:
        return r20, False, True
    r5 = detect(levels, 5, nfeatures)
    if hi < nfeatures:
        return r5, True, True
    return (r20, r5), None, False


# --------------------------------------------------------------------------------------------------- outlines, grid
def outline(bgr, nrows, ncols):
    """cv::rectangle(image, Rect(sx, sy, cw, ch), black) for every cell, columns outer and rows inner (:26-32)."""
    img = np.array(bgr, np.uint8, copy=True)
    h, w, _ = img.shape
    cw, ch = w // ncols, h // nrows
    for i in range(ncols):
        for j in range(nrows):
            sx, sy = i * cw, j * ch
            img[sy, sx:sx + cw] = 0
            img[sy + ch - 1, sx:sx + cw] = 0
            img[sy:sy + ch, sx] = 0
            img[sy:sy + ch, sx + cw - 1] = 0
    return img


def grid_reference(bgr, nrows, ncols, oracle):
    """Everything the grid extractor's outputs are held to.  The stages' u8 inputs come from the oracle: the gray
    conversion (held elsewhere) and the pyramids (held to float64 bilinear here, resize_errors)."""
    img = outline(bgr, nrows, ncols)
    h, w, _ = img.shape
    cw, ch = w // ncols, h // nrows
    cells = []
    for i in range(ncols):
        for j in range(nrows):
            sx, sy = i * cw, j * ch
            gray = oracle.bgr2gray(img[sy:sy + ch, sx:sx + cw])
            levels = oracle.orb_pyramid(gray)
            res, fb, dec = detect_with_fallback(levels)
            cells.append(dict(i=i, j=j, sx=sx, sy=sy, levels=levels, res=res, fallback=fb, decided=dec))
    gray = oracle.bgr2gray(img)
    return dict(img=img, w=w, h=h, cw=cw, ch=ch, nrows=nrows, ncols=ncols, cells=cells, gray=gray)


def _frame_levels(ref, oracle, needed):
    if "flevels" not in ref:
        ref["flevels"] = oracle.orb_pyramid(ref["gray"])
        ref["blurred"] = {}
    for l in needed:
        if l not in ref["blurred"]:
            ref["blurred"][l] = oracle.gaussian7(ref["flevels"][l])
    return ref["flevels"], ref["blurred"]


def descriptor_bits(raw, blurred, cx, cy, angle, pattern):
    """Steered BRIEF at integer centres (cx, cy) on one level with the reported angles (degrees, f32).  Returns (bits, decided)
    as (n, 256) bool arrays; bit 8 * byte + k of a row is (1 << k) of byte `byte`."""
    h, w = raw.shape
    pat = np.asarray(pattern, np.float64).reshape(256, 4)
    ar = np.radians(np.asarray(angle, np.float32).astype(np.float64))
    ca, sa = np.cos(ar)[:, None], np.sin(ar)[:, None]
    samples, dec = [], np.ones((len(cx), 256), bool)
    for e in range(2):
        fx, fy = pat[None, :, 2 * e], pat[None, :, 2 * e + 1]
        rx = fx * ca - fy * sa
        ry = fx * sa + fy * ca
        bnd = C_ROT * EPS * (np.abs(fx) + np.abs(fy)) * (2 + np.abs(ar)[:, None])
        for r in (rx, ry):
            dec &= np.abs(np.abs(r - np.floor(r)) - 0.5) > bnd
        px = cx[:, None] + np.floor(rx + 0.5).astype(np.int64)
        py = cy[:, None] + np.floor(ry + 0.5).astype(np.int64)
        inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        qx = np.abs(px); qx = np.where(qx >= w, 2 * w - 2 - qx, qx)
        qy = np.abs(py); qy = np.where(qy >= h, 2 * h - 2 - qy, qy)
        samples.append(np.where(inside, blurred[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)], raw[qy, qx]).astype(np.int32))
    return samples[0] < samples[1], dec


def unpack_desc(desc):
    return np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32), axis=1, bitorder="little").astype(bool)


def new_stats():
    return dict(xy=0.0, angle=0.0, undecided_cells=0, undecided_levels=0, undecided_rows=0, undecided_bits=0, bits=0,
                points=0)


def check_grid(ref, xy, desc, ao, oracle, pattern, cap=None, stats=None):
    """Hold one frame's extract_features_grid outputs (xy, desc, angle/octave, as f32 / u8 arrays of the reported count) to
    grid_reference.  cap: the caller's keypoint capacity (outputs truncated to it).  Asserts; returns stats."""
    st = stats if stats is not None else new_stats()
    xy = np.asarray(xy, np.float32); ao = np.asarray(ao, np.float32)
    n = len(xy)
    oct_ = ao[:, 1].astype(np.int64)
    assert np.array_equal(oct_.astype(np.float32), ao[:, 1]), "octave not an integer"
    cw, ch, nrows, ncols = ref["cw"], ref["ch"], ref["nrows"], ref["ncols"]
    x64, y64 = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    ci = np.clip(np.floor(x64 / cw).astype(np.int64), 0, ncols - 1)
    cj = np.clip(np.floor(y64 / ch).astype(np.int64), 0, nrows - 1)
    cell = ci * nrows + cj
    # ORB::compute regroups by level, stably: levels in order, cells in detection order inside a level
    assert np.all(np.diff(oct_) >= 0), "not grouped by level"
    same = np.diff(oct_) == 0
    assert np.all(np.diff(cell)[same] >= 0), "regrouping by level is not stable"
    sc = SCALE ** oct_
    sx, sy = ci * cw, cj * ch
    xl = np.floor((x64 - sx) / sc + 0.5).astype(np.int64)
    yl = np.floor((y64 - sy) / sc + 0.5).astype(np.int64)
    for v, s0, vl in ((x64, sx, xl), (y64, sy, yl)):
        e = np.abs(v - (s0 + vl * sc))
        r = e / (C_XY * EPS * np.abs(v))
        st["xy"] = max(st["xy"], float(r.max()) if n else 0.0)
        assert np.all(r <= 1), ("coordinate off the level grid", np.nonzero(r > 1)[0][:5])
    # ORB::compute's border filter on the whole frame at level 0
    w, h = ref["w"], ref["h"]
    inb = (x64 >= EDGE) & (x64 < w - EDGE) & (y64 >= EDGE) & (y64 < h - EDGE)
    assert inb.all(), "keypoint outside compute's border"
    total_lo = total_hi = 0
    seen = np.zeros(n, bool)
    for c in ref["cells"]:
        k = c["i"] * nrows + c["j"]
        if not c["decided"]:
            st["undecided_cells"] += 1
            r20, r5 = c["res"]
            opts = [r20, r5]
        else:
            opts = [c["res"]]
        lo = min(o["count_range"][0] for o in opts)
        hi = max(o["count_range"][1] for o in opts)
        total_lo += lo; total_hi += hi
        for l in range(NLEVELS):
            sel = np.nonzero((cell == k) & (oct_ == l))[0]
            seen[sel] = True
            got = set(zip(xl[sel].tolist(), yl[sel].tolist()))
            assert len(got) == len(sel), ("duplicate keypoints", k, l)
            ok = False
            for o in opts:
                L = o["levels"][l]
                cand = dict(((int(a), int(b)), i) for i, (a, b) in enumerate(zip(L["x"], L["y"])))
                if not got <= set(cand):
                    continue
                if L["decided"] and len(opts) == 1 and cap is None:
                    want = set((int(a), int(b)) for a, b in zip(L["x"][L["keep"]], L["y"][L["keep"]]))
                    assert got == want, ("keypoint set", k, l, len(got), len(want), sorted(got ^ want)[:6])
                idx = np.array([cand[p] for p in zip(xl[sel].tolist(), yl[sel].tolist())], np.int64)
                d = angle_diff(ao[sel, 0], L["angle"][idx])
                if d.size:
                    st["angle"] = max(st["angle"], float(d.max()) / ATAN_BOUND)
                assert np.all(d <= ATAN_BOUND), ("angle", k, l, float(d.max()) if d.size else 0)
                assert np.all((ao[sel, 0] >= 0) & (ao[sel, 0] <= 360))
                ok = True
                break
            assert ok, ("keypoints that no definition gives", k, l, len(got))
            if len(opts) == 1 and not opts[0]["levels"][l]["decided"]:
                st["undecided_levels"] += 1
    assert seen.all(), "keypoint outside every cell"
    if cap is None:
        assert total_lo <= n <= total_hi, ("count", n, total_lo, total_hi)
    else:
        assert n == min(cap, n) and (n == cap or total_lo <= n <= total_hi), ("count", n, total_lo, total_hi, cap)
    st["points"] += n
    # descriptors on the whole outlined frame's blurred levels
    levels_used = sorted(set(oct_.tolist()))
    raw, blurred = _frame_levels(ref, oracle, levels_used)
    bits = unpack_desc(desc)
    for l in levels_used:
        sel = np.nonzero(oct_ == l)[0]
        cxf, cyf = x64[sel] / SCALE ** l, y64[sel] / SCALE ** l
        cdec = np.ones(len(sel), bool)
        for cv in (cxf, cyf):
            cdec &= np.abs(np.abs(cv - np.floor(cv)) - 0.5) > C_CENTRE * EPS * np.abs(cv)
        st["undecided_rows"] += int((~cdec).sum())
        sel = sel[cdec]
        cx = np.floor(cxf[cdec] + 0.5).astype(np.int64)
        cy = np.floor(cyf[cdec] + 0.5).astype(np.int64)
        want, dec = descriptor_bits(raw[l], blurred[l], cx, cy, ao[sel, 0], pattern)
        st["bits"] += int(dec.size)
        st["undecided_bits"] += int((~dec).sum())
        bad = dec & (want != bits[sel])
        assert not bad.any(), ("descriptor bits", l, int(bad.sum()), sel[np.nonzero(bad.any(1))[0][:5]])
    return st
