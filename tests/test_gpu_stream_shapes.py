"""Shape edge cases of the streaming kernels (corner response + candidates, 7x7 blur) and of the staged
descriptor kernel, against the oracle, bit for bit.

The streaming kernels split a frame into 256-pixel column strips and row segments; the cases below put
frame borders on, next to and between strip / segment seams, and include the smallest frames the
vectorised path accepts.  The descriptor cases cover a rotation whose sample offsets need the widest
staged patch and a pattern whose offsets exceed it (direct sampling)."""
import numpy as np
import pytest
import torch

from vslam_amd import synth

pytestmark = pytest.mark.gpu

# (w, h): w % 4 == 0 takes the streaming path
SHAPES = [(4, 4), (8, 5), (12, 135), (252, 40), (256, 91), (260, 136), (264, 181), (512, 33), (516, 271), (1028, 64)]


def textured(w, h, seed, n=2):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    # blocks give real corners and plateaus on top of the noise
    for f in range(n):
        for _ in range(max(1, w * h // 600)):
            x, y = rng.integers(0, w), rng.integers(0, h)
            g[f, y:y + rng.integers(2, 9), x:x + rng.integers(2, 9)] = rng.integers(0, 256)
    return g


@pytest.mark.parametrize("w,h", SHAPES)
def test_blur_and_corners_on_seams(ctx, oracle, w, h):
    gray = textured(w, h, 1000 + w + h)
    t = torch.from_numpy(gray).cuda()
    blur = ctx.gaussian7(t).cpu().numpy()
    maxc = 300
    xy, n = ctx.good_features(t, maxc)
    ctx.synchronize()
    xy, n = xy.cpu().numpy(), n.cpu().numpy()
    for f in range(gray.shape[0]):
        assert np.array_equal(blur[f], oracle.gaussian7(gray[f])), (w, h, f)
        ref = oracle.good_features(gray[f], maxc)
        assert n[f] == len(ref), (w, h, f, n[f], len(ref))
        assert np.array_equal(xy[f, :n[f]], ref), (w, h, f)


def test_corners_on_strip_seam_columns(ctx, oracle):
    """Isolated bright dots placed exactly on the first / last column of a strip (x = 255, 256, 511, 512) and
    next to them: those candidates are emitted unverified by the detector and completed by the selection."""
    w, h = 772, 96
    rng = np.random.default_rng(7)
    gray = rng.integers(100, 110, (2, h, w), dtype=np.uint8)
    for f in range(2):
        for y in range(6, h - 6, 9):
            for x in (254, 255, 256, 257, 510, 511, 512, 513, 767, 768, 769):
                if rng.random() < 0.7:
                    gray[f, y + (x % 3), x] = rng.integers(180, 256)
    t = torch.from_numpy(gray).cuda()
    for maxc in (50, 2000):
        xy, n = ctx.good_features(t, maxc, min_distance=1.0)
        xy, n = xy.cpu().numpy(), n.cpu().numpy()
        for f in range(2):
            ref = oracle.good_features(gray[f], maxc, min_dist=1.0)
            assert n[f] == len(ref), (maxc, f, n[f], len(ref))
            assert np.array_equal(xy[f, :n[f]], ref), (maxc, f)


@pytest.mark.parametrize("angle_deg,scale,table", [(45.0, 1.15, "orb"), (-133.0, 1.0, "orb"), (0.0, 1.0, "synthetic"),
                                                   (0.0, 1.9, "orb"), (10.0, 1.7, "synthetic"), (45.0, 1.15, "synthetic")])
def test_describe_other_rotations_and_wide_patterns(ctx, oracle, angle_deg, scale, table):
    """45 degrees stretches a +-15 pattern to +-21 (the widest staged patch); patterns scaled to +-25 exceed the
    staged patch and are sampled from the image directly (still inside the 31-pixel keypoint border)."""
    w, h = 320, 240
    gray = textured(w, h, 99)
    blur = ctx.gaussian7(torch.from_numpy(gray).cuda())
    base = synth.brief_pattern() if table == "orb" else synth.synthetic_pattern()
    pat = np.clip(np.rint(base.astype(np.float32) * scale), -29, 29).astype(np.int8)
    ca, sa = synth.keypoint_rotation(angle_deg)
    rng = np.random.default_rng(3)
    K = 700
    pts = np.rint(np.stack([rng.uniform(0, w - 1, (2, K)), rng.uniform(0, h - 1, (2, K))], -1)).astype(np.float32)
    n = np.array([K, 77], np.int32)
    xy_out, desc, n_out = ctx.orb_describe(blur, torch.from_numpy(pts).cuda(), torch.from_numpy(n).cuda(), ca, sa,
                                           torch.from_numpy(pat).cuda())
    xy_out, desc, n_out, blur = xy_out.cpu().numpy(), desc.cpu().numpy(), n_out.cpu().numpy(), blur.cpu().numpy()
    for f in range(2):
        rd, keep = oracle.orb_describe(blur[f], pts[f, :n[f]], ca, sa, pat)
        assert n_out[f] == len(keep), f
        assert np.array_equal(desc[f, :len(keep)], rd), f


# The detector's first kernel is cvtColor as well for widths that are a multiple of 4 (response.hip: the BGR form of
# min_eigen_tiered_kernel): strips that end inside / at / beyond the image, one-strip and many-strip widths, heights of one
# and several row segments (a segment's first rows convert rows of the segment above again), padded rows, and rows whose
# padding breaks the alignment (unaligned 12-byte loads in the same kernel).
BGR_SHAPES = [(64, 64, 0), (252, 140, 0), (256, 91, 0), (260, 136, 4), (264, 181, 0), (516, 271, 8), (772, 96, 0), (1028, 70, 0),
              (1924, 75, 0), (260, 136, 2), (516, 100, 1),
              # widths that are no multiple of 4: gray / blurred planes with padded rows (mirrored tail), the last column in
              # every position of a lane's four pixels, in the first lane of a strip of its own (257, 1281) and in the last (255)
              (65, 64, 0), (253, 140, 0), (254, 91, 0), (255, 70, 0), (257, 136, 0), (258, 100, 3), (259, 181, 0), (515, 271, 0),
              (1277, 96, 0), (1278, 75, 1), (1279, 70, 0), (1281, 70, 0)]


@pytest.mark.parametrize("w,h,pad", BGR_SHAPES)
def test_extract_from_bgr_on_seams(ctx, oracle, w, h, pad):
    rng = np.random.default_rng(4000 + w + h + pad)
    n = 3
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    for f in range(n):
        for _ in range(max(1, w * h // 500)):
            x, y = rng.integers(0, w), rng.integers(0, h)
            bgr[f, y:y + rng.integers(2, 12), x:x + rng.integers(2, 12)] = rng.integers(0, 256, 3)
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    maxc = 400
    if pad:
        rows = np.zeros((n, h, 3 * w + pad), dtype=np.uint8)
        rows[:, :, :3 * w] = bgr.reshape(n, h, 3 * w)
        rows[:, :, 3 * w:] = rng.integers(0, 256, (n, h, pad), dtype=np.uint8)   # the padding is not to be looked at
        out = ctx.extract_features(torch.from_numpy(rows).cuda(), maxc, ca, sa, torch.from_numpy(pat).cuda(), width=w)
    else:
        out = ctx.extract_features(torch.from_numpy(bgr).cuda(), maxc, ca, sa, torch.from_numpy(pat).cuda())
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for f in range(n):
        r = oracle.extract_features(bgr[f], maxc, ca, sa, pat)
        assert out["n_detected"][f] == r["n_detected"], (w, h, pad, f)
        k = r["n"]
        assert out["n"][f] == k, (w, h, pad, f)
        assert np.array_equal(out["xy"][f, :k], r["xy"]), (w, h, pad, f)
        assert np.array_equal(out["desc"][f, :k], r["desc"]), (w, h, pad, f)
        assert np.array_equal(out["nodes"][f, :k], r["nodes"]), (w, h, pad, f)


def test_stage_entries_after_a_padded_extract(ctx, oracle):
    """extract_features at a width that gets padded internal rows (67), then the stage entry points on the same context with
    the caller's packed rows, at that width and at a multiple of 4: each stage reads rows of exactly `width` bytes."""
    h, maxc = 96, 150
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    bgr = synth.frames_numpy(4100, 1, 67, h)
    out = ctx.extract_features(torch.from_numpy(bgr).cuda(), maxc, ca, sa, torch.from_numpy(pat).cuda())
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for f in range(bgr.shape[0]):
        r = oracle.extract_features(bgr[f], maxc, ca, sa, pat)
        assert out["n"][f] == r["n"] and np.array_equal(out["desc"][f, :r["n"]], r["desc"]), f
    rng = np.random.default_rng(4101)
    for w in (67, 68):
        gray = textured(w, h, 4102 + w)
        t = torch.from_numpy(gray).cuda()
        eig = ctx.min_eigen(t)
        blur = ctx.gaussian7(t)
        xy, n = ctx.good_features(t, maxc)
        K = 60   # keypoints on both sides of the 31-pixel border
        pts = np.rint(np.stack([rng.uniform(20, w - 21, (2, K)), rng.uniform(20, h - 21, (2, K))], -1)).astype(np.float32)
        pts[:, :2] = [[31, 31], [w - 32, h - 32]]
        xy_out, desc, n_out = ctx.orb_describe(blur, torch.from_numpy(pts).cuda(), torch.full((2,), K, dtype=torch.int32).cuda(),
                                               ca, sa, torch.from_numpy(pat).cuda())
        ctx.synchronize()
        eig, blur, xy, n = eig.cpu().numpy(), blur.cpu().numpy(), xy.cpu().numpy(), n.cpu().numpy()
        desc, n_out = desc.cpu().numpy(), n_out.cpu().numpy()
        for f in range(2):
            assert np.array_equal(eig[f].view(np.uint32), oracle.min_eigen(gray[f]).view(np.uint32)), (w, f)
            assert np.array_equal(blur[f], oracle.gaussian7(gray[f])), (w, f)
            ref = oracle.good_features(gray[f], maxc)
            assert n[f] == len(ref) and np.array_equal(xy[f, :n[f]], ref), (w, f)
            rd, keep = oracle.orb_describe(blur[f], pts[f], ca, sa, pat)
            assert 0 < len(keep) < K and n_out[f] == len(keep) and np.array_equal(desc[f, :len(keep)], rd), (w, f)


@pytest.mark.parametrize("w,h", [(509, 77), (510, 77), (511, 77), (1277, 96), (257, 64), (258, 70), (259, 64), (512, 77)])
def test_detected_corners_before_the_border_filter(ctx_exp, oracle, w, h):
    """The corners goodFeaturesToTrack returns, in rank order, BEFORE ORB::compute drops the ones within 31 pixels of the border
    (vslam_debug_detect, experiments build): what extract_features' own outputs cannot show -- corners in the first and last
    columns' neighbourhood, where the padded rows of an odd width (mirrored tail, a lane across the last column) and the strip
    seams live.  Budget above the corner count (nothing is truncated away), and below it (rank order matters); twice over, the
    second time on workspaces the first left dirty; one frame whose strongest response lies ON the last column."""
    rng = np.random.default_rng(77 + w + h)
    bgr = rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8)
    for f in range(3):
        for _ in range(max(1, w * h // 500)):
            x, y = rng.integers(0, w), rng.integers(0, h)
            bgr[f, y:y + rng.integers(2, 12), x:x + rng.integers(2, 12)] = rng.integers(0, 256, 3)
    bgr[3] = 100                                                     # a flat frame with one small pattern in its last three columns
    patch = np.array([[255, 0, 0], [0, 0, 255], [255, 255, 0], [0, 0, 0], [255, 0, 0], [0, 255, 255]], np.uint8)
    bgr[3, h // 2 - 3:h // 2 + 3, w - 3:] = patch[:, :, None]
    e3 = oracle.min_eigen(oracle.bgr2gray(bgr[3]))
    assert np.unravel_index(np.argmax(e3), e3.shape)[1] == w - 1, "the frame's strongest response should lie on the last column"
    t = torch.from_numpy(bgr).cuda()
    gray = [oracle.bgr2gray(bgr[f]) for f in range(4)]
    for maxc in (4000, 150):
        for rep in range(2):
            xy, n = ctx_exp.debug_detect(t, maxc)
            ctx_exp.synchronize()
            xy, n = xy.cpu().numpy(), n.cpu().numpy()
            for f in range(4):
                ref = oracle.good_features(gray[f], maxc)
                assert n[f] == len(ref), (w, h, maxc, rep, f, n[f], len(ref))
                assert np.array_equal(xy[f, :n[f]], ref), (w, h, maxc, rep, f)
    assert len(oracle.good_features(gray[3], 4000)) > 0
