"""extract_features(Frame&, nrows, ncols) (src/Frame.cpp:16-51) on the device vs the oracle: outlined
image, keypoint coordinates and order, angles, octaves and descriptors — all bit-exact.  Every case also holds the device's
outputs to the definitional reference tests/ref_orb.py (keypoint sets per cell and level, coordinates, angles, decided
descriptor bits, count), and the directed cases assert that they land on the boundary they are named for."""
import numpy as np
import pytest
import torch

import ref_orb as R
from orb_cases import count_scene, dots, noise, photos
from vslam_amd import synth

pytestmark = pytest.mark.gpu


def _run(ctx, oracle, bgr, nrows, ncols, cap=16384, pat=None, truncate=False):
    """Device on a batch of frames: bit-exact against the oracle, then held to ref_orb.  Unless truncate, every frame's
    keypoints must fit in cap.  Returns (refs, oracle counts per frame, device outputs)."""
    pat = synth.brief_pattern() if pat is None else pat
    bgr = np.ascontiguousarray(bgr)
    dev = torch.from_numpy(bgr.copy()).cuda()
    out = ctx.extract_features_grid(dev, nrows, ncols, torch.from_numpy(pat).cuda(), cap)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    outlined = dev.cpu().numpy()
    refs, found = [], []
    st = R.new_stats()
    for f in range(bgr.shape[0]):
        ref_img, xy, desc, ao = oracle.extract_features_grid(bgr[f], nrows, ncols, pat)
        assert truncate or len(xy) <= cap, (f, len(xy), cap)
        k = min(len(xy), cap)
        assert np.array_equal(outlined[f], ref_img), f            # cv::rectangle side effect, :32
        assert out["n"][f] == k, (f, out["n"][f], k)
        assert np.array_equal(out["angle_octave"][f, :k].view(np.uint32), ao[:k].view(np.uint32)), f
        assert np.array_equal(out["xy"][f, :k].view(np.uint32), xy[:k].view(np.uint32)), f
        assert np.array_equal(out["desc"][f, :k], desc[:k]), f
        ref = R.grid_reference(bgr[f], nrows, ncols, oracle)
        R.check_grid(ref, out["xy"][f, :k], out["desc"][f, :k], out["angle_octave"][f, :k], oracle, pat,
                     cap=cap if len(xy) > cap else None, stats=st)
        refs.append(ref)
        found.append(len(xy))
    assert st["undecided_cells"] == 0 and st["undecided_levels"] == 0, st
    assert st["undecided_bits"] <= 0.01 * max(st["bits"], 1), st
    return refs, found, out


@pytest.mark.parametrize("w,h,nrows,ncols", [(640, 480, 5, 5), (640, 480, 2, 3), (333, 250, 1, 1), (1280, 720, 5, 5)])
def test_grid_orb_bit_exact(ctx, oracle, w, h, nrows, ncols):
    _, found, _ = _run(ctx, oracle, synth.frames_numpy(70 + w + nrows, 1, w, h), nrows, ncols)
    assert min(found) > 100, "synthetic frame should give ORB keypoints"


def test_grid_orb_long_lists_use_global_scratch(ctx, oracle):
    """One 640x480 cell of pure noise gives FAST lists far longer than the 8191 entries the largest LDS tier of retainBest
    holds, so its replay runs out of the per-slot global scratch."""
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (1, 480, 640, 3), dtype=np.uint8)
    gray = oracle.bgr2gray(bgr[0])
    assert len(oracle.fast9_16(gray, 20)) > 6000
    refs, found, _ = _run(ctx, oracle, bgr, 1, 1, cap=4096)
    assert 400 <= found[0] <= 4096
    assert max(L["n_fast"] for L in refs[0]["cells"][0]["res"]["levels"]) >= 8192


@pytest.mark.parametrize("w,h,level,axis,target", [(320, 74, 1, 1, 62), (320, 76, 1, 1, 63), (320, 77, 1, 1, 64),
                                                   (107, 240, 3, 0, 62), (109, 240, 3, 0, 63), (111, 240, 3, 0, 64)])
def test_grid_orb_unbuilt_level_boundary(ctx, oracle, w, h, level, axis, target):
    """A level whose side is 62 has no inner region (31 <= x < w - 31) and is never built on the device; 63 and 64 are."""
    bgr = np.stack([noise(w + h, w, h), synth.frames_numpy(w * h, 1, w, h)[0]])
    refs, _, _ = _run(ctx, oracle, bgr, 1, 1)
    for ref in refs:
        levels = ref["cells"][0]["levels"]
        assert levels[level].shape[1 - axis] == target == R.level_sizes(w, h)[level][axis]
        assert levels[level - 1].shape[1 - axis] > 62


def test_grid_orb_cell_side_324_level_3_from_the_float_scale(ctx, oracle):
    """src/Frame.cpp passes scaleFactor = 1.2f: level 3 of a 324-px cell is 187 (188 from a double 1.2), and so is every
    coordinate's scale from level 3 on."""
    refs, found, _ = _run(ctx, oracle, synth.frames_numpy(14, 1, 648, 324), 1, 2)
    for ref in refs:
        for c in ref["cells"]:
            assert c["levels"][3].shape == (187, 187) and R.level_sizes(324, 324)[3] == (187, 187)
    assert min(found) > 400


@pytest.mark.parametrize("n", [511, 512, 2047, 2048, 4095, 4096, 8191, 8192])
def test_grid_orb_list_lengths_at_lds_tier_edges(ctx, oracle, n):
    """retainBest keeps its lists in LDS tiers of 512, 2048 and 8192 entries, then global scratch: FAST lists of lengths
    on either side of each edge, all cut (longer than twice level 0's budget of 109)."""
    refs, _, _ = _run(ctx, oracle, dots(n)[None], 1, 1)
    c = refs[0]["cells"][0]
    res = c["res"]
    assert c["decided"] and res["levels"][0]["n_fast"] == n > 2 * R.level_budget()[0]


@pytest.mark.parametrize("target", [499, 500, 501])
def test_grid_orb_fallback_count_boundary(ctx, oracle, target):
    """src/Frame.cpp:34 at the boundary: threshold-20 counts of 499 (falls back to threshold 5), 500 and 501 (kept)."""
    refs, found, _ = _run(ctx, oracle, count_scene(target)[None], 1, 1)
    c = refs[0]["cells"][0]
    assert c["decided"] and c["fallback"] == (target < 500)
    assert R.detect(c["levels"], 20)["count_range"] == (target, target)
    if target >= 500:
        assert found[0] == target


def test_grid_orb_descriptor_discs_leaving_the_level(ctx, oracle):
    """A keypoint of the grid extractor stays >= 30 px inside its frame level, so ORB's own pattern (radius 19) never leaves
    it; the same pattern scaled by 3 (radius 56) does at every level, and orb_desc takes its path with per-sample border
    tests (samples outside the level read the unblurred reflect-101 frame).  1 x 1 grid, keypoints up to octave 7."""
    pat = (synth.brief_pattern().astype(np.int32) * 3).astype(np.int8)
    bgr = np.stack([noise(11, 640, 480), synth.frames_numpy(12, 1, 640, 480)[0]])
    refs, found, out = _run(ctx, oracle, bgr, 1, 1, pat=pat)
    rad = int(np.ceil(np.sqrt((pat.astype(np.int32).reshape(-1, 2) ** 2).sum(1).max()))) + 1
    for f, ref in enumerate(refs):
        xy, oc = out["xy"][f, :found[f]], out["angle_octave"][f, :found[f], 1].astype(int)
        cx = np.floor(xy[:, 0] / R.SCALE ** oc + 0.5); cy = np.floor(xy[:, 1] / R.SCALE ** oc + 0.5)
        lw = np.array([ref["flevels"][l].shape[1] for l in oc]); lh = np.array([ref["flevels"][l].shape[0] for l in oc])
        leaves = (cx - rad < 0) | (cx + rad >= lw) | (cy - rad < 0) | (cy + rad >= lh)
        assert leaves[oc >= 5].sum() > 10 and leaves.sum() > 100, f
        edge = (np.minimum(cx, cy) <= 31) & (oc >= 5)
        assert edge.any(), "keypoints on the border filter's edge at high octaves"


def test_grid_orb_several_frames_stride_below_count(ctx, oracle):
    """Three frames per call with kp_stride below every frame's count: each output is the first kp_stride keypoints."""
    refs, found, out = _run(ctx, oracle, synth.frames_numpy(41, 2, 640, 480)[:3], 2, 2, cap=300,
                             truncate=True)
    assert min(found) > 300 and list(out["n"]) == [300] * 3


def test_grid_orb_c3g_shape(ctx, oracle):
    """1280 x 720 in 4 x 4 cells, the shape of bench.py's C3g workload."""
    _, found, _ = _run(ctx, oracle, synth.frames_numpy(0x5EED0003, 1, 1280, 720), 4, 4)
    assert min(found) > 3000


def test_grid_orb_photographs_against_reference(ctx, oracle):
    _, found, _ = _run(ctx, oracle, np.stack(photos()), 2, 2)
    assert min(found) > 50
