"""The prune certificate with a hypothesis per LANE (ransac_prune.hip "Mapping", ransac_prune_tile.h): phi is the A operand of
v_mfma_f32_32x32x2_f32 and F the B operand, so a lane's sixteen result registers are sixteen matches of its own hypothesis, and
the misses are counted in the lane.  The experiments build keeps the form this replaced -- a hypothesis per tile row, the misses
counted from compare masks on the scalar unit -- behind VSLAM_RANSAC_PRUNE_ROWS, for the prune kernel and for the screen's
head path.  Both compute the same fma chain per (hypothesis, match), so everything is compared bit for bit:
(a) X[h], the certified misses behind the head, of every hypothesis (debug_ransac_prune_x), with the pair-level gate off so that
    every pair is walked -- and with it what the stage returns;
(b) pot0 and the routing word as the screen's head path leaves them (debug_ransac_head), with the head route forced on.
The inputs are the generators of tests/test_gpu_ransac_headstart.py; the row form alone produces every compared value."""
import numpy as np
import pytest

from test_gpu_prune import _env, _evaluate, _same
from test_gpu_ransac import _find
from test_gpu_ransac_headstart import (HEAD, _batch, _identity_pairs, first_exit_inputs, plateau_inputs,  # noqa: F401
                                       uncertified_inputs)

from vslam_amd import synth

pytestmark = pytest.mark.gpu

FORMS = (("lanes", {}), ("rows", {"VSLAM_RANSAC_PRUNE_ROWS": 1}))
HYPS = [31, 33, 128, 130]                     # lanes without a hypothesis: in one wave, one lane into the second, none, two into the next workgroup
# behind a head of 128: one match; exactly one tile; one into the second; the first look (two tiles); one past it; a partial last tile
WALK_SIZES = [129, 160, 161, 192, 193, 257]
HEAD_SIZES = [3, 32, 33, 128, 200]            # n0 = 3, 32, 33, 128 and 128 with matches behind it
THR = 10.0


def walk_inputs(oracle, Hy):
    """WALK_SIZES of the 65 % data of edge_inputs (ransac_inputs.batch) and of first_exit_inputs' exact 55 % data."""
    K = max(WALK_SIZES)
    a1, a2, ap, am = _batch(5300 + Hy, WALK_SIZES, K, 1280, 720)
    B = len(WALK_SIZES)
    b1 = np.zeros((B, K, 2), np.float32); b2 = np.zeros((B, K, 2), np.float32)
    for b in range(B):
        b1[b], b2[b], _ = synth.two_view_points(6100 + b, K, 1280, 720, inlier_frac=0.55, noise_px=0.0, integer=False)
    xy1, xy2 = np.concatenate([a1, b1]), np.concatenate([a2, b2])
    pairs = np.concatenate([ap, _identity_pairs(B, K)])
    m = np.concatenate([am, np.array(WALK_SIZES, np.int32)])
    sets = np.stack([oracle.ransac_sets(31 + b, int(n), Hy) for b, n in enumerate(m)])
    return xy1, xy2, pairs, m, sets, THR


def _both_forms(ctx_exp, B, Hy, run, **env):
    """run() through the experiments build in either form: its outputs, X, and pot0 / the routing word of the head."""
    res = {}
    for form, sw in FORMS:
        with _env(**env, **sw):
            out = run()
            X = ctx_exp.debug_ransac_prune_x(B, Hy)
            pot0, route = ctx_exp.debug_ransac_head(B, Hy)
            ctx_exp.synchronize()
        res[form] = dict(out=out, X=X.cpu().numpy(), pot0=pot0.cpu().numpy(), route=route.cpu().numpy())
    return res


def _assert_identical(res, tag, m):
    lanes, rows = res["lanes"], res["rows"]
    walked = (rows["X"] > 0).sum(axis=1)
    print("%s: X > 0 at %s hypotheses per pair (m = %s), X sums to %d" % (tag, walked.tolist(), np.asarray(m).tolist(), rows["X"].sum()))
    assert np.array_equal(lanes["X"], rows["X"]), (tag, np.argwhere(lanes["X"] != rows["X"])[:4])
    assert np.array_equal(lanes["route"], rows["route"]), tag
    assert np.array_equal(lanes["pot0"], rows["pot0"]), (tag, np.argwhere(lanes["pot0"] != rows["pot0"])[:4])
    _same(lanes["out"], rows["out"], tag)
    assert (rows["X"] > 0).any(), tag       # the walk happened: the comparison is not one of zeros


@pytest.mark.parametrize("Hy", HYPS)
def test_x_at_the_tile_and_look_edges(ctx_exp, oracle, Hy):
    """(a) m = 129 .. 257 behind a head of 128, at hypothesis counts that leave lanes, waves and workgroups partly empty."""
    xy1, xy2, pairs, m, sets, thr = walk_inputs(oracle, Hy)
    res = _both_forms(ctx_exp, len(m), Hy, lambda: _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr), VSLAM_RANSAC_PRUNE_GATE=0)
    _assert_identical(res, "edges, H = %d" % Hy, m)


@pytest.mark.parametrize("name", ["first exit exact", "first exit noisy", "plateau"])
def test_x_where_the_stop_rules_fire(ctx_exp, oracle, name):
    """(a) first_exit_inputs: rows whose hypotheses all die (nobody alive); plateau_inputs: 130 to 150 good hypotheses that
    miss fewer than half of the matches seen (the plateau rule).  The same tiles are walked, so X is the same."""
    inp = {"first exit exact": lambda: first_exit_inputs(oracle, True), "first exit noisy": lambda: first_exit_inputs(oracle, False),
           "plateau": lambda: plateau_inputs(oracle)}[name]()
    xy1, xy2, pairs, m, sets, thr = inp
    Hy = sets.shape[1]
    res = _both_forms(ctx_exp, len(m), Hy, lambda: _find(ctx_exp, oracle, xy1, xy2, pairs, m, sets, thr), VSLAM_RANSAC_PRUNE_GATE=0)
    _assert_identical(res, name, m)


def test_x_with_uncertified_lanes(ctx_exp, oracle):
    """(a) uncertified_inputs: c is +inf in the lanes of the all-NaN hypothesis and wherever the range test fails; such a lane
    counts nothing and is never alive, in either form."""
    xy1, xy2, pairs, m, sets, hypF = uncertified_inputs(oracle)
    Hy = hypF.shape[1]
    res = _both_forms(ctx_exp, len(m), Hy, lambda: _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, THR), VSLAM_RANSAC_PRUNE_GATE=0)
    _assert_identical(res, "uncertified", m)
    nan = np.isnan(hypF).all(axis=2)
    assert nan.any() and (res["lanes"]["X"][nan] == 0).all()


@pytest.mark.parametrize("Hy", HYPS)
def test_head_pot0_and_route(ctx_exp, oracle, Hy):
    """(b) the head route forced on, n0 = 3, 32, 33 and 128 (a partial first tile, exactly one, one row into the second, all
    four), 30 % inliers: pot0 = n0 - X and the routing word of either form.  The hypotheses are those the solver finds on 200
    matches of each pair; scoring a given F has no lower limit on the matches (VSLAM_OPT_RANSAC_MIN_MATCHES = 1)."""
    K, B = max(HEAD_SIZES), len(HEAD_SIZES)
    xy1 = np.zeros((B, K, 2), np.float32); xy2 = np.zeros((B, K, 2), np.float32)
    for b in range(B):
        xy1[b], xy2[b], _ = synth.two_view_points(8300 + b, K, 1280, 720, inlier_frac=0.30)
    pairs = _identity_pairs(B, K)
    full = np.full(B, K, np.int32)
    sets = np.stack([oracle.ransac_sets(710 + b, K, Hy) for b in range(B)])
    hypF = _find(ctx_exp, oracle, xy1, xy2, pairs, full, sets, THR)["hypF"]
    m = np.array(HEAD_SIZES, np.int32)
    ctx_exp.set_option(ctx_exp.OPT_RANSAC_MIN_MATCHES, 1)
    try:
        res = _both_forms(ctx_exp, B, Hy, lambda: _evaluate(ctx_exp, xy1, xy2, pairs, m, hypF, THR), VSLAM_RANSAC_HEAD_ROUTE=1)
    finally:
        ctx_exp.set_option(ctx_exp.OPT_RANSAC_MIN_MATCHES, 8)
    lanes, rows = res["lanes"], res["rows"]
    n0 = np.minimum(m, HEAD)
    print("H = %d: n0 - pot0 sums per pair to %s (n0 = %s)" % (Hy, (n0[:, None] - rows["pot0"]).sum(axis=1).tolist(), n0.tolist()))
    assert (rows["route"] == 1).all() and np.array_equal(lanes["route"], rows["route"])
    assert np.array_equal(lanes["pot0"], rows["pot0"]), np.argwhere(lanes["pot0"] != rows["pot0"])[:4]
    assert np.array_equal(lanes["X"], rows["X"])
    _same(lanes["out"], rows["out"], "head, H = %d" % Hy)
    # the comparison is not one of untouched values: the head certifies misses at every n0, and never more than it holds
    assert ((rows["pot0"] < n0[:, None]).any(axis=1)).all() and (rows["pot0"] >= 0).all()
