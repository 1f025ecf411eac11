"""ransac_solve_kernel, path by path: wave tails, every order the closing part can visit the rows in, the private-copy path
beside normal lanes of the same wave, and the out-of-range rotation parameters.  Each case compares hypF with
oracle.find_fundamental(...)["hypF"] bit for bit, as tests/test_gpu_ransac.py does, on hand-made `sets`; what a case is
meant to exercise is asserted on its input, on the CPU, from a float64 restatement of the sweeps."""
import os

import numpy as np
import pytest
import torch

from ransac_inputs import batch as _batch

pytestmark = pytest.mark.gpu

THR = 10.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def design(xy1, xy2, pairs, s):
    """The 8 x 9 design matrices (float32, as the kernel forms them) of the sets s (H, 8) of one item."""
    a, c = xy1[pairs[s, 0]], xy2[pairs[s, 1]]                      # (H, 8, 2)
    u1, v1, u2, v2 = a[..., 0], a[..., 1], c[..., 0], c[..., 1]
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(np.float32)


def first_step(A):
    """p, a, b, g2 of the first (0, 1) pair step of one 8 x 9 matrix, in float64 (p before doubling)."""
    r0, r1 = A[0].astype(np.float64), A[1].astype(np.float64)
    p, a, b = float(r0 @ r1), float(r0 @ r0), float(r1 @ r1)
    return p, a, b, (2 * p) ** 2 + (a - b) ** 2


def sweeps64(A):
    """One-sided Jacobi on the rows of A (H, 8, 9) float32, in OpenCV's pair order: sums, the convergence test and the
    rotation parameters in float64, c, s and the rotated rows in float32 as OpenCV keeps them.  Returns the rows as they
    stand when the sweeps end, before they are sorted."""
    A = A.astype(np.float32)
    eps = 2.0 * float(np.finfo(np.float32).eps)
    for _ in range(30):
        changed = False
        for i in range(7):
            for j in range(i + 1, 8):
                ai, aj = A[:, i].copy(), A[:, j].copy()
                di, dj = ai.astype(np.float64), aj.astype(np.float64)
                p, a, b = (di * dj).sum(1), (di * di).sum(1), (dj * dj).sum(1)
                rot = np.abs(p) > eps * np.sqrt(a * b)
                if not rot.any():
                    continue
                changed = True
                with np.errstate(all="ignore"):
                    p2, beta = 2 * p, a - b
                    gamma = np.sqrt(p2 * p2 + beta * beta)
                    s_neg = np.sqrt((gamma - beta) * 0.5 / gamma).astype(np.float32)
                    c_neg = (p2 / (gamma * s_neg.astype(np.float64) * 2)).astype(np.float32)
                    c_pos = np.sqrt((gamma + beta) / (gamma * 2)).astype(np.float32)
                    s_pos = (p2 / (gamma * c_pos.astype(np.float64) * 2)).astype(np.float32)
                    c = np.where(rot, np.where(beta < 0, c_neg, c_pos), np.float32(1))[:, None]
                    s = np.where(rot, np.where(beta < 0, s_neg, s_pos), np.float32(0))[:, None]
                    A[:, i], A[:, j] = c * ai + s * aj, (-s) * ai + c * aj
        if not changed:
            break
    return A.astype(np.float64)


def row_norms64(xy1, xy2, pairs, s):
    return np.sqrt((sweeps64(design(xy1, xy2, pairs, s)) ** 2).sum(-1))   # (H, 8)


def run(c, xy1, xy2, pairs, m, sets):
    """hypF of the context c for the batch."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = c.ransac_fundamental(t(xy1), t(xy2), t(pairs), t(m), t(sets), THR)
    c.synchronize()
    return out["hypF"].cpu().numpy()


def reference(oracle, xy1, xy2, pairs, m, sets):
    return [oracle.find_fundamental(xy1[b], xy2[b], pairs[b, :n], sets[b], THR)["hypF"] if n >= 8 else None
            for b, n in enumerate(m)]


def same_bits(got, ref, tag):
    for b, r in enumerate(ref):
        if r is None:
            assert not bits(got[b]).any(), f"{tag}: item {b} has fewer than 8 matches and its hypF was written"
            continue
        bad = np.nonzero((bits(got[b]) != bits(r)).any(axis=1))[0]
        assert bad.size == 0, f"{tag}: item {b}: {bad.size} of {r.shape[0]} hypothesis F differ, first {bad[:5]}"


# ---- the cases: inputs and the oracle's answer, made once and shared by the product and the experiments build

TAILS = [1, 63, 64, 65, 129]


def _tails(oracle, H):
    sizes = [40, 8, 5, 23]                                    # an item of exactly 8 matches, and a skipped one
    xy1, xy2, pairs, m = _batch(900 + H, sizes, 48, 1280, 720)
    sets = np.zeros((len(sizes), H, 8), np.int32)
    for b, n in enumerate(sizes):
        if n >= 8:
            sets[b] = oracle.ransac_sets(70 + b, n, H)
    return xy1, xy2, pairs, m, sets


def _orders(oracle):
    """192 random hypotheses whose rows end the sweeps in many different orders.  A rotation leaves the larger norm in the
    row of the lower index, so on matches in general position the sweeps end with the rows sorted and the sort has nothing
    to do.  Rows that never meet in a rotation keep the order they came in: matches on the image's axes (one coordinate
    of each point 0) give sparse design rows, many pairs of them orthogonal from the start.  The 192 are drawn from 4096
    random sets on such matches, round robin over the orders the float64 restatement finds, leaving out sets with a tiny
    row (those take the other path)."""
    K = 600
    rng = np.random.default_rng(1200)
    xy1 = rng.uniform(1, [1280, 720], (1, K, 2)).astype(np.float32)
    xy2 = (xy1 + rng.uniform(-8, 8, (1, K, 2))).clip(1, [1279, 719]).astype(np.float32)
    fam = rng.integers(0, 4, K)
    xy1[0, fam % 2 == 0, 1] = 0                               # (x, 0) or (0, y) in the first frame ...
    xy1[0, fam % 2 == 1, 0] = 0
    xy2[0, fam // 2 == 0, 1] = 0                              # ... and, independently, in the second
    xy2[0, fam // 2 == 1, 0] = 0
    pairs = np.stack([np.arange(K), np.arange(K)], 1).astype(np.int32)[None]
    m = np.array([K], np.int32)
    pool = oracle.ransac_sets(81, K, 4096)
    norms = row_norms64(xy1[0], xy2[0], pairs[0], pool)
    by_order = {}
    for h in np.nonzero(norms.min(1) > 1e-30)[0]:
        by_order.setdefault(tuple(np.argsort(-norms[h], kind="stable")), []).append(h)
    picked, depth = [], 0
    while len(picked) < 192:
        picked += [hs[depth] for hs in by_order.values() if len(hs) > depth][:192 - len(picked)]
        depth += 1
    sets = pool[np.array(picked)][None]
    return xy1, xy2, pairs, m, np.ascontiguousarray(sets)


MIXED_EIGHT, MIXED_TWO = 21, 40                               # lanes of the first wave


def _mixed(oracle):
    xy1, xy2, pairs, m = _batch(1300, [300, 150], 300, 1280, 720)
    sets = np.stack([oracle.ransac_sets(91, 300, 128), oracle.ransac_sets(92, 150, 128)])
    sets[0, MIXED_EIGHT] = sets[0, MIXED_EIGHT, 0]            # one match, eight times
    sets[0, MIXED_TWO, 1] = sets[0, MIXED_TWO, 0]             # the first two matches identical: row 1 is zero after step (0, 1)
    return xy1, xy2, pairs, m, sets


def _range(oracle):
    xy1, xy2, pairs, m = _batch(1400, [200, 120, 64], 200, 1280, 720)
    xy1[1] *= np.float32(2.0 ** 50)                           # products of two coordinates stay below FLT_MAX = 2^128
    xy2[1] *= np.float32(2.0 ** 50)
    sets = np.stack([oracle.ransac_sets(95 + b, int(n), 96) for b, n in enumerate(m)])
    return xy1, xy2, pairs, m, sets


@pytest.fixture(scope="module")
def cases(oracle):
    made = {}

    def get(name):
        if name not in made:
            if name.startswith("tails"):
                inp = _tails(oracle, int(name[5:]))
            else:
                inp = {"orders": _orders, "mixed": _mixed, "range": _range}[name](oracle)
            made[name] = (inp, reference(oracle, *inp))
        return made[name]

    return get


ALL_CASES = ["tails%d" % H for H in TAILS] + ["orders", "mixed", "range"]


# ---- the product build

@pytest.mark.parametrize("H", TAILS)
def test_wave_tails(ctx, oracle, cases, H):
    """Idle lanes of the last wave redo the last hypothesis and store nothing; an item below 8 matches is left alone.
    ransac_fundamental hands the stage a zero-filled hypF and takes no buffer of the caller's, so "left alone" is checked
    as "still all zero bits": a kernel that wrote zeros there would pass."""
    inp, ref = cases("tails%d" % H)
    assert list(inp[3]) == [40, 8, 5, 23] and ref[2] is None
    same_bits(run(ctx, *inp), ref, f"H={H}")


def test_row_orders(ctx, oracle, cases):
    """The closing part visits the rows in the order of their norms.  The input must make it take many orders."""
    inp, ref = cases("orders")
    xy1, xy2, pairs, m, sets = inp
    norms = row_norms64(xy1[0], xy2[0], pairs[0], sets[0])
    assert norms.min() > 1e-30, "a tiny row here would send a wave down the other path"
    perms = {tuple(np.argsort(-w, kind="stable")) for w in norms}
    print(f"row orders: {len(perms)} distinct sort permutations among {len(norms)} hypotheses")
    assert len(perms) >= 20, len(perms)
    same_bits(run(ctx, *inp), ref, "orders")


def test_mixed_waves(ctx, oracle, cases):
    """Two degenerate hypotheses inside a wave of normal ones: their zero rows send the whole wave through the private
    copy, and every neighbour still gets the bits it would have got on the usual path."""
    inp, ref = cases("mixed")
    xy1, xy2, pairs, m, sets = inp
    norms = row_norms64(xy1[0], xy2[0], pairs[0], sets[0][:64])
    tiny = np.nonzero(norms.min(1) <= float(np.finfo(np.float32).tiny))[0]
    assert list(tiny) == [MIXED_EIGHT, MIXED_TWO], tiny         # those two and no neighbour
    same_bits(run(ctx, *inp), ref, "mixed")


def test_out_of_range_operands(ctx, oracle, cases):
    """g2 of a rotation beyond 2^400: the wave leaves the short sqrt / division sequences for jacobi_cs_full."""
    inp, ref = cases("range")
    xy1, xy2, pairs, m, sets = inp
    p, a, b, g2 = first_step(design(xy1[1], xy2[1], pairs[1], sets[1][:1])[0])
    eps = 2.0 * float(np.finfo(np.float32).eps)
    assert abs(p) > eps * np.sqrt(a * b), "hypothesis 0 does not rotate in its first step"
    assert not (2.0 ** -400 < g2 < 2.0 ** 400), g2
    pn, an, bn, g2n = first_step(design(xy1[0], xy2[0], pairs[0], sets[0][:1])[0])
    assert 2.0 ** -400 < g2n < 2.0 ** 400                        # and the item beside it stays inside
    same_bits(run(ctx, *inp), ref, "range")


# ---- the experiments build's split form (sweeps + null-space row in one kernel, the rank-2 step in ransac_close_kernel)

@pytest.fixture(scope="module", params=[4, 5])
def ctx_split(request):
    from vslam_amd import Context, capi
    if not os.path.exists(capi.EXP_LIB_PATH):
        pytest.skip("the experiments build is not there")
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    os.environ["VSLAM_RANSAC_SOLVE_SPLIT"] = str(request.param)   # read when the context is made
    try:
        c = Context(0, lib=capi.load_library(capi.EXP_LIB_PATH))
    finally:
        del os.environ["VSLAM_RANSAC_SOLVE_SPLIT"]
    yield c
    c.close()


@pytest.mark.parametrize("name", ALL_CASES)
def test_split_form_same_bits(ctx_split, oracle, cases, name):
    inp, ref = cases(name)
    same_bits(run(ctx_split, *inp), ref, "split " + name)
