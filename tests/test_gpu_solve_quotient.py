"""jacobi_pair_9's first rotation parameter as one quotient for both signs of beta (ransac_solve.hip):
sqrt(((gamma + |beta|) * 0.5) / gamma) where the kernel selected between ((gamma - beta) * 0.5) / gamma and
(gamma + beta) / (gamma * 2).  An identity on the operations performed, so no bit of hypF may move: the product, the
experiments build and the experiments build with the selected form switched back in (VSLAM_RANSAC_SOLVE_QUOTIENT=two) are
held to oracle.find_fundamental(...)["hypF"] as uint32, at 64 and 65 hypotheses (one full wave; one wave and a tail), on
sets made so that the first rotation of every lane has the sign the case names.  What a case is meant to exercise is
asserted on its input, on the CPU.  The identity itself is checked on 10^6 random (gamma, beta) in float64, on the CPU."""
import numpy as np
import pytest

from ransac_inputs import batch as _batch
from test_gpu_prune import _env
from test_gpu_solve_paths import design, reference, run, same_bits

ITEMS = ["negative", "positive", "mixed", "zero", "vote", "degenerate"]
K = 200
VOTE_LANE, EIGHT_LANE, TWO_LANE = 5, 21, 40
EPS = 2.0 * float(np.finfo(np.float32).eps)


def first_steps(xy1, xy2, pairs, s):
    """p (doubled, as the kernel has it when it forms g2), beta = a - b, g2 and `rotates` of the first (0, 1) step of every set."""
    A = design(xy1, xy2, pairs, s).astype(np.float64)
    p, a, b = (A[:, 0] * A[:, 1]).sum(1), (A[:, 0] ** 2).sum(1), (A[:, 1] ** 2).sum(1)
    with np.errstate(over="ignore"):
        return 2 * p, a - b, (2 * p) ** 2 + (a - b) ** 2, np.abs(p) > EPS * np.sqrt(a * b)


def _order(xy1, xy2, pairs, s, negative):
    """The sets with their first two matches ordered so that beta < 0 where `negative` (per lane), beta > 0 elsewhere."""
    _, beta, _, _ = first_steps(xy1, xy2, pairs, s)
    s = s.copy()
    swap = (beta < 0) != negative
    s[swap, 0], s[swap, 1] = s[swap, 1].copy(), s[swap, 0].copy()
    return s


def _inputs(oracle, H):
    xy1, xy2, pairs, m = _batch(1500 + H, [K] * len(ITEMS), K, 1280, 720)      # all K points matched: pairs is i <-> i
    assert all(np.array_equal(pairs[b, :, 0], np.arange(K)) for b in range(len(ITEMS)))
    sets = np.stack([oracle.ransac_sets(60 + b, K, H) for b in range(len(ITEMS))]).astype(np.int32)
    lanes = np.arange(H)
    for b, neg in ((0, np.ones(H, bool)), (1, np.zeros(H, bool)), (2, lanes % 2 == 0)):
        sets[b] = _order(xy1[b], xy2[b], pairs[b], sets[b], neg)
    # zero: small integer coordinates (every sum below is exact in float64), point 2 k + 1 = point 2 k with x and y swapped
    # in both frames: its design row holds the same nine numbers in another order, so the two rows' norms are equal
    z = ITEMS.index("zero")
    rng = np.random.default_rng(1600 + H)
    for xy in (xy1, xy2):
        xy[z, 0::2] = rng.integers(1, 700, (K // 2, 2)).astype(np.float32)
        xy[z, 1::2] = xy[z, 0::2, ::-1]
    k = rng.integers(0, K // 2, H)
    sets[z, :, 0], sets[z, :, 1] = 2 * k, 2 * k + 1
    for h in range(H):                      # the other six: distinct points, none of the pair's
        rest = np.setdiff1d(np.arange(K), [2 * k[h], 2 * k[h] + 1])
        sets[z, h, 2:] = rng.permutation(rest)[:6]
    # vote: points 0 .. 7 scaled by 2^50 (products of two coordinates stay below FLT_MAX), used by one lane alone
    v = ITEMS.index("vote")
    xy1[v, :8] *= np.float32(2.0 ** 50)
    xy2[v, :8] *= np.float32(2.0 ** 50)
    sets[v] = oracle.ransac_sets(77, K - 8, H) + 8
    sets[v, VOTE_LANE] = np.arange(8)
    # degenerate: one match eight times; the first two matches identical
    d = ITEMS.index("degenerate")
    sets[d, EIGHT_LANE] = sets[d, EIGHT_LANE, 0]
    sets[d, TWO_LANE, 1] = sets[d, TWO_LANE, 0]
    return xy1, xy2, pairs, m, np.ascontiguousarray(sets)


@pytest.fixture(scope="module")
def cases(oracle):
    made = {}

    def get(H):
        if H not in made:
            inp = _inputs(oracle, H)
            made[H] = (inp, reference(oracle, *inp))
        return made[H]
    return get


@pytest.mark.parametrize("H", [64, 65])
def test_cases_are_what_they_say(cases, H):
    """CPU: the signs of beta, beta = 0 exactly, the one lane out of range, all in the first step and all rotating."""
    (xy1, xy2, pairs, m, sets), ref = cases(H)
    step = {name: first_steps(xy1[b], xy2[b], pairs[b], sets[b]) for b, name in enumerate(ITEMS)}
    inside = lambda g2: (g2 > 2.0 ** -400) & (g2 < 2.0 ** 400)
    for name in ("negative", "positive", "mixed", "zero"):
        p, beta, g2, rot = step[name]
        assert rot.all() and inside(g2).all() and (np.abs(p) > 2.0 ** -300).all(), name
    assert (step["negative"][1] < 0).all() and (step["positive"][1] > 0).all()
    assert ((step["mixed"][1] < 0) == (np.arange(H) % 2 == 0)).all() and (step["mixed"][1] != 0).all()
    assert (step["zero"][1] == 0).all()
    A = design(xy1[3], xy2[3], pairs[3], sets[3])
    assert not (A[:, 0] == A[:, 1]).all(1).any(), "zero: the two rows must differ, only their norms are equal"
    p, beta, g2, rot = step["vote"]
    out = ~inside(g2)
    assert rot[VOTE_LANE] and list(np.nonzero(out)[0]) == [VOTE_LANE], np.nonzero(out)[0]
    p, beta, g2, rot = step["degenerate"]
    assert beta[EIGHT_LANE] == 0 and beta[TWO_LANE] == 0 and rot[TWO_LANE]
    assert all(r is not None and r.shape == (H, 9) for r in ref)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [64, 65])
def test_product_same_bits(ctx, cases, H):
    inp, ref = cases(H)
    same_bits(run(ctx, *inp), ref, f"product H={H}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["one", "two"])
@pytest.mark.parametrize("H", [64, 65])
def test_experiments_build_same_bits(ctx_exp, cases, H, form):
    """The experiments build's kernel, and the earlier form of the quotient in it: the same bits as the oracle, so as each other."""
    inp, ref = cases(H)
    with _env(**({"VSLAM_RANSAC_SOLVE_QUOTIENT": "two"} if form == "two" else {})):
        got = run(ctx_exp, *inp)
    same_bits(got, ref, f"experiments, {form} H={H}")


def test_quotient_identity_float64():
    """CPU, numpy float64 (IEEE operations, as the kernel's): for gamma = sqrt(p^2 + beta^2) with g2 in (2^-400, 2^400) the
    selected quotient and the one expression have the same bits, for both signs of beta, for beta = +-0 and for |beta| = gamma
    to the last bit."""
    rng = np.random.default_rng(12)
    n = 1_000_000
    mant = lambda: rng.uniform(1.0, 2.0, n)
    e = rng.integers(-150, 150, n)
    beta = np.ldexp(mant(), e) * rng.choice([-1.0, 1.0], n)
    p = np.ldexp(mant(), e + rng.integers(-60, 60, n))       # from far below beta (gamma = |beta|) to far above
    beta[:1000] = rng.choice([0.0, -0.0], 1000)
    g2 = p * p + beta * beta
    keep = (g2 > 2.0 ** -400) & (g2 < 2.0 ** 400) & (np.abs(p) > 2.0 ** -300)
    assert keep.sum() > 0.95 * n
    gamma, beta = np.sqrt(g2[keep]), beta[keep]
    two = np.where(beta < 0, ((gamma - beta) * 0.5) / gamma, (gamma + beta) / (gamma * 2))
    one = ((gamma + np.abs(beta)) * 0.5) / gamma
    assert (beta < 0).sum() > 0.4 * n and (beta > 0).sum() > 0.4 * n and (beta == 0).sum() >= 900
    assert (gamma == np.abs(beta)).sum() > 1000
    assert np.array_equal(one.view(np.uint64), two.view(np.uint64))
    assert ((one >= 0.5) & (one <= 1.0)).all()
