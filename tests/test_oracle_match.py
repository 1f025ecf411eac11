import numpy as np
import pytest

import ref_int
from vslam_amd import synth


def test_ratio_identity_exhaustive():
    """`m0.distance < m1.distance * 0.7` (float vs float*double, src/Frame.cpp:91) equals the
    integer test 10*d0 < 7*d1 for every pair of Hamming distances the kernel can see."""
    for d0 in range(257):
        for d1 in range(d0, 257):
            ref = bool(np.float32(d0) < np.float64(np.float32(d1)) * 0.7)
            assert ref == (10 * d0 < 7 * d1), (d0, d1)


def test_knn2_against_numpy_bruteforce(oracle):
    d1, d2, _ = synth.descriptors_pair(11, 150, 170)
    d2[5] = d2[17]          # force distance ties between train rows
    d2[40] = d2[17]
    i0, e0, i1, e1 = oracle.match_knn2(d1, d2)
    bits1 = np.unpackbits(d1, axis=1).astype(np.int32)
    bits2 = np.unpackbits(d2, axis=1).astype(np.int32)
    D = (bits1[:, None, :] != bits2[None, :, :]).sum(-1)
    order = np.lexsort((np.arange(D.shape[1])[None, :].repeat(D.shape[0], 0), D), axis=1)   # by (dist, idx)
    assert np.array_equal(i0, order[:, 0]) and np.array_equal(i1, order[:, 1])
    assert np.array_equal(e0, D[np.arange(150), order[:, 0]])
    assert np.array_equal(e1, D[np.arange(150), order[:, 1]])


def test_ratio_pairs_are_in_query_order_and_recover_truth(oracle):
    d1, d2, truth = synth.descriptors_pair(3, 400, 420)
    pairs, rc = oracle.match_knn2_ratio(d1, d2)
    assert rc == 0 and len(pairs) > 150
    assert np.all(np.diff(pairs[:, 0]) > 0)
    assert np.mean(truth[pairs[:, 0]] == pairs[:, 1]) > 0.99


def test_degenerate_train_set_is_rejected(oracle):
    d1, d2, _ = synth.descriptors_pair(4, 10, 10)
    _, rc = oracle.match_knn2_ratio(d1, d2[:1])
    assert rc != 0


def _hold(oracle, a, t):
    """oracle match_knn2 / match_knn2_ratio == tests/ref_int.py (bit unpacking never enters: a popcount table in integers)."""
    pairs, rc = oracle.match_knn2_ratio(a, t)
    if len(t) < 2:
        assert rc != 0 or len(pairs) == 0
        assert len(ref_int.ratio_pairs(a, t)) == 0
        return
    knn = np.stack(oracle.match_knn2(a, t), 1) if len(a) else None
    ref_int.hold_match(a, t, knn=knn, pairs=pairs)


@pytest.mark.parametrize("i,n1,n2", [(0, 500, 500), (1, 700, 650), (2, 1, 2), (3, 513, 257), (4, 256, 512), (5, 0, 10), (6, 10, 1),
                                     (7, 10, 0), (8, 3, 2)])
def test_ragged_shapes_against_ref_int(oracle, i, n1, n2):
    """The shapes of test_knn2_and_ratio_bit_exact_ragged_batch, equal train rows included."""
    a, t, _ = synth.descriptors_pair(100 + i, n1, n2)
    if len(t) > 50:
        t[7] = t[33]
    _hold(oracle, a, t)


def test_extreme_distances_against_ref_int(oracle):
    """The inputs of test_extreme_distances_and_index_range: K = 2100, distances 0, 1, 255, 256, all-zero / all-one rows."""
    rng = np.random.default_rng(77)
    K = 2100
    q = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    q[0] = 0; q[1] = 255; q[2] = 0; q[3] = 255
    t = rng.integers(0, 256, (K, 32), dtype=np.uint8)
    t[5] = ~q[10]; t[K - 1] = q[11]; t[K - 2] = q[11]; t[K - 2, 0] ^= 1; t[100] = 255; t[101] = 0
    far = np.stack([~q[12]] * 40)
    far[:, 0] ^= np.arange(40, dtype=np.uint8) % 7
    _hold(oracle, q, t)
    _hold(oracle, q[12:13], far)
    i0, e0, i1, e1 = ref_int.knn2(q, t)
    assert (i0[11], e0[11], i1[11], e1[11]) == (K - 1, 0, K - 2, 1) and e0[10] <= 256
    assert ref_int.knn2(q[10:11], np.stack([t[5], t[5]]))[1::2] == [256, 256]      # the complement: every bit differs
