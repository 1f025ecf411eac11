"""Integer restatements of the matcher, of the RANSAC sample sets and of the accept rule, written from the reference sources
(not from oracle/ and not from the kernels), pure numpy / Python.  They hold oracle/vso_match.cpp, oracle/vso_ransac.cpp and
the device to an independent definition, where the bit-exact tests only show that those agree with each other.

  knn2, ratio_pairs   src/Frame.cpp:83-94    BFMatcher(NORM_HAMMING).knnMatch(d1, d2, 2): per query the two train rows of the
                                             smallest Hamming distance, ties to the lower train index; a query survives when
                                             m0.distance < m1.distance * 0.7, which for integer distances 0 .. 256 is
                                             10 * d0 < 7 * d1 (proved exhaustively in tests/test_oracle_match.py)
  lemire_sets         src/RansacFilter.cpp:6-34   std::mt19937 + libstdc++'s uniform_int_distribution for a 32-bit engine
  accept_rule         src/RansacFilter.cpp:44-66  the sequential scan with its float comparison of the sums

Everything here is exact: an output either equals these or it is wrong."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


# ------------------------------------------------------------------------------------------------------------ matcher
def knn2(d1, d2, chunk=128):
    """The two nearest train rows of d2 (n2, 32) for every query row of d1 (n1, 32) by Hamming distance, ordered by
    (distance, train index).  Returns idx0, dist0, idx1, dist1 (int32, length n1); needs n2 >= 2.  Works through the queries
    in chunks so that the n1 x n2 x 32 table of byte distances is never held at once."""
    d1 = np.asarray(d1, np.uint8).reshape(-1, 32)
    d2 = np.asarray(d2, np.uint8).reshape(-1, 32)
    n1, n2 = len(d1), len(d2)
    assert n2 >= 2, "knnMatch(k = 2) is read at [1]: two train rows at least"
    out = [np.zeros(n1, np.int32) for _ in range(4)]
    idx = np.arange(n2, dtype=np.int64)
    for q0 in range(0, n1, chunk):
        a = d1[q0:q0 + chunk]
        D = _POP[np.bitwise_xor(a[:, None, :], d2[None, :, :])].sum(2, dtype=np.int64)        # (chunk, n2), 0 .. 256
        key = D * n2 + idx[None, :]                    # (distance, index) as one integer: unique per row
        i0 = key.argmin(1)
        r = np.arange(len(a))
        k0 = key[r, i0]
        key[r, i0] = np.iinfo(np.int64).max
        i1 = key.argmin(1)
        k1 = key[r, i1]
        out[0][q0:q0 + len(a)] = i0; out[1][q0:q0 + len(a)] = k0 // n2
        out[2][q0:q0 + len(a)] = i1; out[3][q0:q0 + len(a)] = k1 // n2
    return out


def ratio_pairs(d1, d2, chunk=128):
    """src/Frame.cpp:86-94: (query, best train) for every query with 10 * d0 < 7 * d1, in query order; nothing for fewer than
    two train rows (the reference reads m[1] of a one-element result there: undefined, the project emits nothing)."""
    d2 = np.asarray(d2, np.uint8).reshape(-1, 32)
    d1 = np.asarray(d1, np.uint8).reshape(-1, 32)
    if len(d2) < 2 or len(d1) == 0:
        return np.zeros((0, 2), np.int32)
    i0, e0, _, e1 = knn2(d1, d2, chunk)
    keep = 10 * e0.astype(np.int64) < 7 * e1.astype(np.int64)
    return np.stack([np.nonzero(keep)[0], i0[keep]], 1).astype(np.int32)


def hold_match(d1, d2, knn=None, pairs=None):
    """Hold one item's matcher outputs to the definitions above: knn (n1, 4) = idx0, dist0, idx1, dist1 per query and / or the
    surviving pairs (m, 2).  Returns the number of queries held."""
    d1 = np.asarray(d1, np.uint8).reshape(-1, 32)
    d2 = np.asarray(d2, np.uint8).reshape(-1, 32)
    if knn is not None and len(d2) >= 2 and len(d1):
        ref = knn2(d1, d2)
        g = np.asarray(knn).reshape(-1, 4)[:len(d1)]
        for c, name in enumerate(("best index", "best distance", "second index", "second distance")):
            bad = np.nonzero(g[:, c] != ref[c])[0]
            assert bad.size == 0, ("knn2 " + name, bad[:5], g[bad[:5], c], ref[c][bad[:5]])
    if pairs is not None:
        ref = ratio_pairs(d1, d2)
        got = np.asarray(pairs).reshape(-1, 2)
        assert len(got) == len(ref) and np.array_equal(got, ref), ("ratio pairs", len(got), len(ref))
    return len(d1)


# ----------------------------------------------------------------------------------------------------------- RANSAC sets
def lemire_sets(seed, n, H, min_items=8):
    """Independent restatement of initialize_sets (src/RansacFilter.cpp:6-34): numpy's MT19937 seeded by init_genrand is
    std::mt19937(seed); the mapping is libstdc++'s Lemire multiply-shift with rejection for a 32-bit engine.  Every set is 8
    wide and zero-initialised (:17); min_items indices are drawn into it (:22), the rest stay 0."""
    rs = np.random.RandomState(seed & 0xFFFFFFFF)
    out = np.zeros((H, 8), dtype=np.int32)
    if min_items <= 0 or H == 0:
        return out
    assert n >= min_items, "fewer matches than draws: the reference indexes an empty vector"
    buf, pos = [], 0

    def raw():                                            # one raw 32-bit output of the engine
        nonlocal buf, pos
        if pos == len(buf):
            buf = rs.randint(0, 2 ** 32, size=4096, dtype=np.uint64).tolist(); pos = 0
        pos += 1
        return buf[pos - 1]

    for i in range(H):
        moved = {}                                        # available_indices = all_indices (:20), kept as its differences
        for j in range(min_items):
            rng = n - j                                   # distr(0, size - 1), :24
            prod = raw() * rng
            low = prod & 0xFFFFFFFF
            if low < rng:
                thr = (2 ** 32 - rng) % rng
                while low < thr:
                    prod = raw() * rng
                    low = prod & 0xFFFFFFFF
            r = prod >> 32
            out[i, j] = moved.get(r, r)                   # :28
            moved[r] = moved.get(rng - 1, rng - 1)        # :30-31: the last entry takes its place, the vector shrinks
    return out


def hold_sets(seed, n, H, got, min_items=8):
    """Hold one stream of sample sets to lemire_sets."""
    ref = lemire_sets(seed, n, H, min_items)
    got = np.asarray(got).reshape(H, 8)
    bad = np.nonzero((got != ref).any(1))[0]
    assert bad.size == 0, ("ransac sets", int(bad.size), bad[:5], got[bad[:2]], ref[bad[:2]])
    return H


# ----------------------------------------------------------------------------------------------------------- accept rule
def accept_rule(counts, sums):
    """src/RansacFilter.cpp:44-66 as written: best_score = 0 (float), best_nInliers = 0; hypothesis i replaces the best when
    count > best_nInliers, or count == best_nInliers and sum > best_score, the sums compared as floats (NaN > x and x > NaN
    are false).  Returns (winner or -1, best count, best sum as np.float32)."""
    best_n, best_s, winner = 0, np.float32(0.0), -1
    sums = np.asarray(sums, np.float32)
    for i, c in enumerate(np.asarray(counts).tolist()):
        s = sums[i]
        if c > best_n or (c == best_n and bool(s > best_s)):
            best_n, best_s, winner = c, s, i
    return winner, best_n, best_s
