"""HIP k-d tree vs the oracle: node arrays and radius hit lists, bit-exact and in order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _points(seed, n, w, h, integer=True):
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1)
    return (np.rint(p) if integer else p).astype(np.float32)


def test_build_bit_exact_with_ties(ctx, oracle):
    K = 2100
    cases = [_points(1, 2000, 1280, 720), _points(2, 2100, 100, 100), _points(3, 1, 10, 10), _points(4, 2, 10, 10),
             _points(5, 3, 10, 10), _points(6, 777, 1280, 720, integer=False), np.zeros((0, 2), np.float32),
             np.full((300, 2), 5.0, np.float32), _points(7, 1500, 8, 2000)]
    xy = np.zeros((len(cases), K, 2), np.float32); n = np.zeros(len(cases), np.int32)
    for b, c in enumerate(cases):
        xy[b, :len(c)] = c; n[b] = len(c)
    nodes = ctx.kdtree_build(torch.from_numpy(xy).cuda(), torch.from_numpy(n).cuda()).cpu().numpy()
    for b, c in enumerate(cases):
        ref = oracle.kdtree_build_frame(c)
        assert np.array_equal(nodes[b, :len(c)], ref), f"case {b}"


def test_radius_search_order_and_counts(ctx, oracle):
    K, Q = 2000, 300
    cases = [(_points(11, 2000, 1280, 720), 2.0), (_points(12, 1800, 100, 100), 2.0), (_points(13, 900, 300, 300), 7.5),
             (_points(14, 5, 50, 50), 60.0)]
    B = len(cases)
    xy = np.zeros((B, K, 2), np.float32); n = np.zeros(B, np.int32)
    qs = np.zeros((B, Q, 2), np.float32); nq = np.full(B, Q, np.int32)
    for b, (c, r) in enumerate(cases):
        xy[b, :len(c)] = c; n[b] = len(c)
        rng = np.random.default_rng(50 + b)
        base = c[rng.integers(0, len(c), Q)] + rng.uniform(-2.5, 2.5, size=(Q, 2))
        qs[b] = base.astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    nodes = ctx.kdtree_build(t(xy), t(n))
    for r in sorted({c[1] for c in cases}):
        hits, counts = ctx.kdtree_radius(nodes, t(xy), t(n), t(qs), t(nq), r, hit_cap=64)
        hits, counts = hits.cpu().numpy(), counts.cpu().numpy()
        for b, (c, rr) in enumerate(cases):
            if rr != r:
                continue
            ref_nodes = oracle.kdtree_build_frame(c)
            for q in range(Q):
                ref, cnt = oracle.kdtree_radius_frame(ref_nodes, c, qs[b, q], r, cap=64)
                assert counts[b, q] == cnt, (b, q)
                assert np.array_equal(hits[b, q, :min(cnt, 64)], ref), (b, q)


def test_radius_property_full_size(ctx):
    """4000 points, 4000 queries: the hit SET equals brute force (d^2 < r^2 with the |split| <= r
    pruning never losing a point) — the reference test's own acceptance rule (test_kdtree.cpp:119-129)."""
    K = 4000
    c = _points(21, K, 1920, 1080)
    xy = torch.from_numpy(c[None]).cuda(); n = torch.tensor([K], dtype=torch.int32).cuda()
    nodes = ctx.kdtree_build(xy, n)
    assert sorted(nodes[0].cpu().tolist()) == list(range(K))      # a permutation of the points
    rng = np.random.default_rng(22)
    qs = (c + rng.uniform(-3, 3, size=c.shape)).astype(np.float32)
    hits, counts = ctx.kdtree_radius(nodes, xy, n, torch.from_numpy(qs[None]).cuda(), n, 4.0, hit_cap=32)
    hits, counts = hits[0].cpu().numpy(), counts[0].cpu().numpy()
    d2 = ((qs[:, None, 0] - c[None, :, 0]) ** 2 + (qs[:, None, 1] - c[None, :, 1]) ** 2)
    for q in range(0, K, 7):
        want = set(np.nonzero(d2[q] < np.float32(16.0))[0].tolist())
        assert counts[q] == len(want) and set(hits[q, :counts[q]].tolist()) == want


def _native_exe(tmp_path, name):
    import os
    import subprocess
    from vslam_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build.build_host()
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tests", "native", name + ".cpp"),
                    "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "vslam_amd"), "-lvslam_host", "-lvslam_amd",
                    "-Wl,-rpath," + os.path.join(root, "vslam_amd")], check=True)
    return exe


def test_reference_test_procedure_on_the_device(tmp_path):
    """/root/reference/tests/test_kdtree.cpp:148-151 — the reference's only test — against the product:
    construct_kdtree(KDTree&) / nearest / radius_search of include/vslam/KDTree.h (C++ drop-in -> C ABI -> HIP),
    same unseeded glibc rand() stream, 2 x 1000 trials of 2500-2999 points, the reference's acceptance rules.
    The reference prints '1000 successes out of 1000 trials' twice."""
    import subprocess
    exe = _native_exe(tmp_path, "kdtree_ref_procedure")
    out = subprocess.run([exe, "1000"], check=True, capture_output=True, text=True, timeout=900).stdout.split()
    nn_ok, rad_ok, trials = map(int, out)
    assert (nn_ok, rad_ok, trials) == (1000, 1000, 1000)


def test_nearest_batch_matches_oracle(ctx, oracle):
    """kdtree_nearest_kernel vs the oracle's nearest(KDTree) on 4 trees x 600 queries: ties (integer grids),
    off-grid points, a query on top of a point, and the max_distance_sq cut-off whose 'nothing found' answer is the
    default-constructed {0,0} in the reference (src/KDTree.cpp:38-42; index -1 at the C ABI)."""
    import ctypes as C
    K, Q = 3000, 600
    cases = [_points(31, 2999, 100, 100), _points(32, 2500, 1280, 720), _points(33, 1700, 640, 480, integer=False),
             _points(34, 3, 20, 20), np.full((50, 2), 7.0, np.float32)]
    B = len(cases)
    xy = np.zeros((B, K, 2), np.float32); n = np.zeros(B, np.int32)
    qs = np.zeros((B, Q, 2), np.float32); nq = np.full(B, Q, np.int32)
    for b, c in enumerate(cases):
        xy[b, :len(c)] = c; n[b] = len(c)
        rng = np.random.default_rng(70 + b)
        lo, hi = c.min(0) - 5, c.max(0) + 5
        q = rng.uniform(lo, hi, size=(Q, 2))
        q[: Q // 3] = np.rint(q[: Q // 3])                       # integer queries: exact distance ties
        q[Q // 3: Q // 3 + 20] = c[rng.integers(0, len(c), 20)]     # on top of a point
        qs[b] = q.astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    nodes = ctx.kdtree_build(t(xy), t(n))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for max_d2 in (float("inf"), 30.0, 0.75, 0.0):
        best = ctx.kdtree_nearest(nodes, t(xy), t(n), t(qs), t(nq), max_d2).cpu().numpy()
        n_none = 0
        for b, c in enumerate(cases):
            tree = np.zeros((len(c), 2), np.float32)
            assert oracle.lib.vso_kdtree_build_points(fp(c), len(c), fp(tree)) == 0
            for q in range(Q):
                want = np.zeros(2, np.float32)
                oracle.lib.vso_kdtree_nearest_points(fp(tree), len(c), C.c_float(qs[b, q, 0]), C.c_float(qs[b, q, 1]),
                                                     C.c_float(max_d2), fp(want))
                i = best[b, q]
                got = c[i] if i >= 0 else np.zeros(2, np.float32)
                assert np.array_equal(got, want), (max_d2, b, q, i)
                if i >= 0:
                    d = c[i] - qs[b, q]
                    assert np.float32(d[0] * d[0]) + np.float32(d[1] * d[1]) < np.float32(max_d2)
                n_none += i < 0
        if max_d2 == 0.0:
            assert n_none == B * Q          # strict '<' against 0 never holds
        if max_d2 == 0.75:
            assert 0 < n_none < B * Q


@pytest.mark.parametrize("all_sums", [False, True])
def test_trees_of_the_batched_front_end_for_every_fork_point(ctx, oracle, all_sums):
    """VSLAM_OPT_TREE_FORK moves the k-d build (an output nobody reads) to another point of the matching stages; point 4
    lies in a branch that VSLAM_OPT_RANSAC_ALL_SUMS does not take, where the build used to be dropped silently (advisor,
    round 4).  Every fork point, both scoring modes, pairs and sequence form: the trees are the oracle's."""
    from vslam_amd import synth
    w, h, maxc, hyp = 320, 240, 300, 64
    bgr_np = synth.frames_numpy(4242, 3, w, h)
    bgr = torch.from_numpy(bgr_np).cuda()
    pat = synth.brief_pattern()
    ca, sa = synth.keypoint_rotation()
    seeds = torch.arange(3, dtype=torch.int32).cuda()
    ref = [oracle.extract_features(f, maxc, ca, sa, pat) for f in bgr_np]
    ctx.set_option(ctx.OPT_RANSAC_ALL_SUMS, all_sums)
    try:
        for fork in (-1, 0, 1, 2, 3, 4, 5):
            ctx.set_option(ctx.OPT_TREE_FORK, fork)
            for form in ("pairs", "sequence"):
                if form == "pairs":
                    out = ctx.frontend_pairs(bgr, 3, maxc, ca, sa, None, seeds, hyp, 10.0)
                else:
                    out = ctx.frontend_sequence(bgr, maxc, ca, sa, None, torch.arange(5, dtype=torch.int32).cuda(), hyp, 10.0)
                ctx.synchronize()
                nodes, n = out["nodes"].cpu().numpy(), out["n"].cpu().numpy()
                for f, r in enumerate(ref):
                    assert n[f] == r["n"] and np.array_equal(nodes[f, :r["n"]], r["nodes"]), (fork, form, f)
    finally:
        ctx.set_option(ctx.OPT_TREE_FORK, -1)
        ctx.set_option(ctx.OPT_RANSAC_ALL_SUMS, False)


# ------------------------------------------------------------------------------ the selection code only the device compiles
# wave_partition / wave_nth_element (introselect.h, under __HIPCC__) and the lane-per-subtree path below 48 points, on the
# orders the host check of the serial half uses -- and on sequences that take the depth-limit fallback of a MEDIAN selection
# (tests/kd_cases.py; tests/test_kd_cases.py proves on the CPU that they do).
import kd_cases


@pytest.fixture(scope="module")
def planted(oracle):
    """{n: [(order name, xy [n, 2], the oracle's tree)]}: the oracle's selection is the platform's std::nth_element -- the
    definition -- and every one of its trees passes the checker that does not use it.  Computed once, never written to."""
    out = {}
    for n in kd_cases.ORDER_SIZES:
        out[n] = []
        for name, xy in kd_cases.planted_orders(n):
            ref = oracle.kdtree_build_frame(xy)
            assert kd_cases.check_tree(ref, xy) is None, (n, name)
            ref.setflags(write=False)
            out[n].append((name, xy, ref))
    return out


def _build_and_hold(ctx, trees, stride, tag):
    """trees: [(name, xy, ref)] as one batch of that stride -> every tree equals the oracle's and is a k-d tree."""
    B = len(trees)
    xy = np.zeros((B, stride, 2), np.float32); n = np.zeros(B, np.int32)
    for b, (_, c, _) in enumerate(trees):
        xy[b, :len(c)] = c; n[b] = len(c)
    nodes = ctx.kdtree_build(torch.from_numpy(xy).cuda(), torch.from_numpy(n).cuda()).cpu().numpy()
    for b, (name, c, ref) in enumerate(trees):
        assert kd_cases.check_tree(nodes[b, :len(c)], c) is None, (tag, len(c), name, b, kd_cases.check_tree(nodes[b, :len(c)], c))
        assert np.array_equal(nodes[b, :len(c)], ref), (tag, len(c), name, b)
        assert (nodes[b, len(c):] == -1).all(), (tag, len(c), name, b)      # slots past n are not written


@pytest.mark.parametrize("shape", ["1024-threads", "256-threads"])
def test_build_planted_orders_both_workgroup_shapes(ctx, planted, shape):
    """7 orders x 12 sizes.  A batch of up to 32 trees gets the 1024-thread kernel, a larger one the 256-thread kernel (the
    launcher's rule); the same trees must come out of both.  Each tree is built with kp_stride == n -- the partition's 16-bit
    stopper lists filled to their last slot when every key is equal -- and with kp_stride > n."""
    every = [t for n in kd_cases.ORDER_SIZES for t in planted[n]]
    assert len(every) == 84
    if shape == "1024-threads":
        for n in kd_cases.ORDER_SIZES:
            _build_and_hold(ctx, planted[n], n, "stride == n")                     # 7 trees
        for i in range(0, len(every), 28):
            _build_and_hold(ctx, every[i:i + 28], 2100, "stride > n")
    else:
        for n in kd_cases.ORDER_SIZES:
            _build_and_hold(ctx, planted[n] * 5, n, "stride == n")                 # 35 trees
        _build_and_hold(ctx, every, 2100, "stride > n")                            # 84 trees


def test_build_at_the_largest_stride_and_refusal_one_above(ctx, oracle):
    """kp_stride = n = VSLAM_KDTREE_MAX_KP (include/vslam_amd.h; tests/test_kd_cases.py restates the launcher's rule): random
    integer pixels and the adversary's order.  One slot more is VSLAM_ERR_CAPACITY and d_nodes is not touched."""
    from vslam_amd import capi
    k = kd_cases.KDTREE_MAX_KP
    adv = np.stack([kd_cases.adversary(k), np.random.default_rng(41).integers(0, 720, k)], 1).astype(np.float32)
    trees = []
    for name, c in (("pixels", _points(40, k, 1280, 720)), ("adversary", adv)):
        ref = oracle.kdtree_build_frame(c)
        assert kd_cases.check_tree(ref, c) is None, name
        trees.append((name, c, ref))
    _build_and_hold(ctx, trees, k, "stride == limit")
    xy = torch.zeros((1, k + 1, 2), dtype=torch.float32).cuda()
    xy[0, :k] = torch.from_numpy(trees[0][1]).cuda()
    n = torch.tensor([k + 1], dtype=torch.int32).cuda()
    nodes = torch.full((1, k + 1), -77, dtype=torch.int32).cuda()
    rc = ctx.lib.vslam_kdtree_build(ctx.handle, capi._ptr(xy), capi._ptr(n), 1, k + 1, capi._ptr(nodes))
    ctx.synchronize()
    assert capi.ERRORS.get(rc) == "VSLAM_ERR_CAPACITY"
    assert (nodes == -77).all()


# ------------------------------------------------------------------------------ queries on the deepest trees the ABI takes
DEEP_N = (16384, 16383, 8193)
DEEP_Q = 300


@pytest.fixture(scope="module")
def deep(oracle):
    """9 trees of kp_stride = VSLAM_MAX_KP = 16384 (height 15, len = 0x4000 in a stack entry), which the build cannot make and
    the query kernels take: the oracle's nodes.  Random integer pixels, a 100 x 100 lattice (coincident points, distance ties),
    all points equal; 300 queries per tree, on and off the points."""
    K = kd_cases.VSLAM_MAX_KP
    assert K == 16384
    sets = []
    for j, n in enumerate(DEEP_N):
        sets += [("pixels", _points(300 + j, n, 1280, 720)), ("lattice", _points(310 + j, n, 100, 100)),
                 ("equal", np.full((n, 2), 33.0, np.float32))]
    B = len(sets)
    xy = np.zeros((B, K, 2), np.float32); n = np.zeros(B, np.int32); nodes = np.full((B, K), -1, np.int32)
    qs = np.zeros((B, DEEP_Q, 2), np.float32)
    for b, (name, c) in enumerate(sets):
        xy[b, :len(c)] = c; n[b] = len(c)
        nodes[b, :len(c)] = oracle.kdtree_build_frame(c)
        rng = np.random.default_rng(330 + b)
        q = c[rng.integers(0, len(c), DEEP_Q)] + rng.uniform(-3, 3, (DEEP_Q, 2))
        q[:100] = np.rint(q[:100])                                  # integer queries: on lattice points, exact distance ties
        q[100:140] = c[rng.integers(0, len(c), 40)]                 # on top of a point
        q[140:150] += 40.0                                          # some far from everything of the small sets
        qs[b] = q.astype(np.float32)
    for a in (xy, n, nodes, qs):
        a.setflags(write=False)
    return sets, xy, n, nodes, qs


def _d2(q, c):
    """float32, the kernels' expression: dx * dx + dy * dy, each operation rounded once."""
    dx, dy = q[:, None, 0] - c[None, :, 0], q[:, None, 1] - c[None, :, 1]
    return dx * dx + dy * dy


def test_radius_on_the_deepest_trees(ctx, oracle, deep):
    sets, xy, n, nodes, qs = deep
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    nq = torch.full((len(sets),), DEEP_Q, dtype=torch.int32).cuda()
    for r in (2.0, 7.5):
        hits, counts = ctx.kdtree_radius(t(nodes), t(xy), t(n), t(qs), nq, r, hit_cap=64)
        hits, counts = hits.cpu().numpy(), counts.cpu().numpy()
        for b, (name, c) in enumerate(sets):
            inside = _d2(qs[b], c) < np.float32(r) * np.float32(r)
            assert np.array_equal(counts[b], inside.sum(1)), (r, b, name)
            for q in range(DEEP_Q):
                ref, cnt = oracle.kdtree_radius_frame(nodes[b, :len(c)], c, qs[b, q], r, cap=64)
                assert counts[b, q] == cnt, (r, b, name, q)
                assert np.array_equal(hits[b, q, :min(cnt, 64)], ref), (r, b, name, q)
                if cnt <= 64:
                    assert set(hits[b, q, :cnt].tolist()) == set(np.flatnonzero(inside[q]).tolist()), (r, b, name, q)
                assert (hits[b, q, min(cnt, 64):] == -1).all(), (r, b, name, q)
            if name == "equal":     # a query inside r walks the whole tree: n hits, the first 64 are the pre-order prefix
                near = inside[:, 0]
                assert 40 <= near.sum() < DEEP_Q                       # the 40 queries on top of a point at least
                assert (counts[b][near] == len(c)).all() and (counts[b][~near] == 0).all(), (r, b)
                assert (hits[b][near] == nodes[b, :64][None]).all(), (r, b)


def test_nearest_on_the_deepest_trees(ctx, oracle, deep):
    import ctypes as C
    sets, xy, n, nodes, qs = deep
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    nq = torch.full((len(sets),), DEEP_Q, dtype=torch.int32).cuda()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    trees = []
    for name, c in sets:
        tree = np.zeros((len(c), 2), np.float32)
        assert oracle.lib.vso_kdtree_build_points(fp(np.ascontiguousarray(c)), len(c), fp(tree)) == 0
        trees.append(tree)
    for max_d2 in (float("inf"), 0.75, 0.0):
        best = ctx.kdtree_nearest(t(nodes), t(xy), t(n), t(qs), nq, max_d2).cpu().numpy()
        n_none = 0
        for b, (name, c) in enumerate(sets):
            dmin = _d2(qs[b], c).min(1)
            for q in range(DEEP_Q):
                want = np.zeros(2, np.float32)
                oracle.lib.vso_kdtree_nearest_points(fp(trees[b]), len(c), C.c_float(qs[b, q, 0]), C.c_float(qs[b, q, 1]),
                                                     C.c_float(max_d2), fp(want))
                i = best[b, q]
                assert -1 <= i < len(c), (max_d2, b, name, q, i)
                got = c[i] if i >= 0 else np.zeros(2, np.float32)
                assert np.array_equal(got, want), (max_d2, b, name, q, i)
                if i >= 0:
                    d = c[i] - qs[b, q]
                    mine = np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])
                    assert mine == dmin[q] and mine < np.float32(max_d2), (max_d2, b, name, q, i)
                else:
                    assert not dmin[q] < np.float32(max_d2), (max_d2, b, name, q)
                n_none += i < 0
        if max_d2 == float("inf"):
            assert n_none == 0
        if max_d2 == 0.0:
            assert n_none == len(sets) * DEEP_Q          # strict '<' against 0 never holds
        if max_d2 == 0.75:
            assert 0 < n_none < len(sets) * DEEP_Q


def test_cell_table_on_the_deepest_trees(ctx, deep):
    """vslam_kdtree_cell_table at kp_stride = 16384, slots = 32768: every point owns exactly one slot, the slot's key is the
    point's pixel cell, its value the point's pre-order position, and a probe from the documented start finds it."""
    from vslam_amd import capi
    sets, xy, n, nodes, qs = deep
    B, K, slots = len(sets), xy.shape[1], 32768
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    table = torch.zeros((B, slots, 2), dtype=torch.int32).cuda()
    ok = torch.zeros((B,), dtype=torch.int32).cuda()
    d_nodes, d_xy, d_n = t(nodes), t(xy), t(n)
    ctx._check(ctx.lib.vslam_kdtree_cell_table(ctx.handle, capi._ptr(d_nodes), capi._ptr(d_xy), capi._ptr(d_n), B, K, slots,
                                               capi._ptr(table), capi._ptr(ok)))
    ctx.synchronize()
    table = table.cpu().numpy().view(np.uint32)
    assert (ok.cpu().numpy() != 0).all()
    for b, (name, c) in enumerate(sets):
        used = np.flatnonzero(table[b, :, 0] != 0xFFFFFFFF)
        assert len(used) == len(c), (b, name)
        assert (table[b, table[b, :, 0] == 0xFFFFFFFF, 1] == 0xFFFFFFFF).all(), (b, name)
        rank = table[b, used, 1].astype(np.int64)
        assert np.array_equal(np.sort(rank), np.arange(len(c))), (b, name)            # every pre-order position once
        p = c[nodes[b, rank]]
        key = ((np.floor(p[:, 1]).astype(np.int64) + 32768) << 16) | (np.floor(p[:, 0]).astype(np.int64) + 32768)
        assert np.array_equal(table[b, used, 0].astype(np.int64), key), (b, name)
        # open addressing, linear: no empty slot between a key's start and where it lies
        start = ((key * 2654435761) & 0xFFFFFFFF) >> 7 & (slots - 1)
        dist = (used - start) & (slots - 1)
        empty = np.concatenate([[0], np.cumsum(table[b, :, 0] == 0xFFFFFFFF)])
        wrapped = start + dist >= slots
        between = np.where(wrapped, empty[slots] - empty[start] + empty[(start + dist) & (slots - 1)], empty[np.minimum(start + dist, slots)] - empty[start])
        assert (between == 0).all(), (b, name)
