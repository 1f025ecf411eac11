"""tests/ref_refit.py, the float64 reference of vslam_refit_fundamental, held to itself on the CPU.

delta_ref, the largest entry-wise difference between its two formulations (eigh of A^t A, svd of A) over the comparison inputs
of tests/test_gpu_refit.py, measured 3.6e-12 (at kp_stride 64, n = 9: nine noisy correspondences leave the smallest relative
gap of the set, 1.7e-6).  The device comparison allows 2^-23 |F_ref| + 16 delta_ref per entry: delta_ref is computed from the
reference alone, never from a device output."""
import numpy as np

import ref_refit


def test_the_two_formulations_agree_and_delta_ref_is_what_is_recorded():
    res = ref_refit.comparison_results()
    comparable = 0
    for name, (F, st) in res.items():
        assert not st["skipped"], name
        print(f"{name}: delta {st['delta']:.3e} gap {st['gap']:.3e} comparable {st['comparable']}")
        # every comparison input named by a shape is comparable; only the n = 8 member of the mixed batch may fall below the gap
        assert st["comparable"] or name.startswith("mixed"), name
        comparable += st["comparable"]
        # first order, the null vector of A^t A moves by eps * lambda_1 / (lambda_8 - lambda_9): what the gap bound limits
        assert not st["comparable"] or st["delta"] <= 64 * 2.0 ** -52 / st["gap"], name
        assert np.array_equal(F, st["F64"].astype(np.float32))
    assert comparable >= len(res) - 1
    d = ref_refit.delta_ref()
    print(f"delta_ref = {d:.3e}")
    assert 1e-14 < d < 2e-11, d          # recorded: 3.6e-12


def test_properties_and_skip_rules_of_the_reference():
    xy1, xy2, matches, best, F_in = ref_refit.case(1, 64, 40)
    F, st = ref_refit.refit(xy1, xy2, matches[:40], F_in)
    F64 = F.astype(np.float64)
    assert abs(np.linalg.norm(F64) - 1) <= 2.0 ** -22 and np.linalg.svd(F64, compute_uv=False)[2] <= 2.0 ** -22
    assert (F64 * F_in.reshape(3, 3)).sum() >= 0
    Fn, stn = ref_refit.refit(xy1, xy2, matches[:40], -F_in)
    assert np.array_equal(Fn, -F)                                   # the sign follows F_in
    assert st["stats"][0] == 40 and st["stats"][2] < st["stats"][1]
    # out-of-range indices are not counted
    bad = matches[:40].copy(); bad[3, 0] = 64; bad[7, 1] = -1
    Fb, stb = ref_refit.refit(xy1, xy2, bad, F_in, kp_stride=64)
    keep = np.ones(40, bool); keep[[3, 7]] = False
    Fk, _ = ref_refit.refit(xy1, xy2, matches[:40][keep], F_in)
    assert stb["stats"][0] == 38 and np.array_equal(Fb, Fk)
    for F2, s2 in (ref_refit.refit(xy1, xy2, matches[:7], F_in), ref_refit.refit(xy1, xy2, matches[:40], F_in, winner=-1),
                   ref_refit.refit(xy1, xy2, np.repeat(matches[:1], 12, 0), F_in)):
        assert s2["skipped"] and np.array_equal(F2.view(np.uint32), F_in.reshape(3, 3).view(np.uint32))
        assert np.isnan(s2["stats"][1:]).all()


def test_accuracy_claim_on_the_reference():
    """32 pairs, 64 inliers with N(0, 0.5 px) noise, F_in an un-normalised eight-point fit on 8 of them; RMS true Sampson
    distance on 200 held-out exact correspondences: the refit is better in at least 28 pairs, median ratio at most 0.6."""
    ratios = []
    for p1, p2, h1, h2, F_in in ref_refit.accuracy_pairs():
        ident = np.stack([np.arange(len(p1))] * 2, 1)
        F, st = ref_refit.refit(p1, p2, ident, F_in)
        assert not st["skipped"]
        ratios.append(ref_refit.rms_sampson(F, h1, h2) / ref_refit.rms_sampson(F_in, h1, h2))
    ratios = np.array(ratios)
    print(f"better in {(ratios < 1).sum()} of {len(ratios)}, median ratio {np.median(ratios):.3f}, worst {ratios.max():.3f}")
    assert (ratios < 1).sum() >= 28
    assert np.median(ratios) <= 0.6
