"""The pose chain (front end, VSLAM_OPT_POSE_REFIT, extract_Rt, triangulation, VSLAM_OPT_POSE_REFINE, reprojection filter) on
the CPU, put together from the per-stage references -- the oracle's exports, tests/ref_refit.py, tests/ref_refine.py -- in the
order include/vslam_amd.h states for the two options, and the way a device run is held to it.

pairs_pose() runs the chain for one pair entirely on the CPU (every stage fed the stage before it): what the inputs of the GPU
tests are chosen and counted with (tests/test_ref_chain.py).  hold_pairs_pose() compares a device run STAGE BY STAGE WITH
HAND-OFF: each reference stage is fed the device's own output of the stage before it, so no tolerance compounds through the
chain, a bit-exact stage stays bit-exact whatever came before it, and no device stage entry point is called.

Tolerances are the stages' own (tests/test_gpu_refit.py, tests/test_gpu_refine.py); the adjustment does not converge within its
20 iterations on these inputs, so the result is defined by the trajectory -- tests/test_ref_chain.py measures, on the reference
alone, that the trajectory's end moves by less than a sixteenth of the tolerance under reorderings of the matches."""
import hashlib

import numpy as np

import ref_refine as rr
import ref_refit

W, H, MAXC, HYP, THR, PAIRS = 320, 240, 300, 64, 10.0, 3        # the shapes of the option tests (tests/test_gpu_refit.py)
THR_SQ = 4.0                                                    # reproj_threshold_sq of the pose chain
ITERATIONS = 20
KMAT = np.array([[525.0, 0, W // 2], [0, 525.0, H // 2], [0, 0, 1]], np.float32)
C1 = np.c_[KMAT, np.zeros(3, np.float32)]
KD = KMAT.astype(np.float64)
T, FR, KP = 2, 3, 448                                           # the sequence of test_option_through_track_sequences
COMBOS = [(0, 0), (1, 0), (0, 1), (1, 1)]                       # (refit, refine)

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def batch_inputs():
    """frames (2 * PAIRS, H, W, 3): pair b = (frames[b], frames[PAIRS + b]); seeds (PAIRS,) int32."""
    from vslam_amd import synth
    return synth.frames_numpy(900, PAIRS, W, H), np.arange(PAIRS, dtype=np.int32)


def sequence_inputs():
    """bgr (T, FR, H, W, 3); seeds (T, FR - 1) int32: step f of track t is the pair of frames f - 1 and f."""
    from vslam_amd import synth
    return synth.sequences_numpy(2, T, FR, W, H), (np.arange(T * (FR - 1), dtype=np.int32) * 7919 + 5).reshape(T, FR - 1)


# ------------------------------------------------------------------------------------------------ the oracle front end, cached
_FEATURES, _FRONT = {}, {}


def _key(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def features(oracle, bgr):
    from vslam_amd import synth
    k = _key(bgr)
    if k not in _FEATURES:
        ca, sa = synth.keypoint_rotation()
        _FEATURES[k] = oracle.extract_features(bgr, MAXC, ca, sa, synth.brief_pattern())
    return _FEATURES[k]


def front_end(oracle, bgr_a, bgr_b, seed):
    """a, b (the two frames' features), matches (m, 2), F (9,) as match_features returns them, and best (4,) int32 as the device
    reports it: winner, count, bits(sum), m -- from find_fundamental's stages run one by one."""
    seed = int(seed) & 0xFFFFFFFF
    k = (_key(bgr_a), _key(bgr_b), seed)
    if k in _FRONT:
        return _FRONT[k]
    a, b = features(oracle, bgr_a), features(oracle, bgr_b)
    ref = oracle.match_features(a["xy"], a["desc"], b["xy"], b["desc"], seed, HYP, THR)
    best = np.array([-1, 0, 0, len(ref["matches"])], np.int32)
    pairs, rc = oracle.match_knn2_ratio(a["desc"], b["desc"])
    if rc == 0 and len(pairs) >= 8:
        r = oracle.find_fundamental(a["xy"], b["xy"], pairs, oracle.ransac_sets(seed, len(pairs), HYP), THR, want_all=False)
        if r["winner"] >= 0:
            assert np.array_equal(bits(r["F"]), bits(ref["F"])) and int(r["mask"].sum()) == len(ref["matches"])
            best[:3] = r["winner"], r["count"], int(bits(np.float32(r["sum"])).view(np.int32).reshape(-1)[0])
    _FRONT[k] = dict(a=a, b=b, matches=ref["matches"], F=ref["F"], best=best)
    return _FRONT[k]


# ------------------------------------------------------------------------------------------------ the stages
def pre_adjustment(oracle, F, xy1, xy2, matches):
    """R0 (3, 3), t0 (3,), c2_0 (3, 4), X0 (m, 4): the oracle's extract_Rt, camera_matrix and triangulate on the nine words of F."""
    m = np.asarray(matches, np.int32).reshape(-1, 2)
    R0, t0 = oracle.extract_Rt(F, KMAT)
    c2_0 = oracle.camera_matrix(KMAT, R0, t0)
    X0 = oracle.triangulate(xy1[m[:, 0]], xy2[m[:, 1]], C1, c2_0)
    return R0, t0, c2_0, X0


def adjustment(xy1, xy2, matches, R0, t0, X0, thr_sq=THR_SQ):
    """ref_refine.refine as VSLAM_OPT_POSE_REFINE calls it: gate 4 x reproj_threshold_sq, 20 iterations."""
    return rr.refine(xy1, xy2, matches, KMAT, R0, t0, X0, 4.0 * thr_sq, ITERATIONS)


def reprojection_filter(oracle, X, xy1, xy2, matches, c2, thr_sq=THR_SQ):
    m = np.asarray(matches, np.int32).reshape(-1, 2)
    if len(m) == 0:
        return np.zeros(0, np.int32), 0.0
    return oracle.reprojection_filter(X, xy1[m[:, 0]], xy2[m[:, 1]], C1, c2, np.full(len(m), -1, np.int32), thr_sq)


def pairs_pose(oracle, bgr_a, bgr_b, seed, refit=0, refine=0):
    """The whole chain for one pair on the CPU.  Returns a dict of every stage's values (front, F_ransac, F, R0, t0, c2_0, X0, R,
    t, c2, points4d, inlier_idx, error) and the two references' info (refit_info, refine_info; None where the option is off or
    there is no RANSAC winner)."""
    fe = front_end(oracle, bgr_a, bgr_b, seed)
    xy1, xy2, m = fe["a"]["xy"], fe["b"]["xy"], fe["matches"]
    out = dict(front=fe, F_ransac=fe["F"], F=fe["F"], refit_info=None, refine_info=None, winner=int(fe["best"][0]))
    if fe["best"][0] < 0:
        return out
    if refit:
        out["F"], out["refit_info"] = ref_refit.refit(xy1, xy2, m, fe["F"])
        out["F"] = out["F"].reshape(9)
    R0, t0, c2_0, X0 = pre_adjustment(oracle, out["F"], xy1, xy2, m)
    out.update(R0=R0, t0=t0, c2_0=c2_0, X0=X0, R=R0, t=t0, c2=c2_0, points4d=X0)
    if refine:
        out["R"], out["t"], out["c2"], out["points4d"], out["refine_info"] = adjustment(xy1, xy2, m, R0, t0, X0)
    out["inlier_idx"], out["error"] = reprojection_filter(oracle, out["points4d"], xy1, xy2, m, out["c2"])
    return out


def tolerance():
    """The device tolerance of the adjustment, relative to an array's scale (tests/test_gpu_refine.py): 1.7e-6."""
    return 2.0 ** -23 + 16 * rr.delta_ref()


def unrounded(info):
    """(R, t, c2, points (m, 3) with zeros where a match does not participate, part) of a refine() run, before the f32 rounding."""
    X = np.zeros((len(info["part"]), 3))
    X[info["part"]] = info["X64"]
    return info["R64"], info["t64"], rr.camera(KD, info["R64"], info["t64"]), X, info["part"]


def reordered(xy1, xy2, matches, R0, t0, X0, perm):
    """unrounded() of the adjustment run with the matches (and their points) in another order, put back into the given order."""
    inv = np.argsort(perm)
    R, t, c2, X, part = unrounded(adjustment(xy1, xy2, matches[perm], R0, t0, X0[perm])[4])
    return R, t, c2, X[inv], part[inv]


def movement(a, b):
    """Per output array, relative to the array's scale as the device comparison takes it: how far two runs' unrounded() values
    are apart."""
    Ra, ta, ca, Xa, pa = a
    Rb, tb, cb, Xb, pb = b
    assert np.array_equal(pa, pb)
    d = lambda x, y: float(np.abs(x - y).max())
    return dict(R=d(Ra, Rb), t=d(ta, tb), c2=d(ca, cb) / float(np.abs(ca).max()), points=d(Xa, Xb) / float(np.abs(Xa).max()))


# ------------------------------------------------------------------------------------------------ holding a device run
def hold_front_end(fe, xy1, desc1, nodes1, n1, xy2, desc2, nodes2, n2, matches, best, tag):
    """One pair's device front-end outputs (numpy, one pair's rows) against the oracle's bits."""
    for side, f, xy, desc, nodes, n in (("a", fe["a"], xy1, desc1, nodes1, n1), ("b", fe["b"], xy2, desc2, nodes2, n2)):
        assert int(n) == f["n"], (tag, side, "n")
        assert np.array_equal(bits(xy[:f["n"]]), bits(f["xy"])), (tag, side, "xy")
        assert np.array_equal(desc[:f["n"]], f["desc"]), (tag, side, "desc")
        assert np.array_equal(nodes[:f["n"]], f["nodes"]), (tag, side, "nodes")
    m = len(fe["matches"])
    assert np.array_equal(np.asarray(best, np.int32), fe["best"]), (tag, "best", best, fe["best"])
    assert np.array_equal(matches[:m], fe["matches"]), (tag, "matches")


def hold_F(F_dev, fe, refit, tag):
    """d_F against the oracle's bits (REFIT off, or no winner) or against ref_refit.refit of the oracle's F (REFIT on).
    Returns the reference's info, None where nothing was refitted."""
    from test_gpu_refit import hold_F_to_reference
    if not refit or fe["best"][0] < 0:
        assert np.array_equal(bits(F_dev), bits(fe["F"])), (tag, "F")
        return None
    Fr, rs = ref_refit.refit(fe["a"]["xy"], fe["b"]["xy"], fe["matches"], fe["F"], kp_stride=max(MAXC, KP))
    if rs["skipped"]:
        assert np.array_equal(bits(F_dev), bits(fe["F"])), (tag, "F left alone")
        return rs
    hold_F_to_reference(tag, F_dev, (Fr, rs), fe["F"], ref_refit.delta_ref())
    return rs


def hold_adjustment(dev, pre, xy1, xy2, matches, refine, tag, thr_sq=THR_SQ):
    """dev = the device's (R (9,), t (3,), c2 (12,), points4d (>= m, 4)) of one pair, pre = pre_adjustment() of the device's own
    F.  Returns dict(info = the reference's info or None, held = "bits" | "left alone" | "reference" | "properties",
    worst = largest err / tol of a pair held to the reference)."""
    from test_gpu_refine import hold_arrays_to_reference, hold_properties
    R, t, c2, P = dev
    R0, t0, c2_0, X0 = pre
    m = len(matches)

    def same(want_c2, what):
        assert np.array_equal(bits(R), bits(R0).reshape(9)), (tag, what, "R")
        assert np.array_equal(bits(t), bits(t0)), (tag, what, "t")
        assert np.array_equal(bits(c2), bits(want_c2).reshape(12)), (tag, what, "c2")
        assert np.array_equal(bits(P[:m]), bits(X0)), (tag, what, "points4d")
    if not refine:
        same(c2_0, "REFINE off")
        return dict(info=None, held="bits", worst=0.0)
    ref = adjustment(xy1, xy2, matches, R0, t0, X0, thr_sq)
    info = ref[4]
    if info["left_alone"]:
        # the header's rule for an item left alone: R, t and the points keep their bits, and c2 is K [R | t] of them formed in
        # f64 and rounded once (ref[2]) -- on these inputs up to an ulp from c2_0, which extract_Rt forms in f32
        same(ref[2], "left alone")
        print(f"{tag}: left alone ({int(info['stats'][0])} participants), c2 is extract_Rt's bits: "
              f"{np.array_equal(bits(c2), bits(c2_0).reshape(12))}")
        return dict(info=info, held="left alone", worst=0.0)
    n = max(len(xy1), len(xy2))                                  # one stride for both frames, as on the device
    pad = lambda xy: np.concatenate([xy, np.zeros((n - len(xy), 2), np.float32)])
    case = (pad(xy1), pad(xy2), np.asarray(matches, np.int32), np.array([0, m, 0, m], np.int32), None, None, X0)
    front = hold_properties(R, t, c2, P[:m], None, case, tag, KD)
    part = info["part"]
    assert np.isfinite(P[:m]).all(), (tag, "an adjusted pair's points are finite")
    assert (P[:m][part, 3] == 1.0).all(), (tag, "w = 1 in the participating slots")
    if not front[part].all():
        print(f"{tag}: {int((~front[part]).sum())} participating points without positive depth in both cameras as written")
    if info["comparable"]:
        assert front[part].all(), (tag, "every participating point has positive depth in both cameras")
    assert np.array_equal(bits(P[:m][~part]), bits(X0[~part])), (tag, "slots of matches that do not participate keep their bits")
    if not (info["comparable"] and info["margin"] >= rr.DECIDED_MARGIN):
        print(f"{tag}: adjusted, {int(part.sum())} participants, properties only (comparable {info['comparable']}, "
              f"margin {info['margin']:.1e}, singular blocks {info['singular'].tolist()})")
        return dict(info=info, held="properties", worst=0.0)
    worst = hold_arrays_to_reference(tag, (R, t, c2, P[:m]), ref, case, rr.delta_ref(), K=KD)
    print(f"{tag}: adjusted, {int(part.sum())} participants, accepted {int(info['stats'][3])}, last decrease {info['last_rel']:.1e}, "
          f"worst err / tol {worst:.3f}")
    return dict(info=info, held="reference", worst=worst)


def hold_filter(oracle, inlier_idx, n_inliers, error, P, xy1, xy2, matches, c2, tag, thr_sq=THR_SQ):
    kept, err = reprojection_filter(oracle, P[:len(matches)], xy1, xy2, matches, np.asarray(c2, np.float32).reshape(3, 4), thr_sq)
    assert int(n_inliers) == len(kept) and np.array_equal(inlier_idx[:len(kept)], kept), (tag, "inlier_idx")
    assert float(error) == err, (tag, "error", float(error), err)


def hold_pairs_pose(oracle, dev, frames, seeds, refit, refine, untouched=None, tag=""):
    """dev: the outputs of vslam_frontend_pairs_pose (numpy) for frames (2 P, H, W, 3) and seeds (P,).  untouched: the outputs of
    the same call with both options off -- what a pair without a RANSAC winner must still hold.  Returns per pair the
    dict of hold_adjustment with `refit` = the refit reference's info added."""
    P = len(seeds)
    report = []
    for b in range(P):
        tg = f"{tag} pair {b}"
        fe = front_end(oracle, frames[b], frames[P + b], seeds[b])
        hold_front_end(fe, dev["xy"][b], dev["desc"][b], dev["nodes"][b], dev["n"][b], dev["xy"][P + b], dev["desc"][P + b],
                       dev["nodes"][P + b], dev["n"][P + b], dev["matches"][b], dev["best"][b], tg)
        rs = hold_F(dev["F"][b], fe, refit, tg)
        if fe["best"][0] < 0:
            assert untouched is not None, "a pair without a winner needs the options-off outputs"
            for k in ("R", "t", "c2", "points4d", "inlier_idx", "n_inliers", "error"):
                assert np.array_equal(np.ascontiguousarray(dev[k][b]).view(np.uint8),
                                      np.ascontiguousarray(untouched[k][b]).view(np.uint8)), (tg, k, "no winner")
            report.append(dict(info=None, held="no winner", worst=0.0, refit=rs))
            continue
        xy1, xy2, m = fe["a"]["xy"], fe["b"]["xy"], fe["matches"]
        pre = pre_adjustment(oracle, dev["F"][b], xy1, xy2, m)
        r = hold_adjustment((dev["R"][b], dev["t"][b], dev["c2"][b], dev["points4d"][b]), pre, xy1, xy2, m, refine, tg)
        hold_filter(oracle, dev["inlier_idx"][b], dev["n_inliers"][b], dev["error"][b], dev["points4d"][b], xy1, xy2, m,
                    dev["c2"][b], tg)
        r["refit"] = rs
        report.append(r)
    return report
