"""The hand cases of include/vslam_tracks.h that tests/test_ref_tracks.py (the reference), tests/test_tracks_serial.py (the host walk) and
tests/test_gpu_tracks.py (the device) share, and the serial program's file format.

hand_item(): one item whose numbers are exact in binary.  K = [[512, 0, 256], [0, 512, 192], [0, 0, 1]]: Kinv = [[2^-9, 0, -0.5], [0, 2^-9,
-0.375], [0, 0, 1]] without rounding, and the pixel (256, 192) is the ray (0, 0, 1) of its camera.  Cameras (Y = R X + T):
  0  R = I, centre (0, 0, 0)         2  R = I, centre (1, 0, 0)        3, 4, 5  R = I, centres (0.5, 0, 0), (1.5, 0, 0), (2, 0, 0)
  1  rows (0, 0, 1), (0, 1, 0), (-1, 0, 0), centre (3, 0, 2): T = -R c = (-2, 0, 3); its pixel (256, 192) is the ray (-1, 0, 0), which
     meets camera 0's ray (0, 0, 1) at (0, 0, 2) at a right angle.
For "meet": A = (I - e3 e3^t) + (I - e1 e1^t) = diag(1, 2, 1), r = 0 + diag(0, 1, 1) (3, 0, 2) = (0, 0, 2), X0 = (0, 0, 2); both
residuals are 0 there, so g = 0, every candidate equals X, no step is accepted (0 < 0 is false) and the result is (0, 0, 2) exactly,
with cos_parallax 0, cost_out 0 and two good observations.  Its input row (5, 5, 5) lies behind camera 1 (Y_z = -5 + 3): cost_in = +inf.
The point (1, 0.25, 4) projects into a camera with R = I and centre (s, 0, 0) at (128 (1 - s) + 256, 224)."""
import os
import struct
import subprocess

import numpy as np

import ref_tracks as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND_K = np.array([[512, 0, 256], [0, 512, 192], [0, 0, 1]], np.float32)
NAMES = ("meet", "meet_nan_input", "parallel", "one_usable", "same_ray", "behind", "five", "five_truth_input", "empty_row", "past_n")
FIVE_TRUTH = (1.0, 0.25, 4.0)


def hand_item():
    Cs, Kp = 6, 12
    R = np.tile(np.eye(3).reshape(9), (Cs, 1))
    T = np.zeros((Cs, 3))
    R[1] = [0, 0, 1, 0, 1, 0, -1, 0, 0]
    T[1] = [-2, 0, 3]
    for c, s in ((2, 1.0), (3, 0.5), (4, 1.5), (5, 2.0)):
        T[c] = [-s, 0, 0]
    xy = np.full((Cs, Kp, 2), 1000.0, np.float32)
    nxt = [0] * Cs
    rows, pts = [], []

    def obs(cam, where):
        k = nxt[cam]
        nxt[cam] += 1
        xy[cam, k] = where
        return cam, k

    def point(P, entries):
        pts.append(list(P) + [7.0])
        rows.append(entries)
    nan3 = (np.nan, np.nan, np.nan)
    centre = (256, 192)
    five = lambda: [obs(c, (128 * (1 - s) + 256, 224) if c != 2 else (356, 324)) for c, s in ((0, 0.0), (3, 0.5), (2, 1.0), (4, 1.5), (5, 2.0))]
    point((5, 5, 5), [obs(0, centre), obs(1, centre)])                     # meet
    point(nan3, [obs(0, centre), obs(1, centre)])                          # meet_nan_input
    point((0, 0, 3), [obs(0, centre), obs(2, centre)])                     # parallel
    point((0, 0, 3), [obs(0, centre), (9, 0)])                             # one_usable
    k = obs(0, centre)
    point((0, 0, 3), [k, k, k])                                            # same_ray
    point((0, 0, 3), [obs(0, (0, 192)), obs(2, (512, 192))])               # behind: the lines meet at (0.5, 0, -1)
    point(nan3, five())                                                    # five: camera 2's keypoint is (100, 100) off
    point(FIVE_TRUTH, five())                                              # five_truth_input
    point((0, 0, 3), [])                                                   # empty_row
    point((1, 2, 3), [obs(0, centre), obs(1, centre)])                     # past_n
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    flat = [e for r in rows for e in r]
    return dict(points=np.array(pts, np.float32), n=len(pts) - 1, offsets=offsets, cam=np.array([e[0] for e in flat], np.int32),
                kp=np.array([e[1] for e in flat], np.int32), R=R, T=T, n_cams=Cs, xy=xy, K=HAND_K)


S = dict(zip(NAMES, range(len(NAMES))))
# variant -> (params, the statuses written by hand: point name -> status)
HAND_VARIANTS = {
    "defaults": ({}, dict(meet=rt.OK, meet_nan_input=rt.OK, parallel=rt.LOW_PARALLAX, one_usable=rt.TOO_FEW, same_ray=rt.LOW_PARALLAX,
                          behind=rt.BEHIND, five=rt.OK, five_truth_input=rt.OK, empty_row=rt.NO_PART, past_n=rt.NO_PART)),
    "any_parallax": (dict(cos_parallax_max=1.0), dict(meet=rt.OK, parallel=rt.DEGENERATE, same_ray=rt.DEGENERATE, one_usable=rt.TOO_FEW,
                                                      behind=rt.BEHIND)),
    "all_good": (dict(good10=10), dict(meet=rt.OK, five=rt.UNSUPPORTED, five_truth_input=rt.UNSUPPORTED)),
    # the linear start alone, with the support rule out of the way: the outlier drags it off, the true point costs less
    "linear_start": (dict(iterations=0, inlier_px=1000.0, good10=0), dict(meet=rt.OK, five=rt.OK, five_truth_input=rt.WORSE)),
}


def hand_cases():
    """variant -> the item with its params"""
    return {name: dict(hand_item(), params=prm) for name, (prm, _) in HAND_VARIANTS.items()}


def reference(c):
    return rt.triangulate_item(c["points"], c["n"], c["offsets"], c["cam"], c["kp"], c["R"], c["T"], c["n_cams"], c["xy"], c["K"], **c.get("params", {}))


def check_hand(name, got):
    """what was derived by hand, on any implementation's outputs for variant `name`"""
    c = hand_item()
    for pt, st in HAND_VARIANTS[name][1].items():
        assert got["status"][S[pt]] == st, (name, pt, got["status"][S[pt]])
    rows = np.array(c["points"])
    for pt in ("meet", "meet_nan_input"):
        rows[S[pt]] = (0, 0, 2, 1)
    keep = [S[k] for k in NAMES if k not in ("five", "five_truth_input")]
    assert np.array_equal(got["out_points"][keep].view(np.uint32), rows[keep].view(np.uint32)), name
    assert got["counts"][S["meet"]].tolist() == [2, 2] and got["counts"][S["one_usable"]].tolist() == [1, 0]
    info = got["info"]
    assert info[S["meet"], 0] == 0.0 and info[S["meet"], 1] == np.inf and info[S["meet"], 2] == 0.0
    assert np.isnan(info[S["meet_nan_input"], 1]) and info[S["parallel"], 0] == 1.0
    assert (info[[S["one_usable"], S["empty_row"], S["past_n"]]].view(np.uint64) == rt.QNAN64).all()
    if name == "defaults":
        assert got["counts"][S["five"]].tolist() == [5, 4]
        assert np.abs(got["out_points"][S["five"], :3] - FIVE_TRUTH).max() < 0.05 and got["out_points"][S["five"], 3] == 1.0
        assert got["stats"].tolist() == [8, 4, 2, 2]
    if name == "linear_start":
        assert np.array_equal(got["out_points"][S["five_truth_input"]].view(np.uint32), rows[S["five_truth_input"]].view(np.uint32))
        assert info[S["five_truth_input"], 2] > info[S["five_truth_input"], 1] > 0


# ------------------------------------------------------------------------------------------------ the serial program
def build_serial(tmpdir):
    out = os.path.join(str(tmpdir), "tracks_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "tracks_serial.cpp")], check=True)
    return out


def run_serial(exe, tmpdir, cases):
    """cases: a list of items (with optional params) -> the program's results in their order (None for a refused case)"""
    src, dst = os.path.join(str(tmpdir), "tracks_in.bin"), os.path.join(str(tmpdir), "tracks_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            S_, O = len(c["offsets"]) - 1, len(c["cam"])
            p = rt.params(**c.get("params", {}))
            Cs, Kp = len(c["R"]), c["xy"].shape[1]
            f.write(struct.pack("9i", S_, O, int(c["n"]), Cs, int(c["n_cams"]), Kp, p["iterations"], p["min_good"], p["good10"]))
            f.write(struct.pack("3d", p["cos_parallax_max"], p["huber_px"], p["inlier_px"]))
            for a, dt in ((c["K"], np.float32), (c["points"], np.float32), (c["offsets"], np.int32), (c["cam"], np.int32), (c["kp"], np.int32),
                          (c["R"], np.float64), (c["T"], np.float64), (c["xy"], np.float32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
    subprocess.run([exe, src, dst], check=True)
    buf = open(dst, "rb").read()
    pos, out = 0, []

    def take(n, dt=np.int32):
        nonlocal pos
        a = np.frombuffer(buf, dt, n, pos)
        pos += a.nbytes
        return a
    for c in cases:
        S_ = len(c["offsets"]) - 1
        if take(1)[0]:
            out.append(None)
            continue
        out.append(dict(out_points=take(4 * S_, np.float32).reshape(S_, 4), status=take(S_), counts=take(2 * S_).reshape(S_, 2),
                        info=take(3 * S_, np.float64).reshape(S_, 3), stats=take(4)))
    assert pos == len(buf)
    return out


def same_bits(got, ref, name=""):
    for k in rt.OUTS:
        a, b = np.ascontiguousarray(got[k]).reshape(-1).view(np.uint8), np.ascontiguousarray(ref[k]).reshape(-1).view(np.uint8)
        assert np.array_equal(a, b), (name, k)
