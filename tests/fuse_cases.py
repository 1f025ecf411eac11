"""The hand cases of include/vslam_fuse.h that tests/test_fuse_serial.py (the host walk) and tests/test_gpu_fuse.py (the device) share,
and the serial program's file format.  A fusion case: dict(n, offsets, cam, kp, cam_stride, kp_stride, mask or None, expect = fuse_to);
a cull case: dict(points, n, offsets, cam, kp, R, T, n_cams, xy, K, params, expect = keep, expect_counts)."""
import os
import struct
import subprocess

import numpy as np

import ref_fuse as rf
import ref_resect as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fuse(rows, n=None, S=None, mask=None, cam_stride=6, kp_stride=64, expect=None, tail=None):
    """rows: a list of [(cam, kp), ...] per point; S > len(rows): rows past them with junk offsets (`tail`)"""
    S = S or len(rows)
    counts = [len(r) for r in rows]
    offsets = np.zeros(S + 1, np.int32)
    offsets[1:len(rows) + 1] = np.cumsum(counts)
    offsets[len(rows) + 1:] = offsets[len(rows)] if tail is None else tail
    flat = [e for r in rows for e in r] or [(0, 0)]
    return dict(n=len(rows) if n is None else n, offsets=offsets, cam=np.array([e[0] for e in flat], np.int32),
                kp=np.array([e[1] for e in flat], np.int32), cam_stride=cam_stride, kp_stride=kp_stride,
                mask=None if mask is None else np.array(mask, np.int32), expect=None if expect is None else np.array(expect, np.int32))


def fuse_hand_cases():
    c = {}
    c["no_link"] = _fuse([[(0, 1), (1, 1)], [(1, 2), (2, 2)], [(2, 3)]], expect=[0, 1, 2])
    c["one_pair"] = _fuse([[(0, 1), (1, 2)], [(0, 9)], [(1, 2), (2, 3)]], expect=[0, 1, 0])
    c["chain_of_three"] = _fuse([[(0, 1), (1, 1)], [(1, 1), (2, 1)], [(2, 1), (3, 1)]], expect=[0, 0, 0])
    c["two_shared_cells"] = _fuse([[(4, 4)], [(0, 1), (1, 2)], [(1, 2), (0, 1)]], expect=[0, 1, 1])
    c["duplicate_inside_a_row"] = _fuse([[(0, 1), (0, 1), (1, 2), (0, 1)], [(3, 3)]], expect=[0, 1])
    c["invalid_entries"] = _fuse([[(-1, 5), (0, 1)], [(0, 64), (0, 1)], [(6, 1), (0, -2)], [(-1, 5), (2, 2)], [(-1, 5), (3, 3)], [(5, 63), (2, 2)]],
                                 expect=[0, 0, 2, 3, 4, 3])
    c["masked_bridge"] = _fuse([[(0, 1)], [(0, 1), (1, 1)], [(1, 1)], [(0, 1)]], mask=[0, -1, 7, 0], expect=[0, -1, 2, 0])
    c["n_zero"] = _fuse([[(0, 1)], [(0, 1)]], n=0, S=4, expect=[0, 1, 2, 3])
    c["n_negative"] = _fuse([[(0, 1)], [(0, 1)]], n=-3, expect=[0, 1])
    c["n_is_pt_stride"] = _fuse([[(0, 1)], [(2, 1)], [(0, 1)], [(2, 1), (0, 1)]], n=9, expect=[0, 0, 0, 0])
    c["junk_past_n"] = _fuse([[(0, 1)], [(0, 1)], [(0, 1)]], n=2, S=6, tail=-99, expect=[0, 0, 2, 3, 4, 5])
    for name, edit in (("broken_decreasing", lambda o: o.__setitem__(2, o[1] - 1)), ("broken_negative_start", lambda o: o.__setitem__(0, -1)),
                       ("broken_above_obs_stride", lambda o: o.__setitem__(3, 99))):
        k = _fuse([[(0, 1), (1, 1)], [(0, 1)], [(1, 1)]], expect=[0, 1, 2])
        edit(k["offsets"])
        c[name] = k
    return c


def cull_hand_case():
    """One item, six cameras, all at the origin looking down z (the rule does not ask them to differ): a point (0, 0, z) projects to
    (cx, cy) exactly, so a keypoint at (cx + 6, cy) lies exactly on the default disc.  One point per rule; `expect`, `expect_counts`
    are written by hand."""
    K = rr.kmat()
    cx, cy = np.float32(K[0, 2]), np.float32(K[1, 2])
    Cs, Kp = 6, 16
    R = np.tile(np.eye(3).reshape(9), (Cs, 1))
    T = np.zeros((Cs, 3))
    R[1, 0] = np.inf                                             # camera 1 is not finite
    xy = np.full((Cs, Kp, 2), 1000.0, np.float32)               # far from (cx, cy) wherever not set
    on, off_ = (cx + np.float32(6), cy), (np.nextafter(cx + np.float32(6), np.float32(np.inf)), cy)
    centre = (cx, cy)
    rows, pts, expect, counts = [], [], [], []
    nxt = [0] * Cs

    def obs(cam, where):
        k = nxt[cam]
        nxt[cam] += 1
        xy[cam, k] = where
        return cam, k

    def point(P, entries, keep, cnt):
        pts.append(list(P) + [1.0]); rows.append(entries); expect.append(keep); counts.append(cnt)
    point((0, 0, 1), [obs(4, on), obs(5, (cx, cy - np.float32(6)))], 1, (2, 2))                       # exactly on the disc, twice
    point((0, 0, 1), [obs(4, on), obs(5, off_)], 0, (2, 1))                                            # one f32 step outside
    point((0, 0, -1), [obs(4, centre), obs(5, centre)], 0, (2, 0))                                     # Y_z < 0
    point((0, 0, 0), [obs(4, centre), obs(5, centre)], 0, (2, 0))                                      # Y_z == 0
    point((0, 0, 2), [obs(1, centre), obs(4, centre), obs(5, centre)], 1, (2, 2))                      # the non-finite camera is not usable
    point((0, 0, 2), [obs(1, centre), obs(5, centre)], 0, (1, 1))
    point((0, 0, 2), [obs(0, centre), obs(2, centre)], 0, (2, 2))                                      # last + mature_age == C - 1: mature, needs 3
    point((0, 0, 2), [obs(0, centre), obs(2, centre), obs(2, centre)], 1, (3, 3))
    point((0, 0, 2), [obs(0, centre), obs(3, centre)], 1, (2, 2))                                      # last + mature_age == C: young, needs 2
    point((0, 0, 2), [obs(3, centre), obs(3, centre), obs(4, (0, 0)), obs(5, (0, 0))], 1, (4, 2))      # 10 n_good == good10 n_usable
    point((0, 0, 2), [obs(3, centre), obs(3, centre), obs(4, (0, 0)), obs(5, (0, 0)), obs(5, (1, 1))], 0, (5, 2))   # one short
    point((0, 0, 2), [], -1, (0, 0))                                                                   # an empty row
    point((np.nan, 0, 2), [obs(4, centre), obs(5, centre)], -1, (0, 0))                                # a non-finite point
    point((0, 0, 2), [obs(4, (np.nan, cy)), obs(5, centre), (9, 0), (-1, 0), (2, Kp), (2, -1)], 0, (1, 1))   # unusable entries
    point((0, 0, 2), [obs(4, centre), obs(5, centre)], -1, (0, 0))                                     # past n
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    flat = [e for r in rows for e in r]
    return dict(points=np.array(pts, np.float32), n=len(pts) - 1, offsets=offsets, cam=np.array([e[0] for e in flat], np.int32),
                kp=np.array([e[1] for e in flat], np.int32), R=R, T=T, n_cams=Cs, xy=xy, K=K, params={},
                expect=np.array(expect, np.int32), expect_counts=np.array(counts, np.int32))


def fuse_reference(c):
    return rf.fuse_item(c["n"], c["offsets"], c["cam"], c["kp"], c["cam_stride"], c["kp_stride"], c.get("mask"))


def cull_reference(c):
    return rf.cull_item(c["points"], c["n"], c["offsets"], c["cam"], c["kp"], c["R"], c["T"], c["n_cams"], c["xy"], c["K"], **c.get("params", {}))


# ------------------------------------------------------------------------------------------------ the serial program
def build_serial(tmpdir):
    out = os.path.join(str(tmpdir), "fuse_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "fuse_serial.cpp")], check=True)
    return out


def run_serial(exe, tmpdir, cases):
    """cases: a list of fusion cases (they have cam_stride) and cull cases -> the program's results in their order"""
    src, dst = os.path.join(str(tmpdir), "fuse_in.bin"), os.path.join(str(tmpdir), "fuse_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            S, O = len(c["offsets"]) - 1, len(c["cam"])
            if "cam_stride" in c:
                m = c.get("mask")
                f.write(struct.pack("7i", 0, S, O, int(c["n"]), c["cam_stride"], c["kp_stride"], 0 if m is None else 1))
                arrays = [(c["offsets"], np.int32), (c["cam"], np.int32), (c["kp"], np.int32)] + ([] if m is None else [(m, np.int32)])
            else:
                p = rf.cull_params(**c.get("params", {}))
                Cs, Kp = len(c["R"]), c["xy"].shape[1]
                f.write(struct.pack("11i", 1, S, O, int(c["n"]), Cs, int(c["n_cams"]), Kp, p["min_good"], p["mature_good"], p["mature_age"], p["good10"]))
                f.write(struct.pack("d", p["inlier_px"]))
                arrays = [(c["K"], np.float32), (c["points"], np.float32), (c["offsets"], np.int32), (c["cam"], np.int32), (c["kp"], np.int32),
                          (c["R"], np.float64), (c["T"], np.float64), (c["xy"], np.float32)]
            for a, dt in arrays:
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
        S = len(c["offsets"]) - 1
        if "cam_stride" in c:
            r = dict(fuse_to=take(S), out_offsets=take(S + 1))
            t = int(take(1)[0])
            r.update(out_cam=take(t), out_kp=take(t), out_src=take(t), stats=take(4))
        else:
            r = dict(keep=take(S), counts=take(2 * S).reshape(S, 2), stats=take(4))
        out.append(r)
    assert pos == len(buf)
    return out
