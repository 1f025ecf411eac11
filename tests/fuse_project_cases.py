"""The hand cases of include/vslam_fuse_project.h that tests/test_ref_fuse_project.py (the reference and its plants),
tests/test_fuse_project_serial.py (the host walk) and tests/test_gpu_fuse_project.py (the device) share, the random items, and the serial
program's file format.  A case is a dict of one item's arrays in ref_fuse_project.random_item's keys plus `params` (fields of
vslam_search_params over the defaults), `found_stride` (or None) and `expect`: the found pairs (point, cam, kp, dist, holder) in
output order, written by hand, with `expect_stats` where the six counts are written out too.

Every camera of a hand case stands at the origin and looks down z (the rule does not ask them to differ), K = (525, 525, 320, 240) at
640 x 480: a point (0, 0, z) projects to (320, 240) exactly, so a keypoint at (328, 240) lies exactly on the default disc of 8 px.
D(b) is the descriptor with its first b bits set: the Hamming distance of D(a) and D(b) is |a - b|."""
import os
import struct
import subprocess

import numpy as np

import ref_fuse_project as rfp
import ref_resect as rr
from search_cases import D, up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = rr.kmat()
CX, CY = np.float32(K[0, 2]), np.float32(K[1, 2])
W, H = 640, 480
CENTRE = (CX, CY)
FAR = (20.0, 20.0)
INERT = ("n_zero", "n_negative", "broken_decreasing", "broken_negative_start", "broken_above_obs_stride")   # nothing is tried: no plant can show


def cam(kps=(), R=None, T=None, n_kp=None):
    """a camera: kps (x, y, descriptor) rows; the identity pose when R, T are None"""
    return dict(kps=list(kps), R=np.eye(3).reshape(9) if R is None else np.array(R, np.float64), T=np.zeros(3) if T is None else np.array(T, np.float64),
                n_kp=len(kps) if n_kp is None else n_kp)


def case(points, rows, cams, n=None, n_cams=None, kp_stride=None, cam_mask=None, found_stride=None, expect=(), expect_stats=None, **params):
    """points: (x, y, z) rows; rows: per point a list of (cam, kp, descriptor of that observation); cams: cam()s"""
    S, Cs = max(len(points), 1), len(cams)
    P = np.ones((S, 4), np.float32)
    P[:len(points), :3] = np.array(points, np.float32).reshape(-1, 3)
    offsets = np.zeros(S + 1, np.int32)
    offsets[1:len(rows) + 1] = np.cumsum([len(r) for r in rows])
    offsets[len(rows) + 1:] = offsets[len(rows)]
    flat = [e for r in rows for e in r] or [(0, 0, D(0))]
    Kp = kp_stride or max(max(len(c["kps"]) for c in cams), 1)
    xy = np.full((Cs, Kp, 2), 600.0, np.float32)
    desc = np.zeros((Cs, Kp, 32), np.uint8)
    for c, cm in enumerate(cams):
        for k, (x, y, d) in enumerate(cm["kps"]):
            xy[c, k], desc[c, k] = (x, y), d
    return dict(points=P, n=len(points) if n is None else n, offsets=offsets, cam=np.array([e[0] for e in flat], np.int32),
                kp=np.array([e[1] for e in flat], np.int32), obs_desc=np.array([e[2] for e in flat], np.uint8), R=np.stack([c["R"] for c in cams]),
                T=np.stack([c["T"] for c in cams]), n_cams=Cs if n_cams is None else n_cams, xy=xy, desc=desc,
                n_kp=np.array([c["n_kp"] for c in cams], np.int32), cam_mask=None if cam_mask is None else np.array(cam_mask, np.int32), K=K, width=W,
                height=H, found_stride=found_stride, params=params, expect=[tuple(e) for e in expect],
                expect_stats=None if expect_stats is None else np.array(expect_stats, np.int32))


def hand_cases():
    c = {}
    home = cam([(CX, CY, D(0))])                 # camera 0: the keypoint in which point 0 is seen already
    seen0 = [(0, 0, D(0))]                        # the row of a point seen in camera 0 at keypoint 0
    p0 = (0, 0, 2)
    # the disc is closed; one f32 step further out the keypoint is no candidate
    c["disc_on"] = case([p0], [seen0], [home, cam([(CX + np.float32(8), CY, D(3))])], expect=[(0, 1, 0, 3, -1)], expect_stats=[1, 1, 1, 1, 0, 1])
    c["disc_past"] = case([p0], [seen0], [home, cam([(up(CX + np.float32(8)), CY, D(3))])], expect=[], expect_stats=[1, 1, 0, 0, 0, 0])
    # a point already seen in a camera is not tried there, whatever waits for it
    c["already_seen"] = case([p0], [[(0, 1, D(0))]], [cam([(CX, CY, D(0)), FAR + (D(9),)])], expect=[], expect_stats=[0, 0, 0, 0, 0, 0])
    c["seen_at_invalid_kp"] = case([p0, (0, 0, -1)], [[(0, 2, D(0))], [(0, 0, D(0))]], [cam([(CX, CY, D(0)), FAR + (D(9),)])],
                                   expect=[(0, 0, 0, 0, 1)], expect_stats=[1, 1, 1, 1, 1, 1])   # kp 2 == kp_stride: no valid entry, so tried
    # a keypoint held by two points (which stand behind the cameras and propose nothing): the holder is the smaller index
    behind = (0, 0, -1)
    c["holder_smaller"] = case([p0, behind, behind], [seen0, [(1, 0, D(0))], [(1, 0, D(0))]], [home, cam([(CX, CY, D(1))])],
                               expect=[(0, 1, 0, 1, 1)], expect_stats=[3, 1, 1, 1, 1, 1])
    # a free keypoint beside a held one
    c["free_keypoint"] = case([p0, behind], [seen0, [(1, 1, D(0))]], [home, cam([(CX, CY, D(2)), (CX + 1, CY, D(40))])], expect=[(0, 1, 0, 2, -1)],
                              expect_stats=[2, 1, 1, 1, 0, 1])
    # two points proposing one keypoint, tied on d0: the smaller i wins and the other gets nothing
    two = cam([(CX, CY, D(4)), (CX, CY, D(40))])
    c["tie_smaller_i"] = case([p0, (0, 0, 3)], [[(0, 0, D(4))], [(0, 1, D(4))]], [two, cam([(CX, CY, D(0))])], expect=[(0, 1, 0, 4, -1)],
                              expect_stats=[2, 2, 2, 1, 0, 1])
    c["contest_lower_d"] = case([p0, (0, 0, 3)], [[(0, 0, D(4))], [(0, 1, D(2))]], [two, cam([(CX, CY, D(0))])], expect=[(1, 1, 0, 2, -1)],
                                expect_stats=[2, 2, 2, 1, 0, 1])
    # 10 d0 < ratio10 d1 fails at 8 against 10
    c["ratio_failure"] = case([p0], [seen0], [home, cam([(CX, CY, D(10)), (CX + 1, CY, D(8))])], expect=[], expect_stats=[1, 1, 0, 0, 0, 0])
    c["ratio_off"] = case([p0], [seen0], [home, cam([(CX, CY, D(10)), (CX + 1, CY, D(8))])], ratio10=0, expect=[(0, 1, 1, 8, -1)])
    # cameras that take no part
    waits = cam([(CX, CY, D(0))])
    c["masked_camera"] = case([p0], [seen0], [home, waits], cam_mask=[0, -1], expect=[], expect_stats=[0, 0, 0, 0, 0, 0])
    c["mask_zero_is_no_mask"] = case([p0], [seen0], [home, waits], cam_mask=[5, 0], expect=[(0, 1, 0, 0, -1)])
    c["nan_camera"] = case([p0], [seen0], [home, cam([(CX, CY, D(0))], T=(0, np.nan, 0))], expect=[], expect_stats=[0, 0, 0, 0, 0, 0])
    c["inf_rotation"] = case([p0], [seen0], [home, cam([(CX, CY, D(0))], R=(1, 0, 0, 0, 1, 0, np.inf, 0, 1))], expect=[])
    c["camera_at_C"] = case([p0], [seen0], [home, waits], n_cams=1, expect=[], expect_stats=[0, 0, 0, 0, 0, 0])
    c["cameras_above_stride"] = case([p0], [seen0], [home, waits], n_cams=9, expect=[(0, 1, 0, 0, -1)])
    # keypoint counts
    c["n_kp_zero"] = case([p0], [seen0], [home, cam([(CX, CY, D(0))], n_kp=0)], expect=[], expect_stats=[1, 1, 0, 0, 0, 0])
    c["n_kp_negative"] = case([p0], [seen0], [home, cam([(CX, CY, D(0))], n_kp=-4)], expect=[])
    c["n_kp_above_stride"] = case([p0], [seen0], [home, cam([(CX, CY, D(0))], n_kp=99)], expect=[(0, 1, 0, 0, -1)])
    # points that take no part: not finite, an empty row; neither proposes, the first still holds its keypoint
    c["nan_point"] = case([p0, (np.nan, 0, 2)], [seen0, [(0, 1, D(0))]], [cam([(CX, CY, D(0)), FAR + (D(0),)]), cam([(CX, CY, D(0))])],
                          expect=[(0, 1, 0, 0, -1)], expect_stats=[1, 1, 1, 1, 0, 1])
    c["nan_point_holds"] = case([(np.inf, 0, 2), p0], [[(1, 0, D(0))], seen0], [home, cam([(CX, CY, D(0))])], expect=[(1, 1, 0, 0, 0)])
    c["empty_row"] = case([p0, p0], [seen0, []], [home, cam([(CX, CY, D(0))])], expect=[(0, 1, 0, 0, -1)], expect_stats=[1, 1, 1, 1, 0, 1])
    c["n_zero"] = case([p0], [seen0], [home, waits], n=0, expect=[], expect_stats=[0, 0, 0, 0, 0, 0])
    c["n_negative"] = case([p0], [seen0], [home, waits], n=-2, expect=[], expect_stats=[0, 0, 0, 0, 0, 0])
    c["n_above_stride"] = case([p0], [seen0], [home, waits], n=7, expect=[(0, 1, 0, 0, -1)])
    # the three broken CSRs of fuse_cases: nothing found, zero stats
    for name, edit in (("broken_decreasing", lambda o: o.__setitem__(2, o[1] - 1)), ("broken_negative_start", lambda o: o.__setitem__(0, -1)),
                       ("broken_above_obs_stride", lambda o: o.__setitem__(3, 99))):
        k = case([p0, p0, p0], [seen0, [(0, 0, D(0))], [(0, 0, D(0))]], [home, waits], expect=[], expect_stats=[0, 0, 0, 0, 0, 0])
        edit(k["offsets"])
        c[name] = k
    # two found pairs whose (c, i) order is not their (i, c) order; then found_stride one below the number found
    right = (np.float32(372.5), CY)               # where (0.2, 0, 2) projects: 525 x 0.1 + 320
    order = dict(points=[p0, (0.2, 0, 2)], rows=[[(0, 0, D(0)), (1, 0, D(0))], [(0, 1, D(90)), (2, 0, D(90))]],
                 cams=[cam([(CX, CY, D(0)), right + (D(90),)]), cam([(CX, CY, D(0)), right + (D(91),)]), cam([right + (D(90),), (CX, CY, D(5))])])
    c["order_c_then_i"] = case(**order, expect=[(1, 1, 1, 1, -1), (0, 2, 1, 5, -1)], expect_stats=[2, 2, 2, 2, 0, 2])
    c["found_stride_one_short"] = case(**order, found_stride=1, expect=[(1, 1, 1, 1, -1)], expect_stats=[2, 2, 2, 2, 0, 1])
    return c


def random_cases():
    """n on both sides of a 256-lane chunk and of the proposals' 1024 points; 1, 2 and 9 cameras; kp_stride 96 with n_kp differing per
    camera; junk entries; descriptors through flip_bits"""
    c = {}
    for n, cams in ((1, 1), (255, 2), (256, 9), (257, 2), (600, 9)):
        c[f"n{n}c{cams}"] = rfp.random_item(31 * n + cams, n, cams, kp_stride=96, cam_stride=cams + (1 if cams > 1 else 0), S=n + 3)
    c["n257c9_masked"] = dict(rfp.random_item(5, 257, 9, kp_stride=96), cam_mask=np.array([0, 3, -1, 0, 0, -7, 0, 0, 1], np.int32))
    c["n600c2_r3"] = dict(rfp.random_item(6, 600, 2, kp_stride=96), params=dict(radius_px=3.0, dist_threshold=50, ratio10=9))
    return c


def found_of(r):
    """a result's found pairs as the tuples `expect` holds"""
    m = int(r["n_found"])
    return [tuple(int(r[k][j]) for k in ("found_point", "found_cam", "found_kp", "found_dist", "found_holder")) for j in range(m)]


# ------------------------------------------------------------------------------------------------ the serial program
def build_serial(tmpdir):
    out = os.path.join(str(tmpdir), "fuse_project_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, os.path.join(ROOT, "tests", "native", "fuse_project_serial.cpp")], check=True)
    return out


def run_serial(exe, tmpdir, cases):
    """cases: a list of cases -> the program's results in their order (dicts as ref_fuse_project.project_item returns them)"""
    src, dst = os.path.join(str(tmpdir), "fp_in.bin"), os.path.join(str(tmpdir), "fp_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            p = dict(rfp.rs.DEFAULTS)
            p.update(c.get("params", {}))
            S, O, Cs, Kp = len(c["points"]), len(c["cam"]), len(c["R"]), c["xy"].shape[1]
            m = c.get("cam_mask")
            fs = c.get("found_stride")
            f.write(struct.pack("12i", S, O, Cs, Kp, int(c["n"]), int(c["n_cams"]), c["width"], c["height"], 0 if m is None else 1,
                                Cs * S if fs is None else fs, p["dist_threshold"], p["ratio10"]))
            f.write(struct.pack("d", p["radius_px"]))
            arrays = [(c["K"], np.float32), (c["points"], np.float32), (c["offsets"], np.int32), (c["cam"], np.int32), (c["kp"], np.int32),
                      (c["obs_desc"], np.uint8), (c["R"], np.float64), (c["T"], np.float64), (c["xy"], np.float32), (c["desc"], np.uint8),
                      (c["n_kp"], np.int32)] + ([] if m is None else [(m, np.int32)])
            for a, dt in arrays:
                f.write(np.ascontiguousarray(a, dt).tobytes())
    subprocess.run([exe, src, dst], check=True)
    buf = open(dst, "rb").read()
    pos, out = 0, []

    def take(n):
        nonlocal pos
        a = np.frombuffer(buf, np.int32, n, pos)
        pos += a.nbytes
        return a
    for _ in cases:
        m = int(take(1)[0])
        r = dict(n_found=m)
        for k in rfp.OUTS:
            r[k] = take(m)
        r["stats"] = take(6)
        out.append(r)
    assert pos == len(buf)
    return out
