"""The reference's main loop between frame pairs (src/vslam.cpp:53-270) and PointMap (src/PointMap.cpp), restated in plain
Python for ONE track, statement by statement from the reference's text.  The numeric stages are the oracle's exports
(extract_features, match_features, extract_Rt, camera_matrix, associate, triangulate, reprojection_filter); what is modelled
here is the bookkeeping around them: frame.R_t / frame.pose, the propagation of map_point_ids through the matches, the
observation pushes, add_reprojection_inliers and the colour pick.

Conventions the device state is compared under: map_point_ids rows have kp_stride entries (-1 = none), a pair without a RANSAC
winner leaves the map untouched (R_t identity, pose carried over), and a colour whose row int(x) lies outside the image is
(0, 0, 0) (the reference reads out of bounds there)."""
import numpy as np


def pose_product(last_pose, R_t):
    """last_frame.pose * frame.R_t (src/vslam.cpp:88) as OpenCV's small GEMM forms it: exact double products summed left to
    right in double, one rounding to float."""
    A = np.asarray(last_pose, np.float32).reshape(4, 4).astype(np.float64)
    B = np.asarray(R_t, np.float32).reshape(4, 4).astype(np.float64)
    out = np.zeros((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            s = A[r, 0] * B[0, c]
            s = s + A[r, 1] * B[1, c]
            s = s + A[r, 2] * B[2, c]
            s = s + A[r, 3] * B[3, c]
            out[r, c] = np.float32(s)
    return out


class Frame:
    def __init__(self, fid, xy, desc, nodes, kp_stride, image):
        self.id = fid
        self.points = np.asarray(xy, np.float32).reshape(-1, 2)
        self.descriptors = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.nodes = np.asarray(nodes, np.int32)
        self.map_point_ids = np.full(kp_stride, -1, np.int32)           # src/Frame.cpp:73
        self.image = image                                              # (H, W, 3) u8 or None
        self.R_t = np.eye(4, dtype=np.float32)
        self.pose = np.eye(4, dtype=np.float32)


class PointMapModel:
    """struct PointMap + the loop's per-frame state, one track."""

    def __init__(self, oracle, K, width, height, kp_stride, radius=2.0, dist_threshold=64, threshold_sq=4.0):
        self.o = oracle
        self.K = np.asarray(K, np.float32).reshape(3, 3)
        self.W, self.H = width, height
        self.kp_stride = kp_stride
        self.radius, self.dist_threshold, self.threshold_sq = radius, dist_threshold, threshold_sq
        self.size = 0
        self.points = np.zeros((0, 4), np.float32)
        self.colors = []                    # (b, g, r) per map point
        self.frame_ids = []                 # per map point, push order
        self.frame_point_ids = []
        self.frames = []
        # what happened (the non-vacuity conditions of the tests are asserted on these)
        self.stats = dict(propagation_pushes=0, association_claims=0, colors_outside=0, colors_inside=0, growth=[])

    # ---- first frame: identity pose, nothing else (src/vslam.cpp:66-68)
    def first_frame(self, xy, desc, nodes, image=None):
        self.frames.append(Frame(0, xy, desc, nodes, self.kp_stride, image))

    def orb_distance(self, map_point_id, frame, frame_point_id):        # src/PointMap.cpp:36-46
        mn = 0xFFFFFFFF
        d = frame.descriptors[frame_point_id]
        for fid, pid in zip(self.frame_ids[map_point_id], self.frame_point_ids[map_point_id]):
            cur = int(np.unpackbits(d ^ self.frames[fid].descriptors[pid]).sum())
            if cur < mn:
                mn = cur
        return mn

    def _csr(self):
        offs = np.zeros(self.size + 1, np.int32)
        rows = []
        for i in range(self.size):
            for fid, pid in zip(self.frame_ids[i], self.frame_point_ids[i]):
                rows.append(self.frames[fid].descriptors[pid])
            offs[i + 1] = len(rows)
        od = np.array(rows, np.uint8).reshape(-1, 32) if rows else np.zeros((1, 32), np.uint8)
        return offs, od

    # ---- every later frame: src/vslam.cpp:69-262
    def step(self, xy, desc, nodes, image, matches, F, has_model=True, pose=None):
        """matches: (k, 2) int (first = last frame's keypoint, second = this frame's), F the pair's fundamental matrix as
        match_features returns them; has_model False = RANSAC accepted no hypothesis.
        pose = (R (3, 3), t (3,), c2 (3, 4), points_4d (k, 4)): the values VSLAM_OPT_POSE_REFINE leaves after its adjustment.  They
        stand in for extract_Rt's, camera_matrix's and triangulate's, so that R_t and pose, the association, the filter and the
        appended points all use them (include/vslam_amd.h on the option); F is then not read."""
        o = self.o
        frame = Frame(len(self.frames), xy, desc, nodes, self.kp_stride, image)
        last_frame = self.frames[-1]
        self.frames.append(frame)
        if not has_model:
            frame.pose = last_frame.pose.copy()
            self.stats["growth"].append(0)
            return frame
        matches = np.asarray(matches, np.int32).reshape(-1, 2)
        if pose is not None:
            R, t = np.asarray(pose[0], np.float32).reshape(3, 3), np.asarray(pose[1], np.float32).reshape(3)
        else:
            R, t = o.extract_Rt(F, self.K)                                                # :82
        frame.R_t = np.eye(4, dtype=np.float32)
        frame.R_t[:3, :3] = R
        frame.R_t[:3, 3] = t
        frame.pose = pose_product(last_frame.pose, frame.R_t)                             # :88
        p1 = np.zeros((len(matches), 2), np.float32)
        p2 = np.zeros((len(matches), 2), np.float32)
        for i, (first, second) in enumerate(matches):                                      # :101-118
            p1[i] = last_frame.points[first]
            p2[i] = frame.points[second]
            last_id = int(last_frame.map_point_ids[first])
            if last_id > 0:
                frame.map_point_ids[second] = last_id
                self.frame_ids[last_id].append(frame.id)
                self.frame_point_ids[last_id].append(int(second))
                self.stats["propagation_pushes"] += 1
        c1 = np.zeros((3, 4), np.float32)
        c1[:, :3] = self.K
        c2 = o.camera_matrix(self.K, R, t) if pose is None else np.asarray(pose[2], np.float32).reshape(3, 4)   # :122
        if self.size > 0:                                                                  # :126-161
            offs, od = self._csr()
            n = len(frame.points)
            ids, claim = o.associate(self.points[:self.size], c2, self.W, self.H, frame.nodes, frame.points, frame.descriptors,
                                     offs, od, frame.map_point_ids[:n], radius=self.radius, thr=self.dist_threshold)
            frame.map_point_ids[:n] = ids
            for i in range(self.size):
                if claim[i] >= 0:
                    self.frame_ids[i].append(frame.id)
                    self.frame_point_ids[i].append(int(claim[i]))
                    self.stats["association_claims"] += 1
        points_4d = (o.triangulate(p1, p2, c1, c2) if pose is None                        # :186
                     else np.asarray(pose[3], np.float32).reshape(-1, 4)[:len(matches)])
        inliers, _ = o.reprojection_filter(points_4d, p1, p2, c1, c2, frame.map_point_ids[:max(len(matches), 1)],
                                           thr_sq=self.threshold_sq) if len(matches) else (np.zeros(0, np.int32), 0.0)
        colors = []
        for i in inliers:                                                                  # :247: at(row = x, column = y)
            row, col = int(p2[i, 0]), int(p2[i, 1])
            if image is not None and 0 <= row < image.shape[0] and 0 <= col < image.shape[1]:
                colors.append(tuple(int(v) for v in image[row, col]))
                self.stats["colors_inside"] += 1
            else:
                colors.append((0, 0, 0))
                self.stats["colors_outside"] += 1
        self.add_reprojection_inliers(points_4d, inliers, colors, last_frame.id, frame.id, matches)
        self.stats["growth"].append(len(inliers))
        return frame

    def add_reprojection_inliers(self, points_4d, inliers, colors, last_frame_id, frame_id, matches):   # src/PointMap.cpp:3-34
        self.colors.extend(colors)
        new = np.zeros((len(inliers), 4), np.float32)
        for j, row in enumerate(inliers):
            new[j, :3] = points_4d[row, :3]
            new[j, 3] = 1
            self.frame_point_ids.append([int(matches[row][0]), int(matches[row][1])])
        self.points = np.concatenate([self.points[:self.size], new]).astype(np.float32)
        self.size += len(inliers)
        while len(self.frame_ids) < self.size:
            self.frame_ids.append([last_frame_id, frame_id])

    # ---- the state in the device view's layout
    def observations(self):
        """(offsets [size + 1], frame_ids, point_ids) in push order."""
        offs = np.zeros(self.size + 1, np.int32)
        fr, pt = [], []
        for i in range(self.size):
            fr += self.frame_ids[i]
            pt += self.frame_point_ids[i]
            offs[i + 1] = len(fr)
        return offs, np.array(fr, np.int32), np.array(pt, np.int32)

    def snapshot(self):
        """A deep copy of everything a step can change (the capacity tests roll a track back to it)."""
        import copy
        return copy.deepcopy(dict(size=self.size, points=self.points, colors=self.colors, frame_ids=self.frame_ids,
                                  frame_point_ids=self.frame_point_ids, stats=self.stats))

    def restore(self, snap, drop_frame_state=True):
        """Undo the last step's effect on the map; the frame stays recorded without ids, R_t identity, pose carried over."""
        import copy
        s = copy.deepcopy(snap)
        self.size, self.points, self.colors = s["size"], s["points"], s["colors"]
        self.frame_ids, self.frame_point_ids, self.stats = s["frame_ids"], s["frame_point_ids"], s["stats"]
        if drop_frame_state:
            f = self.frames[-1]
            f.map_point_ids[:] = -1
            f.R_t = np.eye(4, dtype=np.float32)
            f.pose = self.frames[-2].pose.copy()


def ransac_winner(oracle, a, b, seed, hyp, threshold, ref=None):
    """The index of the hypothesis find_fundamental accepted for the pair, -1 for none (what the device reports in d_best[0]):
    match_features' stages run one by one (src/Frame.cpp:83-102), since its one-call form returns no winner."""
    pairs, rc = oracle.match_knn2_ratio(a["desc"], b["desc"])
    if rc != 0 or len(pairs) < 8:                       # find_fundamental needs 8 matches to draw a set
        return -1
    sets = oracle.ransac_sets(seed, len(pairs), hyp)
    r = oracle.find_fundamental(a["xy"], b["xy"], pairs, sets, threshold, want_all=False)
    if ref is not None and r["winner"] >= 0:            # the staged run is the one-call run
        assert np.array_equal(r["F"].view(np.uint32), np.asarray(ref["F"], np.float32).view(np.uint32))
        assert int(r["mask"].sum()) == len(ref["matches"])
    return int(r["winner"])


def run_track(oracle, frames_bgr, seeds, K, max_corners, cos_a, sin_a, pattern, hyp, threshold, kp_stride=None,
              map_capacity=None, obs_capacity=None, max_frames=None):
    """The whole loop for one track of images (frames, H, W, 3): returns the model.  With capacities, a step after which the
    map would hold more points / observations than fit is undone (model.overflowed counts them): within a step both only
    grow, so the totals at its end decide.  Frames from max_frames on are not recorded."""
    Fr, H, W, _ = frames_bgr.shape
    kp_stride = kp_stride or max_corners
    m = PointMapModel(oracle, K, W, H, kp_stride)
    feats = [oracle.extract_features(frames_bgr[f], max_corners, cos_a, sin_a, pattern) for f in range(Fr)]
    m.first_frame(feats[0]["xy"], feats[0]["desc"], feats[0]["nodes"], frames_bgr[0])
    m.overflowed = 0
    for f in range(1, Fr if max_frames is None else min(Fr, max_frames)):
        a, b = feats[f - 1], feats[f]
        ref = oracle.match_features(a["xy"], a["desc"], b["xy"], b["desc"], int(seeds[f - 1]), hyp, threshold)
        has_model = ransac_winner(oracle, a, b, int(seeds[f - 1]), hyp, threshold, ref) >= 0
        snap = m.snapshot()
        m.step(b["xy"], b["desc"], b["nodes"], frames_bgr[f], ref["matches"], ref["F"], has_model=has_model)
        n_obs = sum(len(x) for x in m.frame_ids)
        if (map_capacity is not None and m.size > map_capacity) or (obs_capacity is not None and n_obs > obs_capacity):
            m.restore(snap)
            m.stats["growth"].append(0)
            m.overflowed += 1
    return m
