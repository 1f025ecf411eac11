#!/usr/bin/env python3
"""Which earlier frames look like this one?  (include/vslam_places.h; composition only, no device code of its own.)

A few short synthetic tracks (synth.sequences_torch); a vocabulary trained on the first track's descriptors by k-majority; every
frame of every track added to an index, tagged (track, frame); then every frame queried against the entries whose id lies below
its own minus `--gap` (more than `--gap` ids older than itself), with the rounded-log weights of capi.places_weights.  The candidates are printed with their tags and
similarities, and the best one is verified the way the library leaves to its caller: the existing front end (match + RANSAC) runs on
the pair (candidate, query) and the inlier count is printed.

With --sim3 the similarity between the two frames' maps is printed as well (include/vslam_sim3.h).  Each of the two frames is
triangulated against its neighbour in its own track (vslam_frontend_pairs_pose: points in that frame's camera coordinates, in the
unit of that pair's baseline), the front end's inlier matches between candidate and query that have a point on both sides become
3-D / 3-D correspondences, and Context.sim3_ransac relates them: B = s R A + t takes the candidate's little map to the query's.  s is
the ratio of the two baselines, which nothing else in this file knows.  No polish: a revisit may share its camera centre with
the candidate, where the polish cannot see the scale.  Expect "not found" often: two-view points over a short
baseline are rough, and inlier_px (2 px, both ways) is untuned.

With --close --project the geometric round (World.fuse_project, include/vslam_fuse_project.h) then runs over the two end frames of every
closed loop: the world points are searched by projection in those frames, and map points that never shared a keypoint become one track.
With --close (implies --sim3) the found similarities whose two frames lie in ONE track become loops of that track: the tracks are run
through Context.track_sequences into a PointMap with a world attached, each model is brought into the world's unit with the world's
per-pair scales (A and B above are in the units of their own pairs' baselines), and World.close_loops (include/vslam_graph.h) spreads
every loop's error over the frames between its ends.  The statistics per track are printed: usable edges, mean cost before and
after, accepted steps.  No policy decides which loops deserve it: every found one is taken.

    python examples/find_revisits.py [--tracks 3] [--frames 8] [--gap 2] [--words 256] [--sim3] [--close [--project]]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vslam_amd import capi, synth  # noqa: E402


def similarities(ctx, a, bgr, asked, best_id, sizes, rot, dev, models):
    """{query: text}: for every query with a candidate, three pairs through vslam_frontend_pairs_pose -- (candidate, its neighbour),
    (query, its neighbour), (candidate, query) -- then one batch of Context.sim3_ransac over what the three have in common"""
    width, height, max_corners, hyp = sizes
    cos_a, sin_a, pat = rot
    K = np.array([[525, 0, width // 2], [0, 525, height // 2], [0, 0, 1]], np.float32)

    def neighbour(f):   # the next frame of f's own track, the previous one for a track's last frame
        return f + 1 if (f % a.frames) + 1 < a.frames else f - 1
    cands = [int(best_id[q, 0]) for q in asked]
    P = len(asked)
    last = cands + list(asked) + cands
    cur = [neighbour(c) for c in cands] + [neighbour(q) for q in asked] + list(asked)
    both = torch.cat([bgr[last], bgr[cur]]).contiguous()
    seeds = torch.arange(3 * P, dtype=torch.int32, device=dev)
    o = ctx.frontend_pairs_pose(both, 3 * P, max_corners, cos_a, sin_a, pat, seeds, hyp, 10.0, K)
    ctx.synchronize()
    xy, matches, best, X = (o[k].cpu().numpy() for k in ("xy", "matches", "best", "points4d"))
    S = max_corners
    A, B = np.full((P, S, 3), np.nan), np.full((P, S, 3), np.nan)
    xa, xb = np.full((P, S, 2), np.nan, np.float32), np.full((P, S, 2), np.nan, np.float32)
    n = np.zeros(P, np.int32)

    def points_of(pair):   # keypoint of the pair's first frame -> its point in that frame's camera coordinates
        out = {}
        for m in range(max(int(best[pair, 3]), 0) if best[pair, 0] >= 0 else 0):
            p = X[pair, m].astype(np.float64)
            if np.isfinite(p).all() and p[3] != 0 and p[2] / p[3] > 0:
                out[int(matches[pair, m, 0])] = p[:3] / p[3]
        return out
    for i in range(P):
        # the same image gives the same keypoints in every pair it takes part in: the extractor depends on the image alone
        assert np.array_equal(xy[i], xy[2 * P + i]) and np.array_equal(xy[P + i], xy[3 * P + 2 * P + i])
        pc, pq = points_of(i), points_of(P + i)
        for m in range(max(int(best[2 * P + i, 3]), 0) if best[2 * P + i, 0] >= 0 else 0):
            kc, kq = (int(v) for v in matches[2 * P + i, m])
            if kc in pc and kq in pq:
                A[i, n[i]], B[i, n[i]], xa[i, n[i]], xb[i, n[i]] = pc[kc], pq[kq], xy[i, kc], xy[P + i, kq]
                n[i] += 1
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    r = ctx.sim3_ransac(t(A), t(xa), t(B), t(xb), t(n), K, torch.arange(1, P + 1, dtype=torch.int32, device=dev), torch.zeros(P, **f64),
                        torch.zeros((P, 9), **f64), torch.zeros((P, 3), **f64), hypotheses=256)
    ctx.synchronize()
    win, cnt, s, R, T = (r[k].cpu().numpy() for k in ("winner", "n_inliers", "scale", "R", "T"))
    out = {}
    models.extend((cands[i], q, float(s[i]), R[i].copy(), T[i].copy()) for i, q in enumerate(asked) if win[i] >= 0)
    for i, q in enumerate(asked):
        if win[i] < 0:
            out[q] = f"sim3: not found among {n[i]} 3-D pairs"
        else:
            ang = np.degrees(np.arccos(np.clip((np.trace(R[i].reshape(3, 3)) - 1) / 2, -1, 1)))
            out[q] = f"sim3: s {s[i]:.3f}, turn {ang:.1f} deg, t ({T[i][0]:.2f}, {T[i][1]:.2f}, {T[i][2]:.2f}) from {cnt[i]} of {n[i]} 3-D pairs"
    return out


def close_loops(ctx, a, bgr, models, sizes, rot, dev, project=False):
    """the found same-track models as loops of a world built from the same frames; prints World.close_loops' statistics"""
    width, height, max_corners, hyp = sizes
    cos_a, sin_a, pat = rot
    K = np.array([[525, 0, width // 2], [0, 525, height // 2], [0, 0, 1]], np.float32)
    same = [m for m in models if m[0] // a.frames == m[1] // a.frames]
    print(f"loops: {len(same)} of {len(models)} found similarities join two frames of one track")
    if not same:
        return
    seeds = torch.arange(a.tracks * (a.frames - 1), dtype=torch.int32, device=dev).reshape(a.tracks, a.frames - 1).contiguous()
    pmap = capi.PointMap(ctx, a.tracks, a.frames, max_corners, map_capacity=a.frames * max_corners, obs_capacity=4 * a.frames * max_corners)
    world = pmap.attach_world()
    kp = ctx.track_sequences(pmap, bgr.reshape(a.tracks, a.frames, height, width, 3), max_corners, cos_a, sin_a, None, seeds, hyp, 10.0, K)
    ctx.synchronize()
    scale = world.view()["scale"]
    unit = lambda f: float(scale[f // a.frames, min(f % a.frames + 1, a.frames - 1)])   # the world's scale of the pair f was triangulated in
    rows, s, R, T = [], [], [], []
    for c, q, ms, mR, mT in same:   # camera a = the candidate, camera b = the query, both in the world's unit
        rows.append((c // a.frames, c % a.frames, q % a.frames))
        s.append(ms * unit(q) / unit(c))
        R.append(mR)
        T.append(mT * unit(q))
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dt)).to(dev)
    stats = world.close_loops(pmap, t(rows, np.int32), t(s, np.float64), t(R, np.float64), t(T, np.float64))
    ctx.synchronize()
    for k, st in enumerate(stats.cpu().numpy()):
        moved = "left alone" if np.isnan(st[3]) else f"cost per edge {st[1]:.3e} -> {st[2]:.3e} in {int(st[3])} steps"
        print(f"track {k}: {int(st[0])} usable edges, {moved}")
    if project:   # the geometric round over the two ends of every closed loop (include/vslam_fuse_project.h)
        world.fuse(pmap)
        for trk, fa, fb in sorted(set(rows)):
            for f in sorted({fa, fb}):
                ps = world.fuse_project(pmap, kp["xy"], kp["desc"], kp["n"], K, width, height, frames=(f, f + 1)).cpu().numpy()
                print(f"loop of track {trk}, frame {f}: tried {ps[trk, 0]}, found {ps[trk, 3]}, links {ps[trk, 4]}, extras held {ps[trk, 7]}")
    world.close()
    pmap.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--gap", type=int, default=2)
    ap.add_argument("--words", type=int, default=256)
    ap.add_argument("--sim3", action="store_true", help="print the similarity between the best candidate's map and the query's")
    ap.add_argument("--close", action="store_true", help="close the same-track loops among the found similarities (implies --sim3)")
    ap.add_argument("--project", action="store_true", help="with --close: fuse the map points of each closed loop's two ends by projection")
    a = ap.parse_args()
    a.sim3 = a.sim3 or a.close
    width, height, max_corners, hyp, top_k = 320, 240, 1000, 256, 3
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    cos_a, sin_a = synth.keypoint_rotation()
    pat = torch.from_numpy(synth.brief_pattern()).to(dev)
    bgr = synth.sequences_torch(7, a.tracks, a.frames, width, height, dev).reshape(a.tracks * a.frames, height, width, 3).contiguous()
    N = bgr.shape[0]
    fe = ctx.extract_features(bgr, max_corners, cos_a, sin_a, pat)
    desc, n = fe["desc"], fe["n"]
    ctx.synchronize()

    first = torch.cat([desc[f, :int(n[f])] for f in range(a.frames)]).contiguous()          # the first track's descriptors
    tr = ctx.places_train(first, a.words, 4)
    print(f"vocabulary: {a.words} words from {first.shape[0]} descriptors, {int((tr['sizes'] == 0).sum())} of them empty")

    idx = capi.Places(ctx, a.words, N, max_corners)
    idx.set_vocabulary(tr["vocab"])
    tags = torch.tensor([(t, f) for t in range(a.tracks) for f in range(a.frames)], dtype=torch.int32, device=dev)
    ids = idx.add(desc, n, tags)
    idx.set_weights(torch.from_numpy(capi.places_weights(idx.view()["df"], N)).to(dev))
    below = (ids - a.gap).contiguous()
    res = idx.query(desc, n, top_k, below)
    ctx.synchronize()
    best_id, score, den = (res[k].cpu().numpy() for k in ("best_id", "best_score", "best_den"))
    tag = tags.cpu().numpy()

    # verification of every query's best candidate: the front end on the pairs (candidate, query)
    asked = [q for q in range(N) if best_id[q, 0] >= 0]
    inliers = {}
    if asked:
        pairs = len(asked)
        both = torch.cat([bgr[[int(best_id[q, 0]) for q in asked]], bgr[asked]]).contiguous()
        seeds = torch.arange(pairs, dtype=torch.int32, device=dev)
        out = ctx.frontend_pairs(both, pairs, max_corners, cos_a, sin_a, pat, seeds, hyp, 10.0)
        ctx.synchronize()
        inliers = dict(zip(asked, out["best"][:, 3].cpu().numpy().tolist()))

    models = []
    sim3 = similarities(ctx, a, bgr, asked, best_id, (width, height, max_corners, hyp), (cos_a, sin_a, pat), dev, models) if a.sim3 and asked else {}

    for q in range(N):
        cand = ", ".join(f"({tag[e][0]}, {tag[e][1]}) {s / d:.3f}" for e, s, d in zip(best_id[q], score[q], den[q]) if e >= 0)
        line = f"frame ({tag[q][0]}, {tag[q][1]}): " + (cand or "no candidate")
        if q in inliers:
            line += f"   -> best verified with {inliers[q]} inlier matches"
        if q in sim3:
            line += "; " + sim3[q]
        print(line)
    if a.close:
        close_loops(ctx, a, bgr, models, (width, height, max_corners, hyp), (cos_a, sin_a, pat), dev, project=a.project)
    idx.close()
    ctx.close()


if __name__ == "__main__":
    main()
