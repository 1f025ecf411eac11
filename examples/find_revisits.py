#!/usr/bin/env python3
"""Which earlier frames look like this one?  (include/vslam_places.h; composition only, no device code of its own.)

A few short synthetic tracks (synth.sequences_torch); a vocabulary trained on the first track's descriptors by k-majority; every
frame of every track added to an index, tagged (track, frame); then every frame queried against the entries whose id lies below
its own minus `--gap` (more than `--gap` ids older than itself), with the rounded-log weights of capi.places_weights.  The candidates are printed with their tags and
similarities, and the best one is verified the way the library leaves to its caller: the existing front end (match + RANSAC) runs on
the pair (candidate, query) and the inlier count is printed.

    python examples/find_revisits.py [--tracks 3] [--frames 8] [--gap 2] [--words 256]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vslam_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--gap", type=int, default=2)
    ap.add_argument("--words", type=int, default=256)
    a = ap.parse_args()
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

    for q in range(N):
        cand = ", ".join(f"({tag[e][0]}, {tag[e][1]}) {s / d:.3f}" for e, s, d in zip(best_id[q], score[q], den[q]) if e >= 0)
        line = f"frame ({tag[q][0]}, {tag[q][1]}): " + (cand or "no candidate")
        if q in inliers:
            line += f"   -> best verified with {inliers[q]} inlier matches"
        print(line)
    idx.close()
    ctx.close()


if __name__ == "__main__":
    main()
