"""What the resident map costs (vslam_map_* / vslam_track_sequences), one arrangement per process:
  python tools/map_bench.py --what step      ms per vslam_map_step and per stage (vslam_prof_*), features resident
  python tools/map_bench.py --what total     vslam_track_sequences against vslam_frontend_sequence over the same frames
  python tools/map_bench.py --what host      the arrangement without the resident map: vslam_extract_Rt / vslam_associate_map_points /
                                             vslam_triangulate / vslam_reprojection_filter per step with the bookkeeping in numpy on
                                             the host, arrays copied each step
Shape: --tracks 256 --frames 8 at 1280x720 / 2000 keypoints / 4096 hypotheses (--tracks 1: the latency of a single video).
One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("step", "total", "host"), default="step")
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--hyp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from vslam_amd import Context, capi, synth
    T, Fr, w, h, Kp = a.tracks, a.frames, a.width, a.height, a.keypoints
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    ca, sa = synth.keypoint_rotation()
    K = np.array([[525.0, 0, w // 2], [0, 525.0, h // 2], [0, 0, 1]], np.float32)
    bgr = synth.sequences_torch(0x5EED, T, Fr, w, h, dev)
    seeds = torch.arange(T * (Fr - 1), dtype=torch.int32, device=dev).reshape(T, Fr - 1).contiguous()
    pmap = capi.PointMap(ctx, T, Fr, Kp, Fr * Kp, 4 * Fr * Kp)
    out = ctx.track_sequences(pmap, bgr, Kp, ca, sa, None, seeds, a.hyp, 10.0, K)
    ctx.synchronize()
    res = {"what": a.what, "tracks": T, "frames": Fr, "shape": [w, h, Kp, a.hyp],
           "map_points_per_track": float(pmap.view()["sizes"].mean()), "observations_per_track": float(pmap.view()["n_obs"].mean())}

    def batches(f):
        fr = {k: out[k].view(T, Fr, *out[k].shape[1:])[:, f].contiguous() for k in ("xy", "desc", "nodes", "n")}
        if f == 0:
            return fr, None
        pr = {}
        for k in ("matches", "best", "F"):
            full = torch.cat([out[k], torch.zeros_like(out[k][:1])])
            pr[k] = full.view(T, Fr, *out[k].shape[1:])[:, f - 1].contiguous()
        return fr, pr

    per = [batches(f) for f in range(Fr)]
    imgs = [bgr[:, f].contiguous() for f in range(Fr)]
    torch.cuda.synchronize(dev)

    def steps():
        pmap.reset()
        for f in range(1, Fr):
            pmap.step(per[f - 1][0], per[f][0], per[f][1], imgs[f], K)

    def timed(fn):
        fn(); ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    if a.what == "step":
        res["ms_per_map_step"] = timed(steps) / (Fr - 1)
        ctx.prof_enable(True); ctx.prof_reset()
        steps()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        res["ms_per_step_by_stage"] = {k: round(v[0] / (Fr - 1), 4) for k, v in rep.items() if v[1] > 0}
    elif a.what == "total":
        flat = bgr.view(T * Fr, h, w, 3)
        fseeds = torch.zeros(T * Fr - 1, dtype=torch.int32, device=dev)
        fo = ctx.frontend_sequence(flat, Kp, ca, sa, None, fseeds, a.hyp, 10.0)
        res["ms_track_sequences"] = timed(lambda: ctx.track_sequences(pmap, bgr, Kp, ca, sa, None, seeds, a.hyp, 10.0, K, out=out))
        res["ms_frontend_sequence"] = timed(lambda: ctx.frontend_sequence(flat, Kp, ca, sa, None, fseeds, a.hyp, 10.0, out=fo))
        res["ms_map_adds"] = res["ms_track_sequences"] - res["ms_frontend_sequence"]
    else:
        res["ms_per_step_host_bookkeeping"] = timed(lambda: host_steps(ctx, torch, np, per, imgs, K, T, Fr, Kp, w, h)) / (Fr - 1)
    print(json.dumps(res))
    pmap.close()
    ctx.close()


def host_steps(ctx, torch, np, per, imgs, K, T, Fr, Kp, w, h):
    """The loop with the existing per-pair entry points and the map kept in numpy on the host: per step the matches, claims,
    inlier lists, triangulated points and descriptors come down, the CSR arrays and ids go up."""
    dev = per[0][0]["xy"].device
    M = Fr * Kp
    pts = np.zeros((T, M, 4), np.float32); size = np.zeros(T, np.int32)
    obs = [[[] for _ in range(M)] for _ in range(T)]                 # per map point: descriptor rows
    last_ids = np.full((T, Kp), -1, np.int32)
    for f in range(1, Fr):
        cur, pr = per[f]
        lastf = per[f - 1][0]
        R, t, c2 = ctx.extract_Rt(pr["F"], pr["best"], K)
        matches = pr["matches"].cpu().numpy(); nm = pr["best"][:, 3].cpu().numpy()
        desc = cur["desc"].cpu().numpy(); desc_last = lastf["desc"].cpu().numpy()
        ids = np.full((T, Kp), -1, np.int32)
        for b in range(T):
            for k in range(nm[b]):
                first, second = matches[b, k]
                i = last_ids[b, first]
                if i > 0:
                    ids[b, second] = i
                    obs[b][i].append(desc[b, second])
        offs = np.zeros((T, M + 1), np.int32)
        total = max(1, max(sum(len(o) for o in obs[b][:size[b]]) for b in range(T)))
        od = np.zeros((T, total, 32), np.uint8)
        for b in range(T):
            n = 0
            for i in range(size[b]):
                for row in obs[b][i]:
                    od[b, n] = row; n += 1
                offs[b, i + 1] = n
        d_ids = torch.from_numpy(ids).to(dev)
        claim = ctx.associate(torch.from_numpy(pts).to(dev), torch.from_numpy(size).to(dev), c2, w, h, cur["nodes"], cur["xy"],
                              cur["desc"], cur["n"], torch.from_numpy(offs).to(dev), torch.from_numpy(od).to(dev), d_ids)
        p4 = ctx.triangulate(lastf["xy"], cur["xy"], pr["matches"], pr["best"], K, c2)
        idx, n_in, _ = ctx.reprojection_filter(p4, lastf["xy"], cur["xy"], pr["matches"], pr["best"], K, c2, d_ids)
        ctx.synchronize()
        claim = claim.cpu().numpy(); p4 = p4.cpu().numpy(); idx = idx.cpu().numpy(); n_in = n_in.cpu().numpy()
        for b in range(T):
            for i in np.nonzero(claim[b, :size[b]] >= 0)[0]:
                obs[b][i].append(desc[b, claim[b, i]])
            k = min(int(n_in[b]), M - size[b])
            rows = idx[b, :k]
            pts[b, size[b]:size[b] + k, :3] = p4[b, rows, :3]
            pts[b, size[b]:size[b] + k, 3] = 1
            for j, r in enumerate(rows):
                obs[b][size[b] + j] = [desc_last[b, matches[b, r, 0]], desc[b, matches[b, r, 1]]]
            size[b] += k
        last_ids = d_ids.cpu().numpy()


if __name__ == "__main__":
    main()
