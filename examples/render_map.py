#!/usr/bin/env python3
"""A video of the map growing, without a window: the synthetic sequences of examples/track_sequences.py are extracted and
matched once on the device, then the map is advanced one frame at a time (vslam_map_step) and after EVERY step every track's
map is drawn on the device (vslam_map_render: the points in their colours, one wire frustum per frame so far) and written as a
binary PPM.  What the reference shows in its Pangolin window (src/display.cpp), headless.

    python examples/render_map.py [--world [--resect] [--fuse [--project] [--cull] [--retriangulate]] [--adjust] [--search] [--relocalise]] [output directory]

--world: the map also gets a world frame (vslam_map_attach_world) and every image is twice as wide: on the left what the
reference's window shows -- every pair's points in the last frame's camera and in the pair's own unit, stacked at the origin --
and on the right the same points and frusta in one coordinate system (vslam_world_render), seen from the same viewpoint.
--resect (with --world): every frame's pose is resected against the world's points (include/vslam_resect.h) instead of being
chained from the pair's fundamental matrix alone; the accepted steps and participants per pair are printed.
--fuse (with --world): after the last step, before anything else, the map points that share an observation are fused into tracks
(World.fuse, include/vslam_fuse.h) and, with --cull, the points their observations do not support are culled (World.cull, at its
untuned defaults); the world is drawn before and after (track*_before_fuse.ppm / track*_after_fuse.ppm) and the counts are printed.
--adjust, --search and --relocalise then read the merged observation lists.
--project (with --fuse, behind it and ahead of --cull): the geometric round (World.fuse_project, include/vslam_fuse_project.h, at the
search's untuned defaults): every world point is searched by projection in the frames that do not see it yet, the found pairs join
the world's extra log and the fusion runs over the lists with them; the world is drawn before and after
(track*_before_project.ppm / track*_after_project.ppm) and the counts are printed.
--retriangulate (with --fuse, behind it and --cull): every world point is triangulated anew from ALL the observations of its merged
row (World.retriangulate, include/vslam_tracks.h, at its untuned defaults); the world is drawn before and after
(track*_before_retriangulate.ppm / track*_after_retriangulate.ppm) and the counts per status are printed.
--adjust (with --world): after the last step the last window of 8 frames and the points they observe are adjusted together
(World.adjust, include/vslam_adjust.h) and the world is drawn once more: track*_before_adjust.ppm / track*_after_adjust.ppm.
--search (with --world): after the last step (and after --adjust) the last frame is searched by projection against the WHOLE map
of its track and resected against what was found (World.search, include/vslam_search.h); found / seen per track are printed,
beside the links the step itself had.
--relocalise (with --world, last of all): the recorded pose of the last frame is dropped to the identity, as if the track had been
lost, and found again from the map alone (World.relocalise, include/vslam_pnp.h: descriptor match without a pose, P3P RANSAC,
polish, write-back); the world is drawn with the dropped pose and with the one that came back (track*_before_relocalise.ppm /
track*_after_relocalise.ppm) and matches / inliers / found per track are printed.  inlier_px 4 and 1024 hypotheses: on these
synthetic tracks the defaults (2 px, 128) do not find every track; nothing here is tuned.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vslam_amd import Context, capi, synth  # noqa: E402


def write_ppm(path, bgr):
    """bgr: (H, W, 3) uint8 numpy, written as a binary P6 (which is RGB)."""
    h, w, _ = bgr.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(bgr[..., ::-1]).tobytes())


def main():
    args = [a for a in sys.argv[1:] if a not in ("--world", "--resect", "--fuse", "--project", "--cull", "--retriangulate", "--adjust", "--search", "--relocalise")]
    with_world = "--world" in sys.argv[1:]
    resect = "--resect" in sys.argv[1:]
    adjust = "--adjust" in sys.argv[1:]
    search = "--search" in sys.argv[1:]
    relocalise = "--relocalise" in sys.argv[1:]
    fuse = "--fuse" in sys.argv[1:]
    cull = "--cull" in sys.argv[1:]
    project = "--project" in sys.argv[1:]
    retri = "--retriangulate" in sys.argv[1:]
    if (resect or adjust or search or relocalise or fuse) and not with_world:
        sys.exit("--resect, --fuse, --adjust, --search and --relocalise need --world")
    if (cull or retri or project) and not fuse:
        sys.exit("--project, --cull and --retriangulate need --fuse")
    out_dir = args[0] if args else "render_map_out"
    os.makedirs(out_dir, exist_ok=True)
    tracks, frames, width, height, max_corners, hyp = 4, 8, 640, 480, 1000, 512
    W, H = 640, 480                                              # of the view
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    cos_a, sin_a = synth.keypoint_rotation()
    K = np.array([[525.0, 0, width // 2], [0, 525.0, height // 2], [0, 0, 1]], np.float32)   # src/vslam.cpp:32
    bgr = synth.sequences_torch(7, tracks, frames, width, height, dev)
    seeds = torch.arange(tracks * (frames - 1), dtype=torch.int32, device=dev).reshape(tracks, frames - 1).contiguous()
    pmap = capi.PointMap(ctx, tracks, frames, max_corners, map_capacity=frames * max_corners, obs_capacity=4 * frames * max_corners)
    world = pmap.attach_world(resection={} if resect else None) if with_world else None
    # features and matches of every frame and consecutive pair, once (this also runs the whole loop; the map is then rebuilt
    # step by step below so that it can be looked at after every step)
    out = ctx.track_sequences(pmap, bgr, max_corners, cos_a, sin_a, None, seeds, hyp, 10.0, K)
    ctx.synchronize()
    done = pmap.view()
    pts = np.concatenate([done["points"][t, :done["sizes"][t], :3] for t in range(tracks)]).astype(np.float64)
    med = np.median(pts, axis=0)
    spread = float(np.median(np.abs(pts - med))) + 1.0
    eye = -2.0 * spread * med / (np.linalg.norm(med) + 1e-9) + np.array([0.4 * spread, -0.6 * spread, 0.0])
    view = capi.View.look_at(eye, med, (0, -1, 0), W, H, fu=0.6 * W, fv=0.6 * W, z_near=0.05, z_far=1e6, point_size=3)

    def per_frame(a, f):
        return a.view(tracks, frames, *a.shape[1:])[:, f].contiguous()

    def per_pair(a, f):
        full = torch.cat([a, torch.zeros_like(a[:1])])           # tracks * frames - 1 slots -> tracks * frames
        return full.view(tracks, frames, *a.shape[1:])[:, f - 1].contiguous()
    pmap.reset()
    images = torch.empty((tracks, H, W, 3), dtype=torch.uint8, device=dev)
    world_images = torch.empty((tracks, H, W, 3), dtype=torch.uint8, device=dev) if with_world else None
    last = {k: per_frame(out[k], 0) for k in ("xy", "desc", "nodes", "n")}
    for f in range(1, frames):
        cur = {k: per_frame(out[k], f) for k in ("xy", "desc", "nodes", "n")}
        pair = {k: per_pair(out[k], f) for k in ("matches", "best", "F")}
        pmap.step(last, cur, pair, bgr[:, f].contiguous(), K)
        pmap.render(view, W, H, out=(images, None))              # stream-ordered behind the step: no wait in between
        if with_world:
            world.render(pmap, view, W, H, out=(world_images, None))
        ctx.synchronize()
        host = torch.cat([images, world_images], 2).cpu().numpy() if with_world else images.cpu().numpy()
        for t in range(tracks):
            write_ppm(os.path.join(out_dir, f"track{t}_step{f:02d}.ppm"), host[t])
        last = cur
    sizes = pmap.view()["sizes"]
    print(f"{tracks * (frames - 1)} images of {host.shape[2]} x {H} in {out_dir}/; map points per track: {[int(s) for s in sizes]}")
    if with_world:
        v = world.view()
        print("scale per pair, track 0:", [round(float(s), 4) for s in v["scale"][0, 1:]], "links:", v["links"][0, 1:].tolist())
        if resect:
            st = v["resect_stats"][0, 1:]
            print("resection, track 0: participants", [int(x) for x in st[:, 0]], "accepted steps",
                  [None if np.isnan(x) else int(x) for x in st[:, 3]])
        if fuse:
            world.render(pmap, view, W, H, out=(world_images, None))
            before = world_images.cpu().numpy()
            fs = world.fuse(pmap).cpu().numpy()
            if project:
                world.render(pmap, view, W, H, out=(world_images, None))
                fused = world_images.cpu().numpy()
                ps = world.fuse_project(pmap, out["xy"], out["desc"], out["n"], K, width, height).cpu().numpy()
                world.render(pmap, view, W, H, out=(world_images, None))
                ctx.synchronize()
                projected = world_images.cpu().numpy()
                for t in range(tracks):
                    write_ppm(os.path.join(out_dir, f"track{t}_before_project.ppm"), fused[t])
                    write_ppm(os.path.join(out_dir, f"track{t}_after_project.ppm"), projected[t])
                live = [int((world.view()["fuse_to"][t, :sizes[t]] == np.arange(sizes[t])).sum()) for t in range(tracks)]
                print("geometric round per track: pairs tried", ps[:, 0].tolist(), "found", ps[:, 3].tolist(), "of them links", ps[:, 4].tolist(),
                      "extras held", ps[:, 7].tolist(), "live points afterwards", live)
            cs = world.cull(pmap, out["xy"], K).cpu().numpy() if cull else None
            world.render(pmap, view, W, H, out=(world_images, None))
            ctx.synchronize()
            after = world_images.cpu().numpy()
            for t in range(tracks):
                write_ppm(os.path.join(out_dir, f"track{t}_before_fuse.ppm"), before[t])
                write_ppm(os.path.join(out_dir, f"track{t}_after_fuse.ppm"), after[t])
            print("fused per track: points", fs[:, 0].tolist(), "groups with more than one member", fs[:, 1].tolist(), "absorbed", fs[:, 2].tolist(),
                  "observations kept", fs[:, 3].tolist())
            if cull:
                print("culled per track: taking part", cs[:, 0].tolist(), "kept", cs[:, 1].tolist(), "culled", cs[:, 2].tolist())
        if retri:
            world.render(pmap, view, W, H, out=(world_images, None))
            before = world_images.cpu().numpy()
            status, ts = world.retriangulate(pmap, out["xy"], K)
            world.render(pmap, view, W, H, out=(world_images, None))
            ctx.synchronize()
            after, status, ts = world_images.cpu().numpy(), status.cpu().numpy(), ts.cpu().numpy()
            for t in range(tracks):
                write_ppm(os.path.join(out_dir, f"track{t}_before_retriangulate.ppm"), before[t])
                write_ppm(os.path.join(out_dir, f"track{t}_after_retriangulate.ppm"), after[t])
            print("retriangulated per track: taking part", ts[:, 0].tolist(), "moved (OK)", ts[:, 1].tolist(), "low parallax", ts[:, 2].tolist(),
                  "other refusals", ts[:, 3].tolist(), "; statuses 1 .. 6, track 0:", np.bincount(status[0][status[0] > 0], minlength=7)[1:].tolist())
        if adjust:
            world.render(pmap, view, W, H, out=(world_images, None))
            before = world_images.cpu().numpy()
            st = world.adjust(pmap, out["xy"], K, window=8).cpu().numpy()
            world.render(pmap, view, W, H, out=(world_images, None))
            ctx.synchronize()
            after = world_images.cpu().numpy()
            for t in range(tracks):
                write_ppm(os.path.join(out_dir, f"track{t}_before_adjust.ppm"), before[t])
                write_ppm(os.path.join(out_dir, f"track{t}_after_adjust.ppm"), after[t])
            print("adjustment per track: participants", [int(x) for x in st[:, 0]], "mean rho", [round(float(x), 3) for x in st[:, 1]], "->",
                  [round(float(x), 3) for x in st[:, 2]], "accepted steps", [None if np.isnan(x) else int(x) for x in st[:, 3]])
        if search:
            got = world.search(pmap, last, K, width, height, resect={})
            ctx.synchronize()
            found, st = got["n_corr"].cpu().numpy(), got["stats"].cpu().numpy()
            seen = [int((last["xy"][t, :int(last["n"][t])].isfinite().all(1)).sum()) for t in range(tracks)]
            print("search by projection, last frame against the whole map: found / keypoints seen per track",
                  [f"{int(found[t])} / {seen[t]}" for t in range(tracks)], "(links of the last step:", v["links"][:, frames - 1].tolist(), ")")
            print("  resected against them: participants", [int(x) for x in st[:, 0]], "mean rho", [round(float(x), 3) for x in st[:, 1]], "->",
                  [round(float(x), 3) for x in st[:, 2]], "accepted steps", [None if np.isnan(x) else int(x) for x in st[:, 3]])
        if relocalise:
            C = capi.C
            a, f1 = world.arrays(), frames - 1
            recorded = world.view()["Twc"][:, f1].copy()
            eye4 = np.eye(4)
            for t in range(tracks):                              # the last frame's pose dropped to the identity
                for ptr, m in ((a.d_Twc + 8 * 16 * (t * frames + f1), eye4), (a.d_pose + 4 * 16 * (t * frames + f1), eye4.astype(np.float32))):
                    m = np.ascontiguousarray(m)
                    ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, C.c_void_p(ptr), C.c_void_p(m.ctypes.data), C.c_size_t(m.nbytes)))
            world.render(pmap, view, W, H, out=(world_images, None))
            before = world_images.cpu().numpy()
            got = world.relocalise(pmap, last, K, hypotheses=1024, inlier_px=4.0)
            world.render(pmap, view, W, H, out=(world_images, None))
            ctx.synchronize()
            after, back = world_images.cpu().numpy(), world.view()["Twc"][:, f1]
            for t in range(tracks):
                write_ppm(os.path.join(out_dir, f"track{t}_before_relocalise.ppm"), before[t])
                write_ppm(os.path.join(out_dir, f"track{t}_after_relocalise.ppm"), after[t])
            print("relocalised from the map alone: matches", got["n_corr"].cpu().numpy().tolist(), "inliers", got["n_inliers"].cpu().numpy().tolist(),
                  "found", got["found"].cpu().numpy().tolist())
            print("  camera centre, recorded -> relocalised, track 0:", [round(float(x), 3) for x in recorded[0, [3, 7, 11]]], "->",
                  [round(float(x), 3) for x in back[0, [3, 7, 11]]])
    pmap.close()
    if with_world:
        world.close()
    ctx.close()


if __name__ == "__main__":
    main()
