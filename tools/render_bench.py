"""What the device renderer costs (vslam_map_render), every configuration in a FRESH PROCESS (as tools/ab_proc.sh does: which
hardware queue a stream lands on depends on what the process created before it):
  python tools/render_bench.py                       all configurations -> profiles/render_bench.json
  python tools/render_bench.py --one T N S           one configuration (tracks, points per track, point size): one JSON line
Shape: 1280 x 720, 1 / 16 / 256 tracks, 10^4 / 10^6 points per track, point sizes 1 and 3, 64 frames of frusta.
Per configuration: ms per render from HIP events around `reps` renders after warm-up, ms per kernel from vslam_prof_*, and the
point kernel's achieved 64-bit atomic-min updates per second (updates counted on the host from the same projection)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
W, H, FRAMES = 1280, 720, 64
CONFIGS = [(t, n, s) for t in (1, 16, 256) for n in (10 ** 4, 10 ** 6) for s in (1, 3)]


def one(T, N, S, reps):
    import ctypes as C
    import numpy as np
    import torch
    from vslam_amd import Context, capi
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    KP = 8
    pmap = capi.PointMap(ctx, T, FRAMES, KP, N, 1)
    # 63 steps without a RANSAC winner: the map stays empty, the frame counter reaches 64 (poses are written below)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    fr = dict(xy=z((T, KP, 2), torch.float32), desc=z((T, KP, 32), torch.uint8), nodes=z((T, KP), torch.int32), n=z((T,), torch.int32))
    pair = dict(matches=z((T, KP, 2), torch.int32), best=torch.full((T, 4), -1, dtype=torch.int32, device=dev), F=z((T, 9), torch.float32))
    img = z((T, 8, 8, 3), torch.uint8)
    K = np.eye(3, dtype=np.float32)
    for _ in range(FRAMES - 1):
        pmap.step(fr, fr, pair, img, K)
    ctx.synchronize()
    a = pmap.arrays()
    assert a.frames == FRAMES
    rng = np.random.default_rng(1)
    view = capi.View.look_at((0, 0, -6), (0, 0, 0), (0, -1, 0), W, H, fu=900.0, fv=900.0, point_size=S)
    mv = np.array(list(view.mv), np.float64).reshape(4, 4)
    ze = rng.uniform(1.0, 50.0, N)
    xe = rng.uniform(-1, 1, N) * (W / 2) / 900.0 * ze
    ye = rng.uniform(-1, 1, N) * (H / 2) / 900.0 * ze
    pts = np.ones((N, 4), np.float32)
    pts[:, :3] = ((np.stack([xe, ye, ze], -1) - mv[:3, 3]) @ mv[:3, :3]).astype(np.float32)
    cols = rng.integers(0, 256, (N, 3), dtype=np.uint8)
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(16), (FRAMES, 1))
    poses[:, 3:12:4] = rng.uniform(-3, 3, (FRAMES, 3)).astype(np.float32)
    sizes = np.full(T, N, np.int32)

    def h2d(ptr, arr):
        ctx._check(ctx.lib.vslam_copy_h2d(ctx.handle, C.c_void_p(ptr), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)))
    for t in range(T):
        h2d(a.d_points + t * N * 16, pts)
        h2d(a.d_colors + t * N * 3, cols)
        h2d(a.d_pose + t * FRAMES * 64, poses)
    h2d(a.d_sizes, sizes)
    # atomic updates of the point kernel: the clipped square of every drawn point, from the same float64 projection
    P = pts[:, :3].astype(np.float64)
    mv32 = np.array(list(view.mv), np.float32).astype(np.float64)
    e = [((mv32[4 * i] * P[:, 0] + mv32[4 * i + 1] * P[:, 1]) + mv32[4 * i + 2] * P[:, 2]) + mv32[4 * i + 3] for i in range(3)]
    ok = (e[2] >= view.z_near) & (e[2] <= view.z_far)
    px = np.floor(900.0 * e[0] / e[2] + view.u0)
    py = np.floor(900.0 * e[1] / e[2] + view.v0)
    lo, hi = (S - 1) // 2, S // 2
    nx = np.clip(np.minimum(px + hi, W - 1) - np.maximum(px - lo, 0) + 1, 0, None)
    ny = np.clip(np.minimum(py + hi, H - 1) - np.maximum(py - lo, 0) + 1, 0, None)
    updates = int((nx * ny)[ok].sum()) * T
    out = (torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev), None)
    for _ in range(3):
        pmap.render(view, W, H, out=out)
    ctx.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        pmap.render(view, W, H, out=out)
    stop.record()
    stop.synchronize()
    ms = start.elapsed_time(stop) / reps
    ctx.prof_enable(True); ctx.prof_reset()
    for _ in range(reps):
        pmap.render(view, W, H, out=out)
    rep = ctx.prof_report()
    ctx.prof_enable(False)
    kernels = {k: round(v[0] / v[1], 5) for k, v in rep.items() if v[1] > 0}
    pk = kernels.get("render_points_kernel", 0.0)
    res = dict(tracks=T, points_per_track=N, point_size=S, frames=FRAMES, width=W, height=H, reps=reps, ms_per_render=round(ms, 5),
               ms_per_kernel=kernels, point_atomic_updates=updates,
               point_atomic_updates_per_s=(updates / (pk * 1e-3) if pk > 0 else None),
               covered_pixels_track0=int((out[0][0] != 0).any(-1).sum().item()))
    print(json.dumps(res))
    pmap.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, type=int, metavar=("TRACKS", "POINTS", "SIZE"))
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args()
    if a.one:
        T, N, S = a.one
        one(T, N, S, a.reps or (5 if T * N >= 10 ** 7 else 20))
        return
    results = []
    for T, N, S in CONFIGS:
        # a fresh process per configuration; a configuration that fails or hangs ends the run (nothing more is started)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(T), str(N), str(S)], capture_output=True, text=True,
                           timeout=240)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"configuration {(T, N, S)} failed with status {p.returncode}")
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/render_bench.py", note="one fresh process per configuration; ms from HIP events after 3 warm-up "
                           "renders; per-kernel ms from vslam_prof_*; updates = 64-bit atomic-min operations of render_points_kernel",
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
