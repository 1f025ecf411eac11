"""The random scenes of the renderer's tests, shared by tests/test_ref_render.py (which asserts on the reference alone that they
are not trivial) and tests/test_gpu_render.py (which renders them on the device)."""
import numpy as np

import ref_render

# name -> (seed, width, height, point_size, row padding in bytes)
SCENES = {
    "320x240_s3": (11, 320, 240, 3, 0),
    "322x200_s1_padded": (12, 322, 200, 1, 10),
    "1277x96_s4_padded": (13, 1277, 96, 4, 10),
    "320x240_s15_padded": (14, 320, 240, 15, 10),
}
SIZES = [5000, 0, 1800, 3100]          # map points per track; the capacity is the largest
FRAMES, POSE_STRIDE = 6, 7
Z_FAR = 9.0


def _rigid(rng, spread):
    """A random rigid pose as a row-major 4 x 4 (16,) float32."""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = rng.uniform(-spread, spread, 3)
    return P.astype(np.float32).reshape(16)


def make(name):
    """dict(points (T, M, 4), colors (T, M, 3), sizes (T,), pose (T, POSE_STRIDE, 16), frames, view, width, height, pad)."""
    seed, width, height, point_size, pad = SCENES[name]
    rng = np.random.default_rng(seed)
    T, M = len(SIZES), max(SIZES)
    eye = np.array([0.3, -0.2, -5.0])
    view = ref_render.View(ref_render.look_at(eye, (0, 0, 0), (0, 1, 0)), 0.9 * width, 0.9 * width, width // 2, height // 2,
                           z_near=0.2, z_far=Z_FAR, point_size=point_size, flags=ref_render.FRUSTA)
    points = np.zeros((T, M, 4), np.float32)
    # placed in eye space, then taken to the world: a little wider than the view in x and y (squares straddle every edge),
    # deeper than z_far and reaching behind the eye
    ze = rng.uniform(-2.0, Z_FAR + 2.5, (T, M))
    reach = np.where(np.abs(ze) < 0.5, 0.5, ze)
    xe = rng.uniform(-1.12, 1.12, (T, M)) * (width / 2) / float(view.fu) * reach
    ye = rng.uniform(-1.12, 1.12, (T, M)) * (height / 2) / float(view.fv) * reach
    mv = view.mv.astype(np.float64).reshape(4, 4)
    world = (np.stack([xe, ye, ze], -1) - mv[:3, 3]) @ mv[:3, :3]          # R^T (e - t)
    points[..., :3] = world.astype(np.float32)
    points[..., 3] = rng.uniform(-3, 3, (T, M))                  # the stored w is ignored
    colors = rng.integers(0, 256, (T, M, 3), dtype=np.uint8)
    for t, n in enumerate(SIZES):
        if n == 0:
            continue
        # exact depth ties: duplicated points with different colours, the copy at a HIGHER and at a LOWER index
        src = rng.choice(n // 2, n // 10, replace=False)
        points[t, n // 2 + np.arange(n // 10)] = points[t, src]
        points[t, 7:27] = points[t, n - 40:n - 20]
        # not finite anywhere a coordinate can be
        bad = rng.choice(np.arange(n // 2 + n // 10, n - 40), 30, replace=False)
        points[t, bad[:10], rng.integers(0, 3, 10)] = np.nan
        points[t, bad[10:20], rng.integers(0, 3, 10)] = np.inf
        points[t, bad[20:], rng.integers(0, 3, 10)] = -np.inf
    pose = np.stack([np.stack([_rigid(rng, 2.5) for _ in range(POSE_STRIDE)]) for _ in range(T)])
    # a frustum around the viewer (its segments cross the near plane and leave the screen), one far behind, one beyond z_far
    pose[:, 2, 3::4][:, :3] = (eye + np.array([0.1, 0.05, 0.2])).astype(np.float32)
    pose[:, 3, 3::4][:, :3] = np.array([0, 0, -40], np.float32)
    pose[:, 4] = np.eye(4, dtype=np.float32).reshape(16)                              # looks away from the viewer ...
    pose[:, 4, 3::4][:, :3] = np.array([0, 0, Z_FAR - 5.1], np.float32)               # ... from just inside z_far: straddles it
    return dict(points=points, colors=colors, sizes=np.array(SIZES, np.int32), pose=pose, frames=FRAMES, view=view, width=width,
                height=height, pad=pad)
