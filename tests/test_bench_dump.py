"""bench.py --dump-outputs: what the last timed step computed, written as float32 / float64 .npy files that two builds can be
compared with; and the plain run (no --full) that carries only the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs(P, K, rng):
    return dict(xy=rng.random((2 * P, K, 2), dtype=np.float32), desc=rng.integers(0, 256, (2 * P, K, 32), dtype=np.uint8),
                n=rng.integers(0, K, (2 * P,), dtype=np.int32), matches=rng.integers(-1, K, (P, K, 2), dtype=np.int32),
                F=rng.standard_normal((P, 9), dtype=np.float32), err=rng.random((P,)), table=np.arange(7, dtype=np.int32))


@pytest.mark.parametrize("limit", [10 ** 9, 400_000])
def test_dump_is_exact_bounded_and_the_same_sample_every_time(tmp_path, limit):
    P, K = 24, 100
    arrays = _outputs(P, K, np.random.default_rng(3))
    bench.dump_outputs(str(tmp_path / "a"), arrays, P, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), arrays, P, limit=limit)
    idx = np.load(tmp_path / "a" / "sample_pairs.npy").astype(np.int64)
    assert (len(idx) == P) == (limit > 10 ** 6) and len(idx) >= 1 and np.all(np.diff(idx) > 0)
    total = 0
    for name, a in arrays.items():
        d = np.load(tmp_path / "a" / (name + ".npy"))
        assert np.array_equal(d, np.load(tmp_path / "b" / (name + ".npy")))
        assert d.dtype == (np.float32 if a.dtype in (np.uint8, np.float32) else np.float64)
        rows = np.concatenate([idx, P + idx]) if a.shape[0] == 2 * P else idx if a.shape[0] == P else slice(None)
        assert np.array_equal(d, a[rows])
        if a.dtype == np.float32:   # bit for bit, not only equal in value
            assert np.array_equal(d.view(np.uint32), a[rows].view(np.uint32))
        total += d.nbytes
    assert total <= limit


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_the_last_one_computed(tmp_path):
    """No --full: the line holds the headline and nothing measured beside it, --steps is the number of timed steps, and the dump
    of the last step (one context, so every step ran on the same frames) is what the oracle computes on those frames."""
    import torch
    from vslam_amd import shard, synth
    P = 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", str(P),
                        "--in-flight", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "frame-pairs/s" and d["dtype"] == "u8/f32/f64"
    assert not {"parity_in_bench", "cpu_baseline", "roofline", "kernels", "in_flight_sweep", "other_workloads"} & set(d)
    assert np.array_equal(np.load(tmp_path / "sample_pairs.npy"), np.arange(P))
    out = {k: np.load(tmp_path / (k + ".npy")) for k in ("xy", "desc", "nodes", "n", "matches", "best", "F")}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    w, h, K, H, _ = bench.WORKLOADS["C3"]
    seed = 0x5EED0000 + bench.SEED_INDEX["C3"]
    bgr = synth.frames_torch_hard(seed, P, w, h, torch.device("cuda", 0)).cpu().numpy()
    gpu = {"n": out["n"].astype(np.int32), "best": out["best"].astype(np.int32), "matches": out["matches"].astype(np.int32), "F": out["F"]}
    _, parity = bench.oracle_on_frames(bgr[:P], bgr[P:], shard.pair_seeds(seed, 0, P), K, H, 10.0, gpu, 0, "dumped outputs")
    assert parity["bit_exact"], parity
