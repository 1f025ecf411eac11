#!/usr/bin/env python3
"""vslam_prof_* readings of place recognition (include/vslam_places.h), one fresh process per configuration (children of this one,
which never opens the device itself), the library's per-kernel event timing after a warm-up call, `--reps` calls each:

  assign   256 frames x 2000 descriptors against 1024 / 4096 / 16384 words (places_spread_kernel + places_assign_kernel), and beside it
           the matcher on 256 pairs of 2000 x 2000 (the slot match_knn2_kernel: its spread and its knn kernel): the same arithmetic
           without a shared train side.  ns per (descriptor x word) of both, each with its spread, and their ratio.
  train    one k-majority round on 262144 descriptors x 4096 words, kernel by kernel
  query    256 frames of 2000 descriptors against an index of 1024 / 16384 entries (4096 words), kernel by kernel

Descriptors are uniform random bytes (torch's generator on the device): words then fill evenly and an entry has close to min(2000,
n_words) distinct words, the most work a row can be.

    python tools/places_prof.py [--reps 10] [--out profiles/places_prof.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, KP = 256, 2000
CONFIGS = ["assign:1024", "assign:4096", "assign:16384", "match:2000", "train:4096", "query:1024", "query:16384"]


def child(config, reps):
    import torch
    sys.path.insert(0, ROOT)
    from vslam_amd import Context, capi
    kind, size = config.split(":")
    size = int(size)
    ctx = Context(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def rand(*shape):
        return torch.randint(0, 256, shape + (32,), dtype=torch.uint8, device="cuda", generator=g)
    n = torch.full((FRAMES,), KP, dtype=torch.int32, device="cuda")
    desc = rand(FRAMES, KP)
    if kind == "assign":
        vocab = rand(size)
        out = ctx.places_assign(desc, n, vocab, want_dist=False)

        def call():
            ctx.places_assign(desc, n, vocab, out=out, want_dist=False)
        work = FRAMES * KP * size
    elif kind == "match":
        other = rand(FRAMES, KP)

        def call():
            ctx.match_knn2_ratio(desc, n, other, n)
        work = FRAMES * KP * KP
    elif kind == "train":
        rows = rand(262144)
        out = ctx.places_train(rows, size, 1)

        def call():
            ctx.places_train(rows, size, 1, out=out)
        work = 262144 * size
    else:
        idx = capi.Places(ctx, 4096, size, KP)
        idx.set_vocabulary(rand(4096))
        for _ in range(size // FRAMES):
            idx.add(rand(FRAMES, KP), n)
        out = idx.query(desc, n, 16)

        def call():
            idx.query(desc, n, 16, out=out)
        work = FRAMES * size
    call()                      # warm-up: the workspaces grow here
    ctx.synchronize()
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(reps):
        call()
    ctx.synchronize()
    rep = ctx.prof_report()
    ctx.prof_enable(False)
    ms = {k: round(t / reps, 5) for k, (t, cnt) in rep.items() if cnt > 0}
    print("PLACES_PROF " + json.dumps(dict(config=config, work=work, ms_per_call=ms, total_ms=round(sum(ms.values()), 5),
                                           device=torch.cuda.get_device_name(0))))
    ctx.close()


def derive(out):
    """ns per (descriptor x word) and the ratio to the matcher, like with like: the matcher's timing slot brackets its spread of the
    train rows AND its knn kernel, so the assignment's figure is its spread plus its assign kernel.  The assign kernel alone is kept
    beside it."""
    c = out["configs"]
    match_ns = c["match:2000"]["ms_per_call"]["match_knn2_kernel"] * 1e6 / c["match:2000"]["work"]
    out["match_ns_per_descriptor_word"] = round(match_ns, 7)
    for k in ("assign:1024", "assign:4096", "assign:16384"):
        ms = c[k]["ms_per_call"]
        ns = (ms["places_spread_kernel"] + ms["places_assign_kernel"]) * 1e6 / c[k]["work"]
        c[k]["ns_per_descriptor_word"] = round(ns, 7)
        c[k]["assign_kernel_alone_ns_per_descriptor_word"] = round(ms["places_assign_kernel"] * 1e6 / c[k]["work"], 7)
        c[k]["ratio_to_match"] = round(ns / match_ns, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    out = dict(frames=FRAMES, descriptors_per_frame=KP, reps=a.reps, readings="one reading per configuration", configs={})
    for config in CONFIGS:                                     # fresh processes, one at a time
        txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, "--reps", str(a.reps)], check=True,
                             stdout=subprocess.PIPE, text=True, timeout=300).stdout
        r = json.loads([l for l in txt.splitlines() if l.startswith("PLACES_PROF ")][-1][len("PLACES_PROF "):])
        out["device"] = r.pop("device")
        out["configs"][r.pop("config")] = r
    derive(out)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
