"""Inputs shared by the place-recognition tests (tests/test_ref_places.py, test_places_serial.py, test_gpu_places.py): random
descriptors with planted near-duplicates, awkward vocabularies, the 320 x 240 quality fixture, and
the serial host program of vslam_amd/csrc/places_math.h."""
import os
import struct
import subprocess

import numpy as np

import ref_places as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_desc(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (32,), dtype=np.uint8)


def flip_bits(rng, rows, p):
    """rows (k, 32) u8 with every bit flipped with probability p"""
    return rows ^ np.packbits(rng.random((len(rows), 256)) < p, axis=1)


def awkward_vocab(seed, n_words):
    """random words with what ties and extremes need: a duplicated word (the lower index must win), an all-zero and an all-one word"""
    v = random_desc(seed, (n_words,))
    if n_words >= 4:
        v[n_words - 1] = v[1]
        v[2] = 0
        v[n_words // 2] = 255
    return v


def frames_for(seed, vocab, frames, kp_stride, counts):
    """descriptors (frames, kp_stride, 32): random rows, near-duplicates of words (a few bits off), words themselves (distance 0) and
    complements of words (distance 256); n (frames,) = counts cycled"""
    rng = np.random.default_rng(seed)
    d = random_desc(seed + 1, (frames, kp_stride))
    W = len(vocab)
    for f in range(frames):
        k = kp_stride
        near = rng.integers(0, W, size=k)
        kind = rng.integers(0, 8, size=k)
        planted = flip_bits(rng, vocab[near], 0.04)
        d[f][kind >= 3] = planted[kind >= 3]
        d[f][kind == 6] = vocab[near][kind == 6]
        d[f][kind == 7] = ~vocab[near][kind == 7]
    n = np.array([counts[f % len(counts)] for f in range(frames)], np.int32)
    return d, n


def clustered(seed, n, centres, p=0.06):
    """n descriptors around `centres` random centres: what a training run can find"""
    rng = np.random.default_rng(seed)
    c = random_desc(seed + 7, (centres,))
    return flip_bits(rng, c[rng.integers(0, centres, size=n)], p)


# ---- the quality fixture: 16 pairs of 320 x 240 frames, 1000 corners; the "last" frames are the database, the "current" ones the queries
FIX_W, FIX_H, FIX_CORNERS, FIX_PAIRS, FIX_WORDS, FIX_ITERS = 320, 240, 1000, 16, 512, 4
FIX_TRAIN_SEED, FIX_TRAIN_PAIRS = 100, 8
FIX_MARGIN = 0.05


def fixture_frames(seed, pairs):
    from vslam_amd import synth
    return synth.frames_numpy(seed, pairs, FIX_W, FIX_H)


def pack_frames(descs, kp_stride=FIX_CORNERS):
    """a list of (k, 32) arrays -> (frames, kp_stride, 32) u8 zero-padded, n (frames,) i32"""
    d = np.zeros((len(descs), kp_stride, 32), np.uint8)
    n = np.zeros(len(descs), np.int32)
    for f, x in enumerate(descs):
        d[f, :len(x)] = x
        n[f] = len(x)
    return d, n


def oracle_descriptors(oracle, seed, pairs):
    from vslam_amd import synth
    ca, sa = synth.keypoint_rotation()
    pat = synth.brief_pattern()
    return pack_frames([oracle.extract_features(fr, FIX_CORNERS, ca, sa, pat)["desc"] for fr in fixture_frames(seed, pairs)])


def retrieval(best_id, best_score, best_den):
    """top-2 results (queries, 2) -> top-1 ids and the similarity margin of each query to its runner-up"""
    sim = np.where(best_den > 0, best_score / np.maximum(best_den, 1), 0.0)
    return best_id[:, 0], sim[:, 0] - sim[:, 1]


def reference_retrieval(vocab, desc, n, pairs):
    """index the first `pairs` frames, weights from places_weights, query the rest -> (ids, score, den, q_norm) of top_k = 2"""
    idx = rp.Index(len(vocab), pairs, desc.shape[1])
    idx.set_vocabulary(vocab)
    idx.add(desc[:pairs], n[:pairs])
    idx.set_weights(rp.places_weights(idx.df, idx.size))
    return idx, idx.query(desc[pairs:], n[pairs:], 2)


# ---- the serial host program (tests/native/places_serial.cpp)
def build_serial(tmpdir):
    out = os.path.join(str(tmpdir), "places_serial")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                    os.path.join(ROOT, "tests", "native", "places_serial.cpp")], check=True)
    return out


def _w(f, a, dt):
    f.write(np.ascontiguousarray(a, dt).tobytes())


def run_serial(exe, tmpdir, ops):
    """ops: a list of dicts, one program run each:
         dict(op="assign", desc (Fr, Kp, 32), n, vocab) -> word, dist
         dict(op="train", desc (n, 32), n_words, iterations) -> vocab, sizes
         dict(op="index", n_words, vocab, weights (or None), adds [(desc, n)], query_weights (or None), query (desc, n), top_k, below (or None))
           -> offsets, words, tf, df, norms, best_id, best_score, best_den, q_norm"""
    src, dst = os.path.join(str(tmpdir), "places_in.bin"), os.path.join(str(tmpdir), "places_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(ops)))
        for o in ops:
            if o["op"] == "assign":
                Fr, Kp = o["desc"].shape[:2]
                f.write(struct.pack("4i", 0, Fr, Kp, len(o["vocab"])))
                _w(f, o["desc"], np.uint8), _w(f, o["n"], np.int32), _w(f, o["vocab"], np.uint8)
            elif o["op"] == "train":
                f.write(struct.pack("4i", 1, len(o["desc"]), o["n_words"], o["iterations"]))
                _w(f, o["desc"], np.uint8)
            else:
                W = o["n_words"]
                qd, qn = o["query"]
                f.write(struct.pack("4i", 2, W, len(o["adds"]), o["top_k"]))
                _w(f, o["vocab"], np.uint8)
                for wts in (o.get("weights"), o.get("query_weights")):
                    f.write(struct.pack("i", wts is not None))
                    if wts is not None:
                        _w(f, wts, np.int32)
                for d, n in o["adds"]:
                    f.write(struct.pack("2i", d.shape[0], d.shape[1]))
                    _w(f, d, np.uint8), _w(f, n, np.int32)
                f.write(struct.pack("3i", qd.shape[0], qd.shape[1], o.get("below") is not None))
                _w(f, qd, np.uint8), _w(f, qn, np.int32)
                if o.get("below") is not None:
                    _w(f, o["below"], np.int32)
    subprocess.run([exe, src, dst], check=True)
    buf = open(dst, "rb").read()
    pos, out = 0, []

    def take(n, dt=np.int32):
        nonlocal pos
        a = np.frombuffer(buf, dt, n, pos)
        pos += a.nbytes
        return a
    for o in ops:
        if o["op"] == "assign":
            Fr, Kp = o["desc"].shape[:2]
            out.append(dict(word=take(Fr * Kp).reshape(Fr, Kp), dist=take(Fr * Kp).reshape(Fr, Kp)))
        elif o["op"] == "train":
            W = o["n_words"]
            out.append(dict(vocab=take(W * 32, np.uint8).reshape(W, 32), sizes=take(W)))
        else:
            size = int(take(1)[0])
            offsets = take(size + 1)
            nnz = int(offsets[size])
            Q, k = o["query"][0].shape[0], o["top_k"]
            out.append(dict(size=size, offsets=offsets, words=take(nnz), tf=take(nnz), df=take(o["n_words"]), norms=take(size),
                            best_id=take(Q * k).reshape(Q, k), best_score=take(Q * k).reshape(Q, k), best_den=take(Q * k).reshape(Q, k),
                            q_norm=take(Q)))
    assert pos == len(buf)
    return out
