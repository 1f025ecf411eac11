#!/usr/bin/env python3
"""Hot-loop census: what a kernel's basic blocks hold AS COMPILED, by instruction class.

    python tools/loop_census.py match.hip match_knn2_fp4_kernel            one kernel, every block of 8 instructions or more
    python tools/loop_census.py --product                                   the nine kernels of the product's step
    python tools/loop_census.py --min 1 ransac_solve.hip ransac_solve_kernelILb0ELi4E

A source is compiled to assembly exactly as vslam_amd/build.py compiles it into the library (FLAGS + EXTRA_FLAGS of that
file, device side only), the kernel whose symbol contains the given name is cut out and split into basic blocks (at
labels and behind branches), and for every block the instructions are counted by class:

    valu   vector ALU instructions (v_*, the matrix ones excepted)
    salu   scalar ALU and control (s_*, scalar loads excepted)
    lds    ds_*
    mem    global_ / flat_ / buffer_ / scratch_ and scalar loads
    mfma   v_mfma_* / v_smfmac_*
    self   idempotent vector instructions (max, min, and, or) whose source operands all are the destination register:
           `v_max_f32 vN, vN, vN` changes nothing but a signalling NaN -- the form in which the compiler quiets a
           loop-carried operand of fmaxf() / fminf() that it cannot prove to be no NaN
    dup    the same with another destination (`v_max_f32 vM, vN, vN`): a quieting copy
    cnd    v_cndmask_* (selects)

The census counts and classifies; it judges nothing.  What a loop's count should be is for the reader (and
tests/test_hot_loop_budget.py) to derive from the source.  CPU only: hipcc cross-compiles.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (source, part of the mangled symbol, name in the profiles): the kernels of one step of the product build
PRODUCT = [
    ("response.hip", "min_eigen_tiered_kernelILb1E", "min_eigen_tiered<true>"),
    ("ransac_solve.hip", "ransac_solve_kernelILb0ELi4E", "ransac_solve<false,4>"),
    ("blur.hip", "gaussian7_stream_kernel", "gaussian7_stream"),
    ("match.hip", "match_knn2_fp4_kernel", "match_knn2_fp4"),
    ("brief.hip", "rbrief_tile_kernel", "rbrief_tile"),
    ("ransac_prune.hip", "ransac_prune_mfma_kernel", "ransac_prune_mfma"),
    ("ransac_count.hip", "ransac_screen_kernel", "ransac_screen"),
    ("ransac_count.hip", "ransac_count_kernelILb1ELb0E", "ransac_count"),
    ("response.hip", "corner_exact_kernel", "corner_exact"),
]
CLASSES = ("valu", "salu", "lds", "mem", "mfma", "self", "dup", "cnd")
_IDEMPOTENT = re.compile(r"^v_(pk_)?(max|min|and|or)\d?_")
_LABEL = re.compile(r"^([.\w$]+):")
_ENDS_BLOCK = re.compile(r"^s_(cbranch|branch|setpc|swappc|endpgm|call)")


def compile_asm(src, extra=()):
    """The device-side assembly of one source of vslam_amd/csrc, built with the library's own flags."""
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "census.s")
        cmd = [hipcc] + build.FLAGS + list(extra) + build.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", "-o", out, src]
        subprocess.run(cmd, cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def function_body(asm, name):
    """(symbol, lines) of the one function whose symbol contains `name`: from its label to its .Lfunc_end."""
    lines = asm.splitlines()
    starts = [i for i, ln in enumerate(lines)
              if (m := _LABEL.match(ln)) and name in m.group(1) and not m.group(1).startswith(".")]
    assert len(starts) == 1, (name, [lines[i] for i in starts])
    end = next(i for i in range(starts[0] + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return _LABEL.match(lines[starts[0]]).group(1), lines[starts[0] + 1:end]


def instruction(line):
    """(mnemonic, [operands]) of an assembly line, or None for labels, directives, comments and blank lines."""
    text = line.split(";", 1)[0].strip()
    if not text or text.startswith(".") or _LABEL.match(text):
        return None
    parts = text.split(None, 1)
    ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
    return parts[0], ops


def classify(mnemonic, ops):
    """The classes (a subset of CLASSES) one instruction counts in."""
    if mnemonic.startswith(("v_mfma", "v_smfmac")):
        return ("mfma",)
    if mnemonic.startswith("v_"):
        out = ["valu"]
        if mnemonic.startswith("v_cndmask"):
            out.append("cnd")
        srcs = [o for o in ops[1:] if re.fullmatch(r"v\d+|v\[\d+:\d+\]", o)]
        if _IDEMPOTENT.match(mnemonic) and len(srcs) >= 2 and len(srcs) == len(ops) - 1 and len(set(srcs)) == 1:
            out.append("self" if srcs[0] == ops[0] else "dup")
        return tuple(out)
    if mnemonic.startswith("ds_"):
        return ("lds",)
    if mnemonic.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")):
        return ("mem",)
    if mnemonic.startswith("s_"):
        return ("salu",)
    return ()


def blocks(body):
    """The basic blocks of a function body: [{"label", "n", "loop", classes...}], in layout order.  A block starts at a label
    or behind a branch; "loop" says that a branch of the block goes to its own label or to one laid out before it."""
    out, seen = [], set()

    def fresh(label):
        b = {"label": label, "n": 0, "loop": False}
        b.update({c: 0 for c in CLASSES})
        out.append(b)
        return b

    cur = fresh("entry")
    seen.add("entry")
    for ln in body:
        m = _LABEL.match(ln.strip())
        if m:
            if cur is None or cur["n"]:
                cur = fresh(m.group(1))
            cur["label"] = m.group(1)   # (an empty block takes the label: two labels in a row name one block)
            seen.add(m.group(1))
            continue
        ins = instruction(ln)
        if ins is None:
            continue
        if cur is None:
            cur = fresh(out[-1]["label"] + "+")
        mnemonic, ops = ins
        cur["n"] += 1
        for c in classify(mnemonic, ops):
            cur[c] += 1
        if _ENDS_BLOCK.match(mnemonic):
            if ops and ops[-1] in seen:
                cur["loop"] = True
            cur = None
    return [b for b in out if b["n"]]


def totals(bl):
    t = {c: sum(b[c] for b in bl) for c in CLASSES}
    t["n"] = sum(b["n"] for b in bl)
    return t


def census(src, name, asm=None):
    symbol, body = function_body(asm if asm is not None else compile_asm(src), name)
    return symbol, blocks(body)


def format_census(title, symbol, bl, min_n=8):
    head = f"{'block':14s} {'n':>6s} " + " ".join(f"{c:>5s}" for c in CLASSES) + "  loop"
    rows = [f"== {title}  ({symbol})", head]
    for b in bl:
        if b["n"] >= min_n or b["mfma"] or b["self"] or b["dup"]:
            rows.append(f"{b['label']:14s} {b['n']:6d} " + " ".join(f"{b[c]:5d}" for c in CLASSES) + ("  *" if b["loop"] else ""))
    t = totals(bl)
    rows.append(f"{'total':14s} {t['n']:6d} " + " ".join(f"{t[c]:5d}" for c in CLASSES) + f"  blocks={len(bl)}")
    return "\n".join(rows)


def parse_totals(text, title):
    """The `total` row of one kernel's table in a census file (format_census above), as a dict.  The LAST table with that
    title counts when `title` occurs more than once; pass the text of one section to choose."""
    sect = text.split(f"== {title}  (")
    assert len(sect) >= 2, title
    row = next(ln for ln in sect[-1].splitlines() if ln.startswith("total "))
    f = row.split()
    return dict(zip(("n",) + CLASSES, (int(x) for x in f[1:2 + len(CLASSES)])))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--product", action="store_true", help="the nine kernels of the product's step")
    ap.add_argument("--min", type=int, default=8, help="leave out blocks with fewer instructions (default 8)")
    ap.add_argument("-D", action="append", default=[], help="a preprocessor definition, as for the experiments build")
    ap.add_argument("source", nargs="?")
    ap.add_argument("kernel", nargs="?")
    a = ap.parse_args()
    jobs = PRODUCT if a.product else [(a.source, a.kernel, a.kernel)]
    if not a.product and not (a.source and a.kernel):
        ap.error("a source and a kernel name, or --product")
    cache = {}
    for src, name, title in jobs:
        if src not in cache:
            cache[src] = compile_asm(src, ["-D" + d for d in a.D])
        symbol, bl = census(src, name, cache[src])
        print(format_census(title, symbol, bl, a.min))
        print()


if __name__ == "__main__":
    main()
