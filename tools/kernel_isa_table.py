#!/usr/bin/env python3
"""Table of every kernel's device assembly (lines, hash), to show that a change moved code and did not change it.

  python tools/kernel_isa_table.py                         # table of this tree, both builds, to stdout
  python tools/kernel_isa_table.py --csrc OTHER/vslam_amd/csrc > before.txt
  python tools/kernel_isa_table.py --against before.txt    # adds the `equal` column; exit status 1 on any difference

Every csrc/*.hip is compiled to assembly with the build's own flags (build.FLAGS + build.EXTRA_FLAGS, --cuda-device-only -S),
once plain and once with -DVSLAM_EXPERIMENTS.  A kernel's text runs from its label to its .Lfunc_end, which includes the
.amdhsa_kernel descriptor (registers, LDS, scratch); `;` comments are dropped and .LBB<n>_ becomes .LBB_, because <n> is
the function's index in its file.  Kernels are keyed by symbol, not by file, so a kernel may change files.
"""
import argparse
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vslam_amd import build  # noqa: E402


def kernels_of(asm):
    """{symbol: normalised text} for every symbol that has an .amdhsa_kernel descriptor."""
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        m = re.search(r"^" + re.escape(sym) + r":.*?^\.Lfunc_end\d+:", asm, re.M | re.S)
        lines = [re.sub(r"\s*;.*", "", ln).rstrip() for ln in m.group(0).splitlines()[:-1]]
        out[sym] = re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(ln for ln in lines if ln.strip()))
    return out


def table(csrc):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rows = {}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        def one(job):
            tag, extra, src = job
            out = os.path.join(tmp, tag + "_" + src + ".s")
            subprocess.run([hipcc] + build.FLAGS + extra + build.EXTRA_FLAGS.get(src, []) +
                           ["--cuda-device-only", "-S", "-o", out, src], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
            with open(out) as f:
                return tag, src, kernels_of(f.read())
        srcs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")))
        jobs = [(tag, extra, s) for tag, extra in (("product", []), ("experiments", ["-DVSLAM_EXPERIMENTS"])) for s in srcs]
        for tag, src, ks in pool.map(one, jobs):
            for sym, text in ks.items():
                assert (tag, sym) not in rows, "kernel defined twice: " + sym
                rows[(tag, sym)] = (src, text.count("\n") + 1, hashlib.sha256(text.encode()).hexdigest()[:16])
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=build.CSRC, help="directory of .hip sources (default: this tree's)")
    ap.add_argument("--against", help="a table written by an earlier run, to compare with")
    args = ap.parse_args()
    rows = table(args.csrc)
    before = {}
    if args.against:
        for ln in open(args.against):
            f = ln.split()
            if len(f) >= 5 and f[0] in ("product", "experiments"):
                before[(f[0], f[1])] = (f[2], int(f[3]), f[4])
    bad = 0
    print("# build kernel file lines sha256[:16]" + (" file_before equal" if args.against else ""))
    for key in sorted(set(rows) | set(before)):
        src, n, h = rows.get(key, ("-", 0, "-"))
        line = "%s %s %s %d %s" % (key[0], key[1], src, n, h)
        if args.against:
            equal = key in rows and key in before and before[key][1:] == (n, h)
            bad += not equal
            line += " %s %s" % (before.get(key, ("-",))[0], "yes" if equal else "NO")
        print(line)
    if args.against:
        print("# %d kernels, %d differ" % (len(set(rows) | set(before)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
