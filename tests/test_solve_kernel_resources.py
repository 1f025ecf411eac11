"""ransac_solve_kernel<false, 4>, the product's solve kernel, compiled to assembly as the library is built: what its descriptor
says about registers, spills, scratch and LDS.  The kernel keeps nothing of its common path in scratch memory only because of
how the code around its two rare calls is written (ransac_solve.hip: jacobi_cs_full, jacobi_null_row_private), which a
compiler's register allocator is free to undo; this holds the outcome.  CPU only (hipcc cross-compiles)."""
import os
import re
import subprocess
import tempfile

SOLVE = "ransac_solve_kernelILb0ELi4E"      # <SPLIT = false, WPE = 4> in the mangling


def resources(asm, name):
    """The metadata entry (a dict of its integer fields) of the one kernel whose symbol contains `name`."""
    entries = [e for e in asm.split("  - .agpr_count")[1:] if re.search(r"\.name:\s+\S*" + re.escape(name), e)]
    assert len(entries) == 1, (name, len(entries))
    return {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", entries[0], re.M)}


def test_resources_parser():
    asm = """amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 4608
    .name:           _ZN1a19ransac_solve_kernelILb0ELi4EEEvPKf
    .private_segment_fixed_size: 304
    .vgpr_count:     128
    .vgpr_spill_count: 0
  - .agpr_count:     0
    .group_segment_fixed_size: 0
    .name:           _ZN1a19ransac_solve_kernelILb1ELi5EEEvPKf
    .vgpr_spill_count: 281
"""
    r = resources(asm, SOLVE)
    assert r["group_segment_fixed_size"] == 4608 and r["private_segment_fixed_size"] == 304
    assert r["vgpr_count"] == 128 and r["vgpr_spill_count"] == 0


def test_solve_kernel_spills_nothing_and_keeps_its_occupancy():
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = "ransac_solve.hip"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "solve.s")
        cmd = [hipcc] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", "-o", out, src]
        subprocess.run(cmd, cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
        r = resources(open(out).read(), SOLVE)
    print(r)
    assert r["vgpr_count"] <= 128                       # four waves per SIMD
    assert r["group_segment_fixed_size"] <= 10240       # sixteen 64-thread workgroups per CU
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0
    # the private segment is the rare closing path's copy of the rows (72 floats) and its call frame, nothing else
    assert r["private_segment_fixed_size"] <= 72 * 4 + 64, r["private_segment_fixed_size"]
