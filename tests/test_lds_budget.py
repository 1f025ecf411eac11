"""Every kernel that is launched with dynamic LDS, compiled to assembly as the library is built: its static LDS
(.amdhsa_group_segment_fixed_size) plus the largest dynamic size the contract lets a launch ask for must fit gfx950's 160 KB
per workgroup.  The dynamic sizes are restated here from include/vslam_amd.h and the launchers; a static array added to one of
these kernels later cannot silently push a capacity-edge launch over the limit.  CPU only (hipcc cross-compiles)."""
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import kd_cases

LDS_PER_WORKGROUP = 160 * 1024
MAX_KP = kd_cases.VSLAM_MAX_KP

# source -> {kernel name as it appears in the mangled symbol: (largest dynamic LDS in bytes, how many instantiations at least)}
BUDGETS = {
    # 14 bytes per slot and 4 more, rounded up to 16, at kp_stride = VSLAM_KDTREE_MAX_KP; the 1024- and the 256-thread shape
    "kdtree.hip": {"kdtree_build_kernel": ((14 * kd_cases.KDTREE_MAX_KP + 4 + 15) & ~15, 2)},
    "world.hip": {"world_step_kernel": (8 * MAX_KP, 1)},                        # a u64 key per match slot
    "select.hip": {"corner_select_kernel": (128 * 1024, 1)},                    # the launcher's fixed allowance
    "refine.hip": {"refine_pairs_kernel": (3200 * 49, 1)},                      # 3200 points x (6 f64 + a flag byte)
    "assoc.hip": {"assoc_resolve_kernel": (4 * (((MAX_KP + 31) // 32 + 1 & ~1) + MAX_KP), 1)},   # a bit and an owner word per slot
    "ransac_select.hip": {"ransac_tiesum_kernel": (4 * MAX_KP, 1)},             # a float per match slot
}


def static_lds(asm):
    """{mangled kernel symbol: .amdhsa_group_segment_fixed_size}"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        size = re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", m.group(2))
        assert size, m.group(1)
        out[m.group(1)] = int(size.group(1))
    return out


def test_static_lds_parser():
    asm = """
	.amdhsa_kernel _ZN12_GLOBAL__N_119kdtree_build_kernelILi1024ELi48EtEEvPKfPKiiPi
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_private_segment_fixed_size 0
	.end_amdhsa_kernel
	.amdhsa_kernel _Z1k
		.amdhsa_group_segment_fixed_size 1040
	.end_amdhsa_kernel
"""
    assert static_lds(asm) == {"_ZN12_GLOBAL__N_119kdtree_build_kernelILi1024ELi48EtEEvPKfPKiiPi": 0, "_Z1k": 1040}


def test_static_plus_largest_dynamic_lds_fits_the_workgroup():
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert set(BUDGETS) <= set(build.SOURCES)
    assert kd_cases.KDTREE_MAX_KP == 11666 and MAX_KP == 16384
    with tempfile.TemporaryDirectory() as tmp:
        def compile_s(src):
            out = os.path.join(tmp, src.replace(".hip", ".s"))
            cmd = [hipcc] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", "-o", out, src]
            subprocess.run(cmd, cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
            return open(out).read()
        with ThreadPoolExecutor(max_workers=4) as pool:
            asm = dict(zip(BUDGETS, pool.map(compile_s, BUDGETS)))
    for src, kernels in BUDGETS.items():
        sizes = static_lds(asm[src])
        for name, (dynamic, at_least) in kernels.items():
            mine = {sym: s for sym, s in sizes.items() if re.search(r"\d" + name, sym)}     # <length><name> in the mangling
            assert len(mine) >= at_least, (src, name, sorted(sizes))
            for sym, static in mine.items():
                print(f"{src} {sym}: static {static} + dynamic {dynamic} = {static + dynamic} of {LDS_PER_WORKGROUP}")
                assert static + dynamic <= LDS_PER_WORKGROUP, (sym, static, dynamic)
    shapes = [sym for sym in static_lds(asm["kdtree.hip"]) if "kdtree_build_kernel" in sym]
    assert any("ILi1024E" in s for s in shapes) and any("ILi256E" in s for s in shapes), shapes
