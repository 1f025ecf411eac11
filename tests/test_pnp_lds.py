"""The kernels of include/vslam_pnp.h in vslam_amd/csrc/pnp.hip (the match's are search.hip's: tests/test_search_lds.py) compiled
to assembly with the build's flags: static LDS plus the largest dynamic size a launch asks for (none: every launch of pnp.hip
passes 0) fits gfx950's 160 KB per workgroup -- and the 64 KB
a launch gets without an opt-in, since the launcher sets no attribute --, and the count kernel, the hot path, keeps its pose and
its count in registers: no scratch (.amdhsa_private_segment_fixed_size 0).  Every symbol include/vslam_pnp.h declares is exported
and is capi.PNP_SYMBOLS.  CPU only (hipcc cross-compiles)."""
import os
import re
import subprocess

LDS_PER_WORKGROUP = 160 * 1024
LDS_WITHOUT_OPT_IN = 64 * 1024
KERNELS = {"pnp_solve_kernel": 0, "pnp_count_kernel": 0, "pnp_select_kernel": 0, "relocalise_mark_kernel": 0}
NO_SCRATCH = ("pnp_count_kernel", "pnp_select_kernel", "relocalise_mark_kernel")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S)}


def test_pnp_kernels_fit_the_lds_and_the_count_uses_no_scratch(tmp_path):
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert "pnp.hip" in build.SOURCES and "pnp_math.h" in build.HEADERS
    out = str(tmp_path / "pnp.s")
    subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get("pnp.hip", []) + ["--cuda-device-only", "-S", "-o", out, "pnp.hip"],
                   cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
    blocks = kernel_blocks(open(out).read())
    for name, dynamic in KERNELS.items():
        mine = {sym: b for sym, b in blocks.items() if re.search(r"\d" + name, sym)}
        assert len(mine) == 1, (name, sorted(blocks))
        for sym, body in mine.items():
            static = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
            accum = int(re.search(r"\.amdhsa_accum_offset\s+(\d+)", body).group(1))
            print(f"{sym}: static LDS {static} + dynamic {dynamic}, scratch {scratch}, VGPRs {min(vgpr, accum)}, AGPRs {max(vgpr - accum, 0)} "
                  f"(next free vgpr {vgpr}, accum offset {accum})")
            assert static + dynamic <= LDS_PER_WORKGROUP and static + dynamic <= LDS_WITHOUT_OPT_IN
            if name in NO_SCRATCH:
                assert scratch == 0, name
            if name == "pnp_count_kernel":
                assert static >= 256 * 40      # the tile of widened correspondences is staged in LDS
                assert vgpr <= 128             # at least four waves per SIMD


def test_header_symbols_are_exported_and_listed():
    from vslam_amd import build, capi
    build.build()
    lib = capi.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_pnp.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.PNP_SYMBOLS)
    assert not set(names) & (set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS) | set(capi.SEARCH_SYMBOLS))
    for nm in names:
        assert hasattr(lib, nm), nm
    p = capi.PnpParams.make(lib)
    assert (p.hypotheses, p.min_inliers, p.inlier_px) == (128, 8, 2.0)
    assert lib.vslam_pnp_params_default(capi.C.c_void_p(0)) == -1
