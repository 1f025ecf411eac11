"""The kernels of include/vslam_sim3.h in vslam_amd/csrc/sim3.hip compiled to assembly with the build's flags, as tests/test_pnp_lds.py
reads pnp.hip's: static LDS (every launch of sim3.hip passes 0 dynamic bytes) fits the 64 KB a launch gets without an opt-in, and the
count kernel, the hot path, keeps its two matrices and its count in registers -- no scratch (.amdhsa_private_segment_fixed_size 0)
-- with the LDS size DESIGN.md 5n states: a tile of 256 correspondences x ten f64 (20480 B) and the 4 x 64 partial counts (1024 B).
The table DESIGN.md 5n carries is printed.  Every symbol include/vslam_sim3.h declares is exported and is capi.SIM3_SYMBOLS.  CPU
only (hipcc cross-compiles)."""
import os
import re
import subprocess

LDS_WITHOUT_OPT_IN = 64 * 1024
COUNT_LDS = 256 * 10 * 8 + 4 * 64 * 4
KERNELS = ("sim3_solve_kernel", "sim3_count_kernel", "sim3_select_kernel", "sim3_refine_kernel")
NO_SCRATCH = ("sim3_count_kernel", "sim3_select_kernel")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S)}


def test_sim3_kernels_fit_the_lds_and_the_count_uses_no_scratch(tmp_path):
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert "sim3.hip" in build.SOURCES and "sim3_math.h" in build.HEADERS
    out = str(tmp_path / "sim3.s")
    subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get("sim3.hip", []) + ["--cuda-device-only", "-S", "-o", out, "sim3.hip"],
                   cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    blocks = kernel_blocks(asm)
    print("| kernel | VGPRs | AGPRs | SGPRs | LDS (B) | scratch (B) |")
    print("|---|---|---|---|---|---|")
    for name in KERNELS:
        mine = {sym: b for sym, b in blocks.items() if re.search(r"\d" + name, sym)}
        assert len(mine) == 1, (name, sorted(blocks))
        for sym, body in mine.items():
            static = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
            sgpr = int(re.search(r"\.amdhsa_next_free_sgpr\s+(\d+)", body).group(1))
            accum = int(re.search(r"\.amdhsa_accum_offset\s+(\d+)", body).group(1))
            print(f"| `{name}` | {min(vgpr, accum)} | {max(vgpr - accum, 0)} | {sgpr} | {static} | {scratch} |")
            assert static <= LDS_WITHOUT_OPT_IN
            if name in NO_SCRATCH:
                assert scratch == 0, name
            if name == "sim3_count_kernel":
                assert static == COUNT_LDS
                assert vgpr <= 128             # at least four waves per SIMD
                body_text = asm[asm.index(sym + ":"):]
                body_text = body_text[:body_text.index("s_endpgm")]
                assert "v_div_" not in body_text and "v_rcp_f64" not in body_text, "the count divides"
                assert "global_atomic" not in body_text and "scratch_" not in body_text


def test_header_symbols_are_exported_and_listed():
    from vslam_amd import build, capi
    build.build()
    lib = capi.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_sim3.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.SIM3_SYMBOLS)
    others = (set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS) | set(capi.SEARCH_SYMBOLS) | set(capi.PNP_SYMBOLS)
              | set(capi.FUSE_SYMBOLS) | set(capi.TRACK_SYMBOLS) | set(capi.PLACES_SYMBOLS))
    assert not set(names) & others
    for nm in names:
        assert hasattr(lib, nm), nm
    p = capi.Sim3Params.make(lib)
    assert (p.hypotheses, p.min_inliers, p.inlier_px) == (128, 8, 2.0)
    assert lib.vslam_sim3_params_default(capi.C.c_void_p(0)) == -1
