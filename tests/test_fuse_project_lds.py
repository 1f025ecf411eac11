"""The kernels of include/vslam_fuse_project.h in vslam_amd/csrc/fuse_project.hip compiled to assembly with the build's flags, as
tests/test_graph_lds.py reads graph.hip's: every kernel of the file is listed here, its static LDS (every launch of fuse_project.hip
passes 0 dynamic bytes) fits the 64 KB a launch gets without an opt-in -- the proposals keep the grid of one camera's keypoints there,
16 KB of cell ends and 32 KB of uint16 indices --, and none uses scratch.  The table DESIGN.md 5p carries is printed.  Every symbol
include/vslam_fuse_project.h declares is exported, is capi.FUSE_PROJECT_SYMBOLS and is in no other list.  CPU only (hipcc
cross-compiles)."""
import os
import re
import subprocess

LDS_WITHOUT_OPT_IN = 64 * 1024
KERNELS = ("fuse_project_holders_kernel", "fuse_project_propose_kernel", "fuse_project_count_kernel", "fuse_project_fill_kernel",
           "fuse_project_frames_kernel", "fuse_project_append_kernel", "fuse_project_merge_kernel", "fuse_project_gather_desc_kernel")
PROPOSE_LDS = 4096 * 4 + 16384 * 2 + 4 * 4   # the cells' ends, the keypoint indices, the scan
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S)}


def test_fuse_project_kernels_fit_the_lds_without_an_opt_in_and_use_no_scratch(tmp_path):
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert "fuse_project.hip" in build.SOURCES and "fuse_project_math.h" in build.HEADERS
    assert any(h.endswith("vslam_fuse_project.h") for h in build.HEADERS)
    out = str(tmp_path / "fuse_project.s")
    subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get("fuse_project.hip", []) + ["--cuda-device-only", "-S", "-o", out, "fuse_project.hip"],
                   cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
    blocks = kernel_blocks(open(out).read())
    assert len(blocks) == len(KERNELS), sorted(blocks)   # every kernel of the file is looked at
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
            assert static <= LDS_WITHOUT_OPT_IN, name
            assert scratch == 0, name
            if name == "fuse_project_propose_kernel":
                assert static <= PROPOSE_LDS


def test_header_symbols_are_exported_and_listed():
    from vslam_amd import build, capi
    build.build()
    lib = capi.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_fuse_project.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.FUSE_PROJECT_SYMBOLS)
    others = (set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS) | set(capi.SEARCH_SYMBOLS) | set(capi.PNP_SYMBOLS)
              | set(capi.SIM3_SYMBOLS) | set(capi.GRAPH_SYMBOLS) | set(capi.FUSE_SYMBOLS) | set(capi.TRACK_SYMBOLS) | set(capi.PLACES_SYMBOLS))
    assert not set(names) & others
    for nm in names:
        assert hasattr(lib, nm), nm
    null = capi.C.c_void_p(0)
    assert lib.vslam_fuse_project(*[null] * 3, 1, *[null] * 4, 1, *[null] * 3, 1, *[null] * 3, 1, null, null, 8, 8, 1, null, *[null] * 5, 1, null,
                                  null) == -1   # no context
    assert lib.vslam_world_fuse_project_view(null, *[null] * 6) == -1
