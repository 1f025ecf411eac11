"""The search and match kernels (vslam_amd/csrc/search.hip) compiled to assembly with the build's flags: static LDS plus the largest dynamic
size a launch asks for (none: every launch of search.hip passes 0) fits gfx950's 160 KB per workgroup -- and the 64 KB a launch
gets without an opt-in, since the launcher sets no attribute --, and no kernel uses scratch (.amdhsa_private_segment_fixed_size 0).
CPU only (hipcc cross-compiles)."""
import os
import re
import subprocess

LDS_PER_WORKGROUP = 160 * 1024
LDS_WITHOUT_OPT_IN = 64 * 1024
KERNELS = {"search_propose_kernel": 0, "match_propose_kernel": 0, "corr_resolve_kernel": 0, "world_search_pose_kernel": 0,
           "world_search_writeback_kernel": 0}
MAX_KP = 16384


def kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S)}


def test_search_kernels_fit_the_lds_and_use_no_scratch(tmp_path):
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert "search.hip" in build.SOURCES and "search_math.h" in build.HEADERS
    out = str(tmp_path / "search.s")
    subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get("search.hip", []) + ["--cuda-device-only", "-S", "-o", out, "search.hip"],
                   cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
    blocks = kernel_blocks(open(out).read())
    for name, dynamic in KERNELS.items():
        mine = {sym: b for sym, b in blocks.items() if re.search(r"\d" + name, sym)}
        assert len(mine) == 1, (name, sorted(blocks))
        for sym, body in mine.items():
            static = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
            print(f"{sym}: static LDS {static} + dynamic {dynamic}, scratch {scratch}, next free vgpr {vgpr}")
            assert static + dynamic <= LDS_PER_WORKGROUP and static + dynamic <= LDS_WITHOUT_OPT_IN
            assert scratch == 0
            if name == "match_propose_kernel":
                assert static >= 1024 * 32     # a tile of keypoint descriptors; VSLAM_MAX_KP x 32 B would not fit, so the tile loop is real
                assert 16384 * 32 > LDS_PER_WORKGROUP
    # the grid's worst case: a uint16 per keypoint slot and a word per cell (64 x 64), under 64 KB
    propose = next(b for sym, b in blocks.items() if "search_propose_kernel" in sym)
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", propose).group(1)) >= 2 * MAX_KP + 4 * 4096
