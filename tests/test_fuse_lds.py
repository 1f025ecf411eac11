"""The kernels of include/vslam_fuse.h (vslam_amd/csrc/fuse.hip) compiled to assembly with the build's flags: static LDS (no launch
of fuse.hip passes a dynamic size) within the 64 KB a launch gets without an opt-in, since the launchers set no attribute, and no
kernel uses scratch (.amdhsa_private_segment_fixed_size 0).  CPU only (hipcc cross-compiles)."""
import os
import re
import subprocess

LDS_WITHOUT_OPT_IN = 64 * 1024
KERNELS = ("fuse_points_kernel", "cull_points_kernel", "world_fuse_apply_kernel", "world_cull_apply_kernel", "world_cameras_kernel",
           "fuse_gather_desc_kernel", "fuse_identity_kernel")


def kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S)}


def test_fuse_kernels_fit_the_lds_and_use_no_scratch(tmp_path):
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert "fuse.hip" in build.SOURCES and "fuse_math.h" in build.HEADERS
    out = str(tmp_path / "fuse.s")
    subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get("fuse.hip", []) + ["--cuda-device-only", "-S", "-o", out, "fuse.hip"],
                   cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
    blocks = kernel_blocks(open(out).read())
    assert len(blocks) == len(KERNELS), sorted(blocks)
    for name in KERNELS:
        mine = {sym: b for sym, b in blocks.items() if re.search(r"\d" + name, sym)}
        assert len(mine) == 1, (name, sorted(blocks))
        for sym, body in mine.items():
            static = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1))
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
            print(f"{sym}: static LDS {static}, scratch {scratch}, next free vgpr {vgpr}")
            assert static <= LDS_WITHOUT_OPT_IN
            assert scratch == 0
