"""The kernel of include/vslam_tracks.h (vslam_amd/csrc/tracks.hip) compiled to assembly with the build's flags: static LDS (no launch
of tracks.hip passes a dynamic size) within the 64 KB a launch gets without an opt-in, since the launcher sets no attribute, and no
scratch (.amdhsa_private_segment_fixed_size 0): a lane keeps its point's state in registers and forms everything per observation
afresh in every pass.  The kernel list is pinned.  Reads only that metadata.  CPU only (hipcc cross-compiles)."""
import os
import re
import subprocess

LDS_WITHOUT_OPT_IN = 64 * 1024
KERNELS = ("triangulate_tracks_kernel",)


def kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S)}


def test_track_kernels_fit_the_lds_and_use_no_scratch(tmp_path):
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert "tracks.hip" in build.SOURCES and "tracks_math.h" in build.HEADERS
    assert any(h.endswith("vslam_tracks.h") for h in build.HEADERS)
    out = str(tmp_path / "tracks.s")
    subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get("tracks.hip", []) + ["--cuda-device-only", "-S", "-o", out, "tracks.hip"],
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


def test_the_library_exports_the_header_symbols():
    from vslam_amd import build, capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(build.HERE), "include", "vslam_tracks.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.TRACK_SYMBOLS)
    lib = capi.load_library()
    for nm in names:
        assert hasattr(lib, nm), nm
