"""The kernels of include/vslam_graph.h in vslam_amd/csrc/graph.hip compiled to assembly with the build's flags, as
tests/test_sim3_lds.py reads sim3.hip's: every kernel's static LDS (every launch of graph.hip passes 0 dynamic bytes) fits the 64 KB
a launch gets without an opt-in -- the CG vectors stay in L2 --, and the optimiser, which keeps a node's 28 + 7 sums
in registers, uses no scratch.  The table DESIGN.md 5o carries is printed.  Every symbol include/vslam_graph.h declares is exported,
is capi.GRAPH_SYMBOLS and is in no other list.  CPU only (hipcc cross-compiles)."""
import os
import re
import subprocess

LDS_WITHOUT_OPT_IN = 64 * 1024
KERNELS = ("graph_optimize_kernel", "graph_world_gather_kernel", "graph_world_scatter_kernel")
OPTIMIZE_LDS = 4 * 8 + 4 * 4 + 2 * 256 * 4 + 256   # the reduction, the scan, the fill's two columns, __syncthreads_or's words
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S)}


def test_graph_kernels_fit_the_lds_without_an_opt_in(tmp_path):
    from vslam_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert "graph.hip" in build.SOURCES and "graph_math.h" in build.HEADERS
    assert any(h.endswith("vslam_graph.h") for h in build.HEADERS)
    out = str(tmp_path / "graph.s")
    subprocess.run([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get("graph.hip", []) + ["--cuda-device-only", "-S", "-o", out, "graph.hip"],
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
            if name == "graph_optimize_kernel":
                assert static <= OPTIMIZE_LDS
                assert vgpr <= 512   # one workgroup of four waves, a wave per SIMD


def test_header_symbols_are_exported_and_listed():
    from vslam_amd import build, capi
    build.build()
    lib = capi.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_graph.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(vslam_[A-Za-z0-9_]+)\s*\(", text)))
    assert names == sorted(capi.GRAPH_SYMBOLS)
    others = (set(capi.SYMBOLS) | set(capi.RESECT_SYMBOLS) | set(capi.ADJUST_SYMBOLS) | set(capi.SEARCH_SYMBOLS) | set(capi.PNP_SYMBOLS)
              | set(capi.SIM3_SYMBOLS) | set(capi.FUSE_SYMBOLS) | set(capi.TRACK_SYMBOLS) | set(capi.PLACES_SYMBOLS))
    assert not set(names) & others
    for nm in names:
        assert hasattr(lib, nm), nm
    p = capi.GraphParams.make(lib)
    assert (p.max_iterations, p.cg_iterations, p.cg_tolerance) == (20, 2048, 1e-8)
    assert lib.vslam_graph_params_default(capi.C.c_void_p(0)) == -1
    text = open(os.path.join(ROOT, "include", "vslam_graph.h")).read()
    assert "#define VSLAM_GRAPH_MAX_NODES 4096" in text and "#define VSLAM_GRAPH_MAX_EDGES 8192" in text
