"""vslam_amd/csrc/graph_math.h -- the code the kernel of vslam_graph_optimize runs -- walked serially by a stand-alone host program
(tests/native/graph_serial.cpp) built with -fsanitize=address,undefined -ffp-contract=off, against tests/ref_graph.py: the number of
usable edges, which nodes are written and every left-alone item's bits exactly, the optimised nodes within 16 x DELTA_REF.  The
program's workspace is exactly the bytes include/vslam_graph.h states, so a pass that ran past its part would be caught.  No GPU."""
import pytest

import graph_cases as gc
import ref_graph as rg


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("graph_serial")
    return gc.build_serial(tmp), tmp


def test_hand_cases(serial):
    exe, tmp = serial
    cases = gc.hand_cases()
    res = gc.run_serial(exe, tmp, [c[0] for c in cases.values()])
    for (name, (it, moved, use)), got in zip(cases.items(), res):
        assert got["stats"][0] == use, name
        gc.hold(name, got, it, 16 * rg.DELTA_REF)
        assert gc.written(got, it).any() == moved, name


def test_shapes(serial):
    exe, tmp = serial
    items = [gc.shape_item(k) for k in range(len(gc.SHAPES))]
    for k, got in enumerate(gc.run_serial(exe, tmp, items)):
        gc.hold(str(gc.SHAPES[k]), got, items[k], 16 * rg.DELTA_REF)


def test_workspace_bytes_are_the_headers():
    for N, E in ((1, 1), (7, 9), (256, 257), (4096, 8192)):
        words = 4 * N + 3 * E + 4
        assert 8 * (124 * N + 45 * E) + 4 * ((words + 1) // 2 * 2) == (1008 * N + 372 * E + 16 + 7) // 8 * 8
