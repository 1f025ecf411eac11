"""vslam_view_default / vslam_view_look_at are host code (no context, no device): held bit for bit to tests/ref_render.py,
whose own look_at is held to its geometry in tests/test_ref_render.py.  No GPU."""
import ctypes

import numpy as np
import pytest

import ref_render


@pytest.fixture(scope="module")
def lib():
    from vslam_amd import build, capi
    build.build()
    return capi.load_library()


def test_view_struct_layout():
    from vslam_amd import capi
    assert ctypes.sizeof(capi.View) == 116 and capi.View.point_size.offset == 88 and capi.View.background_bgr.offset == 108


def test_default_view_bits(lib):
    from vslam_amd import capi
    for w, h in ((640, 480), (1277, 95), (1, 1)):
        v, r = capi.View.default(w, h, lib), ref_render.default_view(w, h)
        assert np.array_equal(np.array(list(v.mv), np.float32).view(np.uint32), r.mv.view(np.uint32))
        assert (np.float32(v.fu), np.float32(v.fv), v.u0, v.v0, np.float32(v.z_near), v.z_far) == (r.fu, r.fv, r.u0, r.v0, r.z_near, r.z_far)
        assert (v.point_size, v.flags) == (1, capi.RENDER_FRUSTA) and tuple(np.float32(x) for x in (v.box_w, v.box_h_ratio, v.box_z_ratio)) == r.box
        assert tuple(v.background_bgr) == (0, 0, 0) and tuple(v.frustum_bgr) == (255, 0, 0)
    out = capi.View()
    assert lib.vslam_view_default(0, 5, ctypes.byref(out)) == -1 and lib.vslam_view_default(5, 5, None) == -1


def test_look_at_bits_and_degenerate_cases(lib):
    rng = np.random.default_rng(9)
    d3 = ctypes.c_double * 3
    for _ in range(200):
        eye, target, up = rng.uniform(-50, 50, 3), rng.uniform(-50, 50, 3), rng.normal(size=3)
        mv = (ctypes.c_float * 16)()
        assert lib.vslam_view_look_at(d3(*eye), d3(*target), d3(*up), mv) == 0
        assert np.array_equal(np.array(list(mv), np.float32).view(np.uint32), ref_render.look_at(eye, target, up).view(np.uint32))
    mv = (ctypes.c_float * 16)(*([7.0] * 16))
    assert lib.vslam_view_look_at(d3(1, 2, 3), d3(1, 2, 3), d3(0, 1, 0), mv) == -5          # eye == target
    assert lib.vslam_view_look_at(d3(0, 0, 0), d3(0, 3, 0), d3(0, 1, 0), mv) == -5          # up along the view
    assert list(mv) == [7.0] * 16
    assert lib.vslam_view_look_at(None, d3(0, 3, 0), d3(0, 1, 0), mv) == -1
