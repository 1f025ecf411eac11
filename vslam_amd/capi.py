"""ctypes binding of include/vslam_amd.h for the Python harness (tests, bench.py, smoke()).

Plumbing only: torch provides device memory and streams; every computation goes through the
C ABI in libvslam_amd.so.  There is no fallback path: if the library is missing or no HIP device
is visible, construction raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VSLAM_AMD_LIB: another build of the same library (A/B timing of kernel variants: tools/ab_kernels.py)
LIB_PATH = os.environ.get("VSLAM_AMD_LIB") or os.path.join(_HERE, "libvslam_amd.so")
# The experiments build of the same sources (-DVSLAM_EXPERIMENTS): the environment-variable A/B switches and the kernel variants
# that were measured and not chosen live only there (tools/ab_*.py, the variant tests); the product library has neither.
EXP_LIB_PATH = os.path.join(_HERE, "libvslam_amd_exp.so")

OK = 0
ERRORS = {-1: "VSLAM_ERR_INVALID", -2: "VSLAM_ERR_HIP", -3: "VSLAM_ERR_NO_DEVICE",
          -4: "VSLAM_ERR_CAPACITY", -5: "VSLAM_ERR_DEGENERATE", -6: "VSLAM_ERR_COMM"}

# every symbol include/vslam_amd.h declares (tests/test_capi_symbols.py checks the header too)
SYMBOLS = [
    "vslam_ctx_create", "vslam_ctx_make_current", "vslam_ctx_destroy", "vslam_ctx_set_stream", "vslam_ctx_set_option", "vslam_ctx_synchronize", "vslam_ctx_wait",
    "vslam_last_error", "vslam_ctx_workspace_bytes", "vslam_ctx_workspace_fill", "vslam_ctx_workspace_slots", "vslam_version", "vslam_brief_pattern_31", "vslam_dev_alloc", "vslam_dev_free", "vslam_copy_h2d",
    "vslam_copy_d2h", "vslam_debug_stream_copy", "vslam_debug_valu_calib", "vslam_prof_enable", "vslam_prof_reset", "vslam_prof_count", "vslam_prof_get",
    "vslam_match_knn2_ratio", "vslam_ransac_sets", "vslam_ransac_fundamental", "vslam_ransac_solve",
    "vslam_ransac_evaluate", "vslam_refit_fundamental", "vslam_refine_pairs", "vslam_kdtree_build",
    "vslam_kdtree_radius", "vslam_kdtree_nearest", "vslam_kdtree_cell_table", "vslam_extract_features", "vslam_extract_features_grid", "vslam_triangulate_points", "vslam_frontend_pairs_pose", "vslam_pipeline_batches_redone", "vslam_corner_stats", "vslam_bgr2gray", "vslam_min_eigen",
    "vslam_good_features", "vslam_gaussian7", "vslam_orb_describe", "vslam_extract_Rt", "vslam_triangulate", "vslam_associate_map_points", "vslam_reprojection_filter",
    "vslam_match_features",
    "vslam_map_create", "vslam_map_destroy", "vslam_map_reset", "vslam_map_step", "vslam_map_view", "vslam_map_observations",
    "vslam_track_sequences",
    "vslam_world_create", "vslam_world_destroy", "vslam_world_reset", "vslam_world_step", "vslam_world_lift", "vslam_world_view",
    "vslam_map_attach_world", "vslam_world_render",
    "vslam_view_default", "vslam_view_look_at", "vslam_render_points", "vslam_map_render",
    "vslam_frontend_pairs", "vslam_frontend_sequence", "vslam_pack_records",
    "vslam_host_alloc", "vslam_host_free", "vslam_upload_async", "vslam_upload_fence", "vslam_upload_wait", "vslam_download_async",
    "vslam_shard_range", "vslam_multi_create", "vslam_multi_destroy", "vslam_multi_size", "vslam_multi_ctx", "vslam_multi_last_error",
    "vslam_multi_frontend_pairs", "vslam_multi_frontend_pairs_resident", "vslam_comm_info", "vslam_gather_records_v", "vslam_comm_unique_id", "vslam_comm_create", "vslam_comm_destroy", "vslam_gather_records",
    "vslam_pipeline_create", "vslam_pipeline_destroy", "vslam_pipeline_size", "vslam_pipeline_ctx", "vslam_pipeline_last_error",
    "vslam_pipeline_set_option", "vslam_pipeline_acquire", "vslam_pipeline_commit", "vslam_pipeline_submit_pairs", "vslam_pipeline_submit_pairs_pose",
    "vslam_pipeline_submit_sequence", "vslam_pipeline_poll", "vslam_pipeline_wait", "vslam_pipeline_drain",
]

# every symbol include/vslam_resect.h declares (a header of its own beside vslam_amd.h; tests/test_gpu_resect.py checks it)
RESECT_SYMBOLS = [
    "vslam_resect_params_default", "vslam_resect_poses", "vslam_world_set_resection", "vslam_world_step_resect",
    "vslam_world_resection_view",
]


class _Params(C.Structure):
    """A parameter struct of the C ABI: a subclass states its _fields_ and the struct's name, `_struct`, whose <_struct>_default
    fills it."""

    @classmethod
    def make(cls, lib, **fields):
        """<_struct>_default with `fields` written over it"""
        p = cls()
        rc = getattr(lib, cls._struct + "_default")(C.byref(p))
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: {cls._struct}_default")
        for k, v in fields.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"{cls._struct} has no field {k!r}")
            setattr(p, k, v)
        return p


class ResectParams(_Params):
    _struct = "vslam_resect_params"
    _fields_ = [("max_iterations", C.c_int32), ("rounds", C.c_int32), ("min_links", C.c_int32), ("huber_px", C.c_double),
                ("gate_px", C.c_double)]


# every symbol include/vslam_adjust.h declares (a header of its own; tests/test_gpu_adjust.py checks it)
ADJUST_SYMBOLS = ["vslam_adjust_params_default", "vslam_adjust_windows", "vslam_world_adjust"]


class AdjustParams(_Params):
    _struct = "vslam_adjust_params"
    _fields_ = [("max_iterations", C.c_int32), ("rounds", C.c_int32), ("min_obs", C.c_int32), ("n_fixed", C.c_int32),
                ("huber_px", C.c_double), ("gate_px", C.c_double)]


# every symbol include/vslam_search.h declares (a header of its own; tests/test_gpu_search.py checks it)
SEARCH_SYMBOLS = ["vslam_search_params_default", "vslam_search_projection", "vslam_map_observation_descriptors", "vslam_world_search"]


class SearchParams(_Params):
    _struct = "vslam_search_params"
    _fields_ = [("radius_px", C.c_double), ("dist_threshold", C.c_int32), ("ratio10", C.c_int32)]


# every symbol include/vslam_pnp.h declares (a header of its own; tests/test_pnp_lds.py checks it)
PNP_SYMBOLS = ["vslam_pnp_params_default", "vslam_pnp_ransac", "vslam_match_params_default", "vslam_match_points", "vslam_world_relocalise"]


class PnpParams(_Params):
    _struct = "vslam_pnp_params"
    _fields_ = [("hypotheses", C.c_int32), ("min_inliers", C.c_int32), ("inlier_px", C.c_double)]


class MatchParams(_Params):
    _struct = "vslam_match_params"
    _fields_ = [("dist_threshold", C.c_int32), ("ratio10", C.c_int32)]


# every symbol include/vslam_sim3.h declares (a header of its own; tests/test_sim3_lds.py checks it)
SIM3_SYMBOLS = ["vslam_sim3_params_default", "vslam_sim3_ransac", "vslam_sim3_refine", "vslam_world_sim3", "vslam_world_apply_sim3"]


class Sim3Params(_Params):
    _struct = "vslam_sim3_params"
    _fields_ = [("hypotheses", C.c_int32), ("min_inliers", C.c_int32), ("inlier_px", C.c_double)]


# every symbol include/vslam_graph.h declares (a header of its own; tests/test_graph_lds.py checks it)
GRAPH_SYMBOLS = ["vslam_graph_params_default", "vslam_graph_optimize", "vslam_world_close_loops"]


class GraphParams(_Params):
    _struct = "vslam_graph_params"
    _fields_ = [("max_iterations", C.c_int32), ("cg_iterations", C.c_int32), ("cg_tolerance", C.c_double)]


# every symbol include/vslam_fuse.h declares (a header of its own; tests/test_gpu_fuse.py checks it)
FUSE_SYMBOLS = ["vslam_cull_params_default", "vslam_fuse_points", "vslam_cull_points", "vslam_world_fuse", "vslam_world_cull",
                "vslam_world_observations", "vslam_world_fusion_view"]


class CullParams(_Params):
    _struct = "vslam_cull_params"
    _fields_ = [("inlier_px", C.c_double), ("min_good", C.c_int32), ("mature_good", C.c_int32), ("mature_age", C.c_int32),
                ("good10", C.c_int32)]


# every symbol include/vslam_fuse_project.h declares (a header of its own; tests/test_fuse_project_lds.py checks it)
FUSE_PROJECT_SYMBOLS = ["vslam_fuse_project", "vslam_world_fuse_project", "vslam_world_fuse_project_view"]


# every symbol include/vslam_tracks.h declares (a header of its own; tests/test_gpu_tracks.py checks it)
TRACK_SYMBOLS = ["vslam_track_params_default", "vslam_triangulate_tracks", "vslam_world_retriangulate"]


class TrackParams(_Params):
    _struct = "vslam_track_params"
    _fields_ = [("cos_parallax_max", C.c_double), ("huber_px", C.c_double), ("inlier_px", C.c_double), ("iterations", C.c_int32),
                ("min_good", C.c_int32), ("good10", C.c_int32)]


# every symbol include/vslam_places.h declares (a header of its own; tests/test_gpu_places.py checks it)
PLACES_SYMBOLS = ["vslam_places_assign", "vslam_places_train", "vslam_places_create", "vslam_places_destroy", "vslam_places_reset",
                  "vslam_places_set_vocabulary", "vslam_places_set_weights", "vslam_places_add", "vslam_places_query", "vslam_places_view"]
PLACES_MAX_WORDS = 16384


class PlacesArrays(C.Structure):   # vslam_places_arrays
    _fields_ = [("n_words", C.c_int32), ("capacity", C.c_int32), ("max_kp", C.c_int32), ("size", C.c_int32)] + [
        (k, C.c_void_p) for k in ("d_offsets", "d_words", "d_tf", "d_df", "d_norms", "d_tags", "d_weights", "d_vocab")]


def places_weights(df, n_entries):
    """The rounded-log weights of an index: rint(1024 ln(n_entries / df)) where df > 0, else 0, clipped to 65535, int32.  Computed
    HERE, on the host in float64, and nowhere else: the device never takes a logarithm, so the weights are an input to both sides
    of every comparison."""
    import numpy as np
    df = np.asarray(df, np.int64)
    w = np.zeros(df.shape, np.float64)
    pos = df > 0
    w[pos] = np.rint(1024.0 * np.log(np.float64(n_entries) / df[pos].astype(np.float64)))
    return np.clip(w, 0, 65535).astype(np.int32)


class ExtractParams(C.Structure):
    _fields_ = [("max_corners", C.c_int32), ("quality", C.c_double), ("min_distance", C.c_double),
                ("cos_a", C.c_float), ("sin_a", C.c_float), ("d_pattern", C.c_void_p)]


class PoseOutputs(C.Structure):   # vslam_pose_outputs
    _fields_ = [("d_R", C.c_void_p), ("d_t", C.c_void_p), ("d_c2", C.c_void_p), ("d_points4d", C.c_void_p),
                ("d_inlier_idx", C.c_void_p), ("d_n_inliers", C.c_void_p), ("d_error", C.c_void_p)]


class MapArrays(C.Structure):   # vslam_map_arrays
    _fields_ = [("tracks", C.c_int32), ("max_frames", C.c_int32), ("kp_stride", C.c_int32), ("map_capacity", C.c_int32),
                ("obs_capacity", C.c_int32), ("frames", C.c_int32), ("d_points", C.c_void_p), ("d_colors", C.c_void_p),
                ("d_sizes", C.c_void_p), ("d_map_point_ids", C.c_void_p), ("d_R_t", C.c_void_p), ("d_pose", C.c_void_p),
                ("d_obs_counts", C.c_void_p), ("d_n_obs", C.c_void_p)]


class WorldArrays(C.Structure):   # vslam_world_arrays
    _fields_ = [("tracks", C.c_int32), ("max_frames", C.c_int32), ("kp_stride", C.c_int32), ("min_links", C.c_int32),
                ("map_capacity", C.c_int32), ("frames", C.c_int32), ("d_Twc", C.c_void_p), ("d_pose", C.c_void_p),
                ("d_scale", C.c_void_p), ("d_links", C.c_void_p), ("d_carry", C.c_void_p), ("d_carry_index", C.c_void_p),
                ("d_world_points", C.c_void_p)]


class VslamError(RuntimeError):
    pass


RENDER_FRUSTA = 1
RENDER_AS_REFERENCE = 2


class View(C.Structure):   # vslam_view
    """The viewer of vslam_render_points / vslam_map_render.  View.default(w, h) is the reference's window
    (src/display.cpp:25-26); View.look_at(eye, target, up, ...) places the viewer (vslam_view_look_at).  The fields are the
    struct's and can be set freely (point_size, flags, z_near, ...)."""
    _fields_ = [("mv", C.c_float * 16), ("fu", C.c_float), ("fv", C.c_float), ("u0", C.c_float), ("v0", C.c_float),
                ("z_near", C.c_float), ("z_far", C.c_float), ("point_size", C.c_int32), ("flags", C.c_int32),
                ("box_w", C.c_float), ("box_h_ratio", C.c_float), ("box_z_ratio", C.c_float),
                ("background_bgr", C.c_uint8 * 3), ("frustum_bgr", C.c_uint8 * 3)]

    @classmethod
    def default(cls, width, height, lib=None):
        lib = lib or load_library()
        v = cls()
        rc = lib.vslam_view_default(C.c_int(width), C.c_int(height), C.byref(v))
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: vslam_view_default({width}, {height})")
        return v

    @classmethod
    def look_at(cls, eye, target, up, width, height, lib=None, **fields):
        """View.default(width, height) seen from `eye` towards `target`; `fields` overwrite struct members."""
        lib = lib or load_library()
        v = cls.default(width, height, lib)
        d3 = C.c_double * 3
        rc = lib.vslam_view_look_at(d3(*[float(x) for x in eye]), d3(*[float(x) for x in target]), d3(*[float(x) for x in up]), v.mv)
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: vslam_view_look_at({eye}, {target}, {up})")
        for k, val in fields.items():
            if k in ("background_bgr", "frustum_bgr"):
                val = (C.c_uint8 * 3)(*val)
            setattr(v, k, val)
        return v

    def copy(self, **fields):
        v = type(self).from_buffer_copy(self)
        for k, val in fields.items():
            if k in ("background_bgr", "frustum_bgr"):
                val = (C.c_uint8 * 3)(*val)
            setattr(v, k, val)
        return v


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise VslamError(
            f"{path} is missing: run `python -m vslam_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback.")
    lib = C.CDLL(path)
    lib.vslam_last_error.restype = C.c_char_p
    lib.vslam_version.restype = C.c_char_p
    return lib


def _ptr(t):
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


class Context:
    """One vslam_ctx bound to a torch device/stream."""

    def __init__(self, device=0, use_torch_stream=True, lib=None):
        import torch
        self.torch = torch
        self.lib = lib if lib is not None else load_library()
        self.handle = C.c_void_p()
        rc = self.lib.vslam_ctx_create(C.c_int(device), C.byref(self.handle))
        if rc != OK:
            raise VslamError(f"vslam_ctx_create failed: {ERRORS.get(rc, rc)} (no HIP device? there is no CPU fallback)")
        self.device = torch.device("cuda", device)
        self.own_stream = not use_torch_stream
        if use_torch_stream:
            s = torch.cuda.current_stream(self.device)
            self._check(self.lib.vslam_ctx_set_stream(self.handle, C.c_void_p(s.cuda_stream)))

    def _ready(self):
        """Tensors torch has just filled (kernels on torch's stream) are handed to a context that runs on a stream of its own,
        which does not wait for torch's: wait here, or a fill can land on top of the results."""
        if getattr(self, "own_stream", True):
            self.torch.cuda.current_stream(self.device).synchronize()

    def close(self):
        if self.handle:
            self.lib.vslam_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            msg = self.lib.vslam_last_error(self.handle)
            raise VslamError(f"{ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def _dev(self, t, dtype, name):
        torch = self.torch
        if t is None:
            return None
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise VslamError(f"{name}: need a contiguous cuda tensor of {dtype}, got {t.dtype} on {t.device}")
        return t

    def synchronize(self):
        self._check(self.lib.vslam_ctx_synchronize(self.handle))

    def corner_stats(self):
        """{frames, px, listed, overflowed, pool}: the corner detector's counters of the last batch (vslam_corner_stats)."""
        a = (C.c_uint64 * 5)()
        self._check(self.lib.vslam_corner_stats(self.handle, a))
        return {"frames": int(a[0]), "px_per_frame": int(a[1]), "listed_pixels": int(a[2]), "frames_overflowed": int(a[3]),
                "pool_sets": int(a[4])}

    def workspace_bytes(self):
        n = C.c_size_t()
        self._check(self.lib.vslam_ctx_workspace_bytes(self.handle, C.byref(n)))
        return n.value

    def workspace_fill(self, byte=0):
        """vslam_ctx_workspace_fill: every workspace slot but the "ctx." ones set to `byte`, stream-ordered (a diagnostic: the next
        call of any entry point must give the bits it gives on any other workspace contents)."""
        self._ready()
        self._check(self.lib.vslam_ctx_workspace_fill(self.handle, C.c_int(int(byte))))

    def workspace_slots(self):
        """vslam_ctx_workspace_slots: {slot name: bytes} of the context's workspaces at the moment."""
        need = C.c_size_t()
        self._check(self.lib.vslam_ctx_workspace_slots(self.handle, C.c_char_p(None), C.c_size_t(0), C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._check(self.lib.vslam_ctx_workspace_slots(self.handle, buf, C.c_size_t(need.value), C.byref(need)))
        return {name: int(size) for name, size in (line.rsplit(" ", 1) for line in buf.value.decode().splitlines())}

    OPT_RANSAC_ALL_SUMS = 1
    OPT_RANSAC_MIN_MATCHES = 2
    OPT_RANSAC_SOLVER = 3
    OPT_MATCH_SHAPE = 4
    OPT_CORNER_WINDOW_PCT = 5
    OPT_RANSAC_MIN_ITEMS = 6
    OPT_CORNER_LIST_CAP = 7
    OPT_MATCH_FORM = 8
    OPT_TREE_FORK = 9
    OPT_POSE_REFIT = 10
    OPT_POSE_REFINE = 11

    def set_option(self, option, value):
        self._check(self.lib.vslam_ctx_set_option(self.handle, C.c_int(option), C.c_int(int(value))))

    # ---------------------------------------------------------------- profiling
    def prof_enable(self, on=True):
        self._check(self.lib.vslam_prof_enable(self.handle, C.c_int(1 if on else 0)))

    def prof_reset(self):
        self._check(self.lib.vslam_prof_reset(self.handle))

    def prof_report(self):
        n = self.lib.vslam_prof_count(self.handle)
        if n < 0:
            self._check(n)
        out = {}
        for i in range(n):
            name = C.create_string_buffer(128)
            ms = C.c_double()
            cnt = C.c_int64()
            self._check(self.lib.vslam_prof_get(self.handle, C.c_int(i), name, C.c_int(128), C.byref(ms), C.byref(cnt)))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out

    def debug_detect(self, bgr, max_corners, width=None):
        """(experiments build only) cvtColor + goodFeaturesToTrack from the 3-byte image: the corners BEFORE the descriptor stage's
        border filter, in rank order -- (xy (F, max_corners, 2), n (F,))."""
        torch = self.torch
        F, H = bgr.shape[0], bgr.shape[1]
        W = width if width is not None else bgr.shape[2]
        stride = bgr.shape[2] * (bgr.shape[3] if bgr.dim() == 4 else 1)
        xy = torch.zeros((F, max_corners, 2), dtype=torch.float32, device=bgr.device)
        n = torch.zeros((F,), dtype=torch.int32, device=bgr.device)
        self._ready()
        self._check(self.lib.vslam_debug_detect(self.handle, _ptr(bgr), C.c_int(F), C.c_int(W), C.c_int(H), C.c_int(stride),
                                                C.c_int(max_corners), C.c_int(max_corners), _ptr(xy), _ptr(n)))
        return xy, n

    def debug_ransac_prune_x(self, batch, hyp):
        """(experiments build only) X[h] of this context's last ransac_prune launch: the matches behind the ranked head that
        were certified misses of each hypothesis, (batch, hyp) int32 (zero where no wave walked the hypothesis)."""
        torch = self.torch
        x = torch.zeros((batch, hyp), dtype=torch.int32, device="cuda")
        self._ready()
        self._check(self.lib.vslam_debug_ransac_prune_x(self.handle, _ptr(x), C.c_int(batch), C.c_int(hyp)))
        return x

    def debug_ransac_head(self, batch, hyp):
        """(experiments build only) of this context's last RANSAC scoring: pot0 as ransac_screen_kernel left it, (batch, hyp)
        int32, and the routing word per pair, (batch,) int32: 1 = the head on the prune certificate, 0 = on the cheap evaluation,
        -1 = too few matches."""
        torch = self.torch
        pot0 = torch.zeros((batch, hyp), dtype=torch.int32, device="cuda")
        route = torch.zeros((batch,), dtype=torch.int32, device="cuda")
        self._ready()
        self._check(self.lib.vslam_debug_ransac_head(self.handle, _ptr(pot0), _ptr(route), C.c_int(batch), C.c_int(hyp)))
        return pot0, route

    def debug_ransac_prune_tile(self, F, xy):
        """(experiments build only) one 32 x 32 tile through ransac_prune's operand and accumulator mapping: F (32, 9), xy (4, 32)
        = x1, y1, x2, y2 -> n, a0 as (hypothesis, match) f32."""
        torch = self.torch
        self._dev(F, torch.float32, "F"); self._dev(xy, torch.float32, "xy")
        assert tuple(F.shape) == (32, 9) and tuple(xy.shape) == (4, 32)
        n = torch.zeros((32, 32), dtype=torch.float32, device=F.device)
        a0 = torch.zeros((32, 32), dtype=torch.float32, device=F.device)
        self._ready()
        self._check(self.lib.vslam_debug_ransac_prune_tile(self.handle, _ptr(F), _ptr(xy), _ptr(n), _ptr(a0)))
        return n, a0

    def debug_valu_calib(self):
        self._check(self.lib.vslam_debug_valu_calib(self.handle))

    def debug_stream_copy(self, src, dst, bytes_per_lane):
        self._check(self.lib.vslam_debug_stream_copy(self.handle, _ptr(src), _ptr(dst), C.c_size_t(src.numel() * src.element_size()),
                                                     C.c_int(bytes_per_lane)))

    # ---------------------------------------------------------------- stages
    def match_knn2_ratio(self, desc1, n1, desc2, n2, want_knn=False):
        torch = self.torch
        B, K, _ = desc1.shape
        self._dev(desc1, torch.uint8, "desc1"); self._dev(desc2, torch.uint8, "desc2")
        self._dev(n1, torch.int32, "n1"); self._dev(n2, torch.int32, "n2")
        pairs = torch.empty((B, K, 2), dtype=torch.int32, device=desc1.device)
        m = torch.empty((B,), dtype=torch.int32, device=desc1.device)
        knn = torch.empty((B, K, 4), dtype=torch.int32, device=desc1.device) if want_knn else None
        self._check(self.lib.vslam_match_knn2_ratio(self.handle, _ptr(desc1), _ptr(n1), _ptr(desc2), _ptr(n2),
                                                    C.c_int(B), C.c_int(K), _ptr(pairs), _ptr(m), _ptr(knn)))
        return (pairs, m, knn) if want_knn else (pairs, m)

    def ransac_sets(self, seeds, m, hyp):
        torch = self.torch
        B = seeds.shape[0]
        self._dev(seeds, torch.int32, "seeds"); self._dev(m, torch.int32, "m")
        sets = torch.empty((B, hyp, 8), dtype=torch.int32, device=seeds.device)
        draws = torch.empty((B, hyp * 8), dtype=torch.int32, device=seeds.device)
        self._check(self.lib.vslam_ransac_sets(self.handle, _ptr(seeds), _ptr(m), C.c_int(B), C.c_int(hyp),
                                               _ptr(sets), _ptr(draws)))
        return sets

    def ransac_fundamental(self, xy1, xy2, pairs, m, sets, threshold):
        torch = self.torch
        B, K, _ = xy1.shape
        H = sets.shape[1]
        dev = xy1.device
        for t, dt, nm in ((xy1, torch.float32, "xy1"), (xy2, torch.float32, "xy2"), (pairs, torch.int32, "pairs"),
                          (m, torch.int32, "m"), (sets, torch.int32, "sets")):
            self._dev(t, dt, nm)
        out = dict(
            F=torch.zeros((B, 9), dtype=torch.float32, device=dev),
            mask=torch.zeros((B, K), dtype=torch.uint8, device=dev),
            best=torch.zeros((B, 4), dtype=torch.int32, device=dev),
            matches=torch.zeros((B, K, 2), dtype=torch.int32, device=dev),
            hypF=torch.zeros((B, H, 9), dtype=torch.float32, device=dev),
            hyp_count=torch.zeros((B, H), dtype=torch.int32, device=dev),
            hyp_sum=torch.zeros((B, H), dtype=torch.float32, device=dev),
        )
        self._check(self.lib.vslam_ransac_fundamental(
            self.handle, _ptr(xy1), _ptr(xy2), _ptr(pairs), _ptr(m), _ptr(sets), C.c_int(B), C.c_int(K),
            C.c_int(H), C.c_float(threshold), _ptr(out["F"]), _ptr(out["mask"]), _ptr(out["best"]),
            _ptr(out["matches"]), _ptr(out["hypF"]), _ptr(out["hyp_count"]), _ptr(out["hyp_sum"])))
        return out

    def ransac_evaluate(self, xy1, xy2, pairs, m, hypF, threshold):
        """compute_fundamental_residual for GIVEN hypotheses + the accept rule (vslam_ransac_evaluate)."""
        torch = self.torch
        B, K, _ = xy1.shape
        H = hypF.shape[1]
        dev = xy1.device
        for t, dt, nm in ((xy1, torch.float32, "xy1"), (xy2, torch.float32, "xy2"), (pairs, torch.int32, "pairs"),
                          (m, torch.int32, "m"), (hypF, torch.float32, "hypF")):
            self._dev(t, dt, nm)
        out = dict(
            F=torch.zeros((B, 9), dtype=torch.float32, device=dev),
            mask=torch.zeros((B, K), dtype=torch.uint8, device=dev),
            best=torch.zeros((B, 4), dtype=torch.int32, device=dev),
            matches=torch.zeros((B, K, 2), dtype=torch.int32, device=dev),
            hyp_count=torch.zeros((B, H), dtype=torch.int32, device=dev),
            hyp_sum=torch.zeros((B, H), dtype=torch.float32, device=dev),
        )
        self._check(self.lib.vslam_ransac_evaluate(
            self.handle, _ptr(xy1), _ptr(xy2), _ptr(pairs), _ptr(m), _ptr(hypF), C.c_int(B), C.c_int(K), C.c_int(H),
            C.c_float(threshold), _ptr(out["F"]), _ptr(out["mask"]), _ptr(out["best"]), _ptr(out["matches"]),
            _ptr(out["hyp_count"]), _ptr(out["hyp_sum"])))
        return out

    def refit_fundamental(self, xy1, xy2, matches, best, F, out=None, want_stats=True):
        """vslam_refit_fundamental: the RANSAC winner F (B, 9) refitted over its inlier matches (B, K, 2) / best (B, 4) as
        ransac_* / match_features return them.  Returns (F_out (B, 9) f32, stats (B, 4) f64 or None); out=F refits in place."""
        torch = self.torch
        B, K, _ = xy1.shape
        for t, dt, nm in ((xy1, torch.float32, "xy1"), (xy2, torch.float32, "xy2"), (matches, torch.int32, "matches"),
                          (best, torch.int32, "best"), (F, torch.float32, "F"), (out, torch.float32, "out")):
            self._dev(t, dt, nm)
        if out is None:
            out = torch.empty((B, 9), dtype=torch.float32, device=xy1.device)
        stats = torch.empty((B, 4), dtype=torch.float64, device=xy1.device) if want_stats else None
        self._ready()
        self._check(self.lib.vslam_refit_fundamental(self.handle, _ptr(xy1), _ptr(xy2), _ptr(matches), _ptr(best), C.c_int(B),
                                                     C.c_int(K), _ptr(F), _ptr(out), _ptr(stats)))
        return out, stats

    def refine_pairs(self, xy1, xy2, matches, best, K, R, t, points4d, gate_sq=16.0, max_iterations=20, want_stats=True):
        """vslam_refine_pairs: two-view bundle adjustment of each pair's R (B, 9 or 3, 3), t (B, 3) and points4d (B, K, 4), IN
        PLACE, over the inlier matches (B, K, 2) / best (B, 4); K: the 3 x 3 camera matrix (host).  Returns
        (R, t, c2 (B, 12), points4d, stats (B, 4) f64 or None) -- R, t and points4d are the tensors passed in."""
        import numpy as np
        torch = self.torch
        B, Kp, _ = xy1.shape
        for x, dt, nm in ((xy1, torch.float32, "xy1"), (xy2, torch.float32, "xy2"), (matches, torch.int32, "matches"),
                          (best, torch.int32, "best"), (R, torch.float32, "R"), (t, torch.float32, "t"),
                          (points4d, torch.float32, "points4d")):
            self._dev(x, dt, nm)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        c2 = torch.empty((B, 12), dtype=torch.float32, device=xy1.device)
        stats = torch.empty((B, 4), dtype=torch.float64, device=xy1.device) if want_stats else None
        self._ready()
        self._check(self.lib.vslam_refine_pairs(self.handle, _ptr(xy1), _ptr(xy2), _ptr(matches), _ptr(best), C.c_int(B), C.c_int(Kp),
                                                Kh.ctypes.data_as(C.c_void_p), C.c_float(gate_sq), C.c_int(max_iterations),
                                                _ptr(R), _ptr(t), _ptr(c2), _ptr(points4d), _ptr(stats)))
        return R, t, c2, points4d, stats

    def resect_poses(self, points, xy, n, K, R, T, want_stats=True, **params):
        """vslam_resect_poses (include/vslam_resect.h): the pose-only adjustment of each item's R (B, 9 or 3, 3) f64 and T (B, 3)
        f64, IN PLACE, from points (B, S, 3) f64 seen at xy (B, S, 2) f32, n (B,) i32 of them; K: the 3 x 3 camera matrix (host);
        params: fields of vslam_resect_params over its defaults.  Returns (R, T, stats (B, 4) f64 or None)."""
        import numpy as np
        torch = self.torch
        B, S, _ = points.shape
        for x, dt, nm in ((points, torch.float64, "points"), (xy, torch.float32, "xy"), (n, torch.int32, "n"),
                          (R, torch.float64, "R"), (T, torch.float64, "T")):
            self._dev(x, dt, nm)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        stats = torch.empty((B, 4), dtype=torch.float64, device=points.device) if want_stats else None
        prm = ResectParams.make(self.lib, **params)
        self._ready()
        self._check(self.lib.vslam_resect_poses(self.handle, _ptr(points), _ptr(xy), _ptr(n), C.c_int(B), C.c_int(S),
                                                Kh.ctypes.data_as(C.c_void_p), C.byref(prm), _ptr(R), _ptr(T), _ptr(stats)))
        return R, T, stats

    def adjust_windows(self, R, T, n_cams, points, n_points, obs_offsets, obs_cam, obs_xy, K, want_stats=True, **params):
        """vslam_adjust_windows (include/vslam_adjust.h): each item's cameras R (B, C, 9) / T (B, C, 3) f64 and points (B, P, 3) f64
        adjusted together IN PLACE from the observations in CSR by point: obs_offsets (B, P + 1) i32, obs_cam (B, O) i32, obs_xy
        (B, O, 2) f32; n_cams / n_points (B,) i32; K: the 3 x 3 camera matrix (host); params: fields of vslam_adjust_params over
        its defaults.  Returns (R, T, points, stats (B, 4) f64 or None)."""
        import numpy as np
        torch = self.torch
        B, Cs = R.shape[0], R.shape[1]
        P, O = points.shape[1], obs_cam.shape[1]
        for x, dt, nm in ((R, torch.float64, "R"), (T, torch.float64, "T"), (n_cams, torch.int32, "n_cams"), (points, torch.float64, "points"),
                          (n_points, torch.int32, "n_points"), (obs_offsets, torch.int32, "obs_offsets"), (obs_cam, torch.int32, "obs_cam"),
                          (obs_xy, torch.float32, "obs_xy")):
            self._dev(x, dt, nm)
        if tuple(obs_offsets.shape) != (B, P + 1):
            raise ValueError(f"obs_offsets has shape {tuple(obs_offsets.shape)}, not {(B, P + 1)}")
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        stats = torch.empty((B, 4), dtype=torch.float64, device=R.device) if want_stats else None
        prm = AdjustParams.make(self.lib, **params)
        self._ready()
        self._check(self.lib.vslam_adjust_windows(self.handle, _ptr(R), _ptr(T), _ptr(n_cams), C.c_int(Cs), _ptr(points), _ptr(n_points),
                                                  C.c_int(P), _ptr(obs_offsets), _ptr(obs_cam), _ptr(obs_xy), C.c_int(O), C.c_int(B),
                                                  Kh.ctypes.data_as(C.c_void_p), C.byref(prm), _ptr(stats)))
        return R, T, points, stats

    def _outputs(self, out, shapes, device):
        """`out` (a dict of output tensors or None) as a new dict with the missing tensors of `shapes` (name -> (shape, dtype)) made,
        zero-filled, and every one of them checked"""
        o = dict(out or {})
        for k, (shape, dt) in shapes.items():
            if k not in o:
                o[k] = self.torch.zeros(shape, dtype=dt, device=device)
            self._dev(o[k], dt, k)
        return o

    def _correspond(self, call, params_cls, params, pose, pose_args, points, n_points, obs_offsets, obs_desc, xy, desc, n_kp, kp_taken,
                    out, want_indices, want_stats):
        """search_projection and match_points: `call` is the library's entry point, params the fields over params_cls' defaults; the
        projection alone has pose, its (name, f64 tensor) pairs, and pose_args, its C arguments between them and d_xy"""
        torch = self.torch
        B, S, _ = points.shape
        Kp, O = xy.shape[1], obs_desc.shape[1]
        for x, dt, nm in ((points, torch.float32, "points"), (n_points, torch.int32, "n_points"), (obs_offsets, torch.int32, "obs_offsets"),
                          (obs_desc, torch.uint8, "obs_desc"), *((x, torch.float64, nm) for nm, x in pose), (xy, torch.float32, "xy"),
                          (desc, torch.uint8, "desc"), (n_kp, torch.int32, "n_kp"), (kp_taken, torch.int32, "kp_taken")):
            self._dev(x, dt, nm)
        if tuple(obs_offsets.shape) != (B, S + 1):
            raise ValueError(f"obs_offsets has shape {tuple(obs_offsets.shape)}, not {(B, S + 1)}")
        shapes = dict(kp_of_point=((B, S), torch.int32), dist=((B, S), torch.int32), corr_points=((B, Kp, 3), torch.float64),
                      corr_xy=((B, Kp, 2), torch.float32), n_corr=((B,), torch.int32))
        if want_indices:
            shapes.update(corr_point=((B, Kp), torch.int32), corr_kp=((B, Kp), torch.int32))
        if want_stats:
            shapes.update(stats=((B, 4), torch.int32))
        o = self._outputs(out, shapes, points.device)
        prm = params_cls.make(self.lib, **params)
        self._ready()
        self._check(call(
            self.handle, _ptr(points), _ptr(n_points), C.c_int(S), _ptr(obs_offsets), _ptr(obs_desc), C.c_int(O),
            *(_ptr(x) for _, x in pose), *pose_args, _ptr(xy), _ptr(desc), _ptr(n_kp), C.c_int(Kp), _ptr(kp_taken), C.c_int(B), C.byref(prm),
            _ptr(o["kp_of_point"]), _ptr(o["dist"]), _ptr(o["corr_points"]), _ptr(o["corr_xy"]), _ptr(o.get("corr_point")),
            _ptr(o.get("corr_kp")), _ptr(o["n_corr"]), _ptr(o.get("stats"))))
        return o

    def search_projection(self, points, n_points, obs_offsets, obs_desc, R, T, K, width, height, xy, desc, n_kp, kp_taken=None,
                          out=None, want_indices=True, want_stats=True, **params):
        """vslam_search_projection (include/vslam_search.h): each item's points (B, S, 4) f32, n_points (B,) i32 of them, with their
        observation descriptors in CSR (obs_offsets (B, S + 1) i32, obs_desc (B, O, 32) u8), projected with R (B, 9) / T (B, 3) f64
        and K (the 3 x 3 camera matrix, host) into a width x height frame with keypoints xy (B, Kp, 2) f32, desc (B, Kp, 32) u8, n_kp
        (B,) i32; kp_taken (B, Kp) i32 or None; params: fields of vslam_search_params over its defaults.  out: a dict of output
        tensors to write into (missing ones are made, zero-filled).  Returns the dict: kp_of_point, dist (B, S) i32; corr_points
        (B, Kp, 3) f64; corr_xy (B, Kp, 2) f32; corr_point, corr_kp (B, Kp) i32 (want_indices); n_corr (B,) i32; stats (B, 4) i32
        (want_stats) -- the layout resect_poses reads."""
        import numpy as np
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        return self._correspond(self.lib.vslam_search_projection, SearchParams, params, (("R", R), ("T", T)),
                                (Kh.ctypes.data_as(C.c_void_p), C.c_int(width), C.c_int(height)), points, n_points,
                                obs_offsets, obs_desc, xy, desc, n_kp, kp_taken, out, want_indices, want_stats)

    def pnp_ransac(self, points, xy, n, K, seeds, R, T, polish=None, out=None, want_index=True, want_counts=False, want_stats=True,
                   **params):
        """vslam_pnp_ransac (include/vslam_pnp.h): a pose without a prior for each item, from points (B, S, 3) f64 seen at xy
        (B, S, 2) f32, n (B,) i32 of them, seeds (B,) i32 / u32 bits; K: the 3 x 3 camera matrix (host); R (B, 9 or 3, 3) and T
        (B, 3) f64 are written IN PLACE where an item is found and keep their bits elsewhere.  params: fields of vslam_pnp_params
        over its defaults; polish: None (no polish) or a dict of vslam_resect_params fields over their defaults.  out: a dict of
        output tensors to write into (missing ones are made, zero-filled).  Returns the dict: R, T; inlier (B, S) i32;
        corr_points (B, S, 3) f64; corr_xy (B, S, 2) f32; corr_index (B, S) i32 (want_index); n_inliers, winner (B,) i32; counts
        (B, hypotheses, 4) i32 (want_counts); stats (B, 4) f64 (want_stats)."""
        import numpy as np
        torch = self.torch
        B, S, _ = points.shape
        for x, dt, nm in ((points, torch.float64, "points"), (xy, torch.float32, "xy"), (n, torch.int32, "n"), (seeds, torch.int32, "seeds"),
                          (R, torch.float64, "R"), (T, torch.float64, "T")):
            self._dev(x, dt, nm)
        prm = PnpParams.make(self.lib, **params)
        shapes = dict(inlier=((B, S), torch.int32), corr_points=((B, S, 3), torch.float64), corr_xy=((B, S, 2), torch.float32),
                      n_inliers=((B,), torch.int32), winner=((B,), torch.int32))
        if want_index:
            shapes.update(corr_index=((B, S), torch.int32))
        if want_counts:
            shapes.update(counts=((B, max(int(prm.hypotheses), 0), 4), torch.int32))
        if want_stats:
            shapes.update(stats=((B, 4), torch.float64))
        o = self._outputs(out, shapes, points.device)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        pol = None if polish is None else ResectParams.make(self.lib, **polish)
        self._ready()
        self._check(self.lib.vslam_pnp_ransac(
            self.handle, _ptr(points), _ptr(xy), _ptr(n), C.c_int(B), C.c_int(S), Kh.ctypes.data_as(C.c_void_p), _ptr(seeds), C.byref(prm),
            C.byref(pol) if pol is not None else C.c_void_p(0), _ptr(R), _ptr(T), _ptr(o["inlier"]), _ptr(o["corr_points"]), _ptr(o["corr_xy"]),
            _ptr(o.get("corr_index")), _ptr(o["n_inliers"]), _ptr(o["winner"]), _ptr(o.get("counts")), _ptr(o.get("stats"))))
        o.update(R=R, T=T)
        return o

    def sim3_ransac(self, A, xa, B, xb, n, K, seeds, scale, R, T, polish=None, out=None, want_index=True, want_counts=False,
                    want_stats=True, **params):
        """vslam_sim3_ransac (include/vslam_sim3.h): the similarity B = s R A + t of each item, from A, B (Bt, S, 3) f64 seen at xa,
        xb (Bt, S, 2) f32, n (Bt,) i32 of them, seeds (Bt,) i32 / u32 bits; K: the 3 x 3 camera matrix of both images (host);
        scale (Bt,), R (Bt, 9 or 3, 3) and T (Bt, 3) f64 are written IN PLACE where an item is found and keep their bits
        elsewhere.  params: fields of vslam_sim3_params over its defaults; polish: None or a dict of vslam_resect_params fields
        over their defaults.  out: a dict of output tensors to write into (missing ones are made, zero-filled).  Returns the
        dict: scale, R, T; inlier (Bt, S) i32; corr_index (Bt, S) i32 (want_index); n_inliers, winner (Bt,) i32; counts
        (Bt, hypotheses) i32 (want_counts); stats (Bt, 4) f64 (want_stats)."""
        import numpy as np
        torch = self.torch
        Bt, S, _ = A.shape
        for x, dt, nm in ((A, torch.float64, "A"), (xa, torch.float32, "xa"), (B, torch.float64, "B"), (xb, torch.float32, "xb"),
                          (n, torch.int32, "n"), (seeds, torch.int32, "seeds"), (scale, torch.float64, "scale"), (R, torch.float64, "R"),
                          (T, torch.float64, "T")):
            self._dev(x, dt, nm)
        prm = Sim3Params.make(self.lib, **params)
        shapes = dict(inlier=((Bt, S), torch.int32), n_inliers=((Bt,), torch.int32), winner=((Bt,), torch.int32))
        if want_index:
            shapes.update(corr_index=((Bt, S), torch.int32))
        if want_counts:
            shapes.update(counts=((Bt, max(int(prm.hypotheses), 0)), torch.int32))
        if want_stats:
            shapes.update(stats=((Bt, 4), torch.float64))
        o = self._outputs(out, shapes, A.device)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        pol = None if polish is None else ResectParams.make(self.lib, **polish)
        self._ready()
        self._check(self.lib.vslam_sim3_ransac(
            self.handle, _ptr(A), _ptr(xa), _ptr(B), _ptr(xb), _ptr(n), C.c_int(Bt), C.c_int(S), Kh.ctypes.data_as(C.c_void_p), _ptr(seeds),
            C.byref(prm), C.byref(pol) if pol is not None else C.c_void_p(0), _ptr(scale), _ptr(R), _ptr(T), _ptr(o["inlier"]),
            _ptr(o.get("corr_index")), _ptr(o["n_inliers"]), _ptr(o["winner"]), _ptr(o.get("counts")), _ptr(o.get("stats"))))
        o.update(scale=scale, R=R, T=T)
        return o

    def sim3_refine(self, A, xa, B, xb, n, K, scale, R, T, mask=None, want_stats=True, **params):
        """vslam_sim3_refine (include/vslam_sim3.h): the 7-parameter polish of each item's scale (Bt,), R (Bt, 9 or 3, 3) and T
        (Bt, 3) f64, IN PLACE, over the correspondences i < n with mask[i] != 0 (mask (Bt, S) i32 or None: all of them); params:
        fields of vslam_resect_params over its defaults.  Returns (scale, R, T, stats (Bt, 4) f64 or None)."""
        import numpy as np
        torch = self.torch
        Bt, S, _ = A.shape
        for x, dt, nm in ((A, torch.float64, "A"), (xa, torch.float32, "xa"), (B, torch.float64, "B"), (xb, torch.float32, "xb"),
                          (n, torch.int32, "n"), (mask, torch.int32, "mask"), (scale, torch.float64, "scale"), (R, torch.float64, "R"),
                          (T, torch.float64, "T")):
            self._dev(x, dt, nm)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        stats = torch.empty((Bt, 4), dtype=torch.float64, device=A.device) if want_stats else None
        prm = ResectParams.make(self.lib, **params)
        self._ready()
        self._check(self.lib.vslam_sim3_refine(self.handle, _ptr(A), _ptr(xa), _ptr(B), _ptr(xb), _ptr(n), C.c_int(Bt), C.c_int(S), _ptr(mask),
                                               Kh.ctypes.data_as(C.c_void_p), C.byref(prm), _ptr(scale), _ptr(R), _ptr(T), _ptr(stats)))
        return scale, R, T, stats

    def graph_optimize(self, scale, R, T, fixed, n_nodes, edge_ab, edge_scale, edge_R, edge_T, edge_weight, n_edges, want_stats=True, **params):
        """vslam_graph_optimize (include/vslam_graph.h): each item's pose graph over Sim(3) optimised IN PLACE.  Nodes: scale (B, S), R
        (B, S, 9 or 3, 3), T (B, S, 3) f64, fixed (B, S) i32, n_nodes (B,) i32; edges: edge_ab (B, Es, 2) i32, edge_scale (B, Es), edge_R
        (B, Es, 9 or 3, 3), edge_T (B, Es, 3), edge_weight (B, Es, 3) f64, n_edges (B,) i32; params: fields of vslam_graph_params over
        its defaults.  Returns (scale, R, T, stats (B, 4) f64 or None)."""
        torch = self.torch
        B, S = scale.shape
        Es = edge_scale.shape[1]
        for x, dt, nm in ((scale, torch.float64, "scale"), (R, torch.float64, "R"), (T, torch.float64, "T"), (fixed, torch.int32, "fixed"),
                          (n_nodes, torch.int32, "n_nodes"), (edge_ab, torch.int32, "edge_ab"), (edge_scale, torch.float64, "edge_scale"),
                          (edge_R, torch.float64, "edge_R"), (edge_T, torch.float64, "edge_T"), (edge_weight, torch.float64, "edge_weight"),
                          (n_edges, torch.int32, "n_edges")):
            self._dev(x, dt, nm)
        stats = torch.empty((B, 4), dtype=torch.float64, device=scale.device) if want_stats else None
        prm = GraphParams.make(self.lib, **params)
        self._ready()
        self._check(self.lib.vslam_graph_optimize(self.handle, _ptr(scale), _ptr(R), _ptr(T), _ptr(fixed), _ptr(n_nodes), C.c_int(B), C.c_int(S),
                                                  _ptr(edge_ab), _ptr(edge_scale), _ptr(edge_R), _ptr(edge_T), _ptr(edge_weight), _ptr(n_edges),
                                                  C.c_int(Es), C.byref(prm), _ptr(stats)))
        return scale, R, T, stats

    def match_points(self, points, n_points, obs_offsets, obs_desc, xy, desc, n_kp, kp_taken=None, out=None, want_indices=True,
                     want_stats=True, **params):
        """vslam_match_points (include/vslam_pnp.h): search_projection without a pose -- every point (B, S, 4) f32 with a valid CSR
        row (obs_offsets (B, S + 1) i32, obs_desc (B, O, 32) u8) against every keypoint (xy (B, Kp, 2) f32, desc (B, Kp, 32) u8,
        n_kp (B,) i32) that is not taken (kp_taken (B, Kp) i32 or None); params: fields of vslam_match_params over its defaults.
        out and the returned dict as search_projection's."""
        return self._correspond(self.lib.vslam_match_points, MatchParams, params, (), (), points, n_points, obs_offsets, obs_desc, xy, desc,
                                n_kp, kp_taken, out, want_indices, want_stats)

    def fuse_points(self, n_points, obs_offsets, obs_cam, obs_kp, cam_stride, kp_stride, mask=None, out=None, want_src=True, want_stats=True):
        """vslam_fuse_points (include/vslam_fuse.h): each item's n_points (B,) i32 points with their observations in CSR (obs_offsets
        (B, S + 1), obs_cam / obs_kp (B, O) i32) grouped by shared (cam, kp); mask (B, S) i32 or None: a point with a value < 0 takes no
        part.  out: a dict of output tensors to write into (missing ones are made, zero-filled).  Returns the dict: fuse_to (B, S);
        out_offsets (B, S + 1); out_cam, out_kp (B, O); out_src (B, O) (want_src); stats (B, 4) (want_stats), all i32."""
        torch = self.torch
        B, S, O = obs_offsets.shape[0], obs_offsets.shape[1] - 1, obs_cam.shape[1]
        for x, nm in ((n_points, "n_points"), (obs_offsets, "obs_offsets"), (obs_cam, "obs_cam"), (obs_kp, "obs_kp"), (mask, "mask")):
            self._dev(x, torch.int32, nm)
        shapes = dict(fuse_to=((B, S), torch.int32), out_offsets=((B, S + 1), torch.int32), out_cam=((B, O), torch.int32),
                      out_kp=((B, O), torch.int32))
        if want_src:
            shapes.update(out_src=((B, O), torch.int32))
        if want_stats:
            shapes.update(stats=((B, 4), torch.int32))
        o = self._outputs(out, shapes, obs_offsets.device)
        self._ready()
        self._check(self.lib.vslam_fuse_points(
            self.handle, _ptr(n_points), C.c_int(S), _ptr(obs_offsets), _ptr(obs_cam), _ptr(obs_kp), C.c_int(O), C.c_int(cam_stride),
            C.c_int(kp_stride), _ptr(mask), C.c_int(B), _ptr(o["fuse_to"]), _ptr(o["out_offsets"]), _ptr(o["out_cam"]), _ptr(o["out_kp"]),
            _ptr(o.get("out_src")), _ptr(o.get("stats"))))
        return o

    def cull_points(self, points, n_points, obs_offsets, obs_cam, obs_kp, R, T, n_cams, xy, K, out=None, want_counts=True, **params):
        """vslam_cull_points (include/vslam_fuse.h): which of each item's points (B, S, 4) f32 their observations (CSR as
        fuse_points takes it) support under the cameras R (B, Cs, 9) / T (B, Cs, 3) f64, n_cams (B,) i32 of them, with keypoints xy
        (B, Cs, Kp, 2) f32 and K (the 3 x 3 camera matrix, host); params: fields of vslam_cull_params over its defaults.  Returns a
        dict: keep (B, S); counts (B, S, 2) (want_counts); stats (B, 4), all i32."""
        import numpy as np
        torch = self.torch
        B, S, O, Cs, Kp = points.shape[0], points.shape[1], obs_cam.shape[1], R.shape[1], xy.shape[2]
        for x, dt, nm in ((points, torch.float32, "points"), (n_points, torch.int32, "n_points"), (obs_offsets, torch.int32, "obs_offsets"),
                          (obs_cam, torch.int32, "obs_cam"), (obs_kp, torch.int32, "obs_kp"), (R, torch.float64, "R"), (T, torch.float64, "T"),
                          (n_cams, torch.int32, "n_cams"), (xy, torch.float32, "xy")):
            self._dev(x, dt, nm)
        shapes = dict(keep=((B, S), torch.int32), stats=((B, 4), torch.int32))
        if want_counts:
            shapes.update(counts=((B, S, 2), torch.int32))
        o = self._outputs(out, shapes, points.device)
        prm = CullParams.make(self.lib, **params)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        self._ready()
        self._check(self.lib.vslam_cull_points(
            self.handle, _ptr(points), _ptr(n_points), C.c_int(S), _ptr(obs_offsets), _ptr(obs_cam), _ptr(obs_kp), C.c_int(O), _ptr(R), _ptr(T),
            _ptr(n_cams), C.c_int(Cs), _ptr(xy), C.c_int(Kp), Kh.ctypes.data_as(C.c_void_p), C.c_int(B), C.byref(prm), _ptr(o["keep"]),
            _ptr(o.get("counts")), _ptr(o["stats"])))
        return o

    def fuse_project(self, points, n_points, obs_offsets, obs_cam, obs_kp, obs_desc, R, T, n_cams, xy, desc, n_kp, K, width, height,
                     cam_mask=None, found_stride=None, out=None, want_stats=True, **params):
        """vslam_fuse_project (include/vslam_fuse_project.h): each item's points (B, S, 4) f32 with their observations in CSR
        (obs_offsets (B, S + 1), obs_cam / obs_kp (B, O) i32, obs_desc (B, O, 32) u8) searched by projection in every camera that does
        not see them yet: R (B, Cs, 9) / T (B, Cs, 3) f64, n_cams (B,) i32, the cameras' keypoints xy (B, Cs, Kp, 2) f32, desc (B, Cs,
        Kp, 32) u8, n_kp (B, Cs) i32, cam_mask (B, Cs) i32 or None, K (the 3 x 3 camera matrix, host); params: fields of
        vslam_search_params over its defaults.  found_stride: slots per item (None: obs_offsets' O).  out: a dict of output tensors to
        write into (missing ones are made, zero-filled).  Returns the dict: found_point, found_cam, found_kp, found_dist,
        found_holder (B, found_stride); n_found (B,); stats (B, 6) (want_stats), all i32."""
        import numpy as np
        torch = self.torch
        B, S, O, Cs, Kp = points.shape[0], points.shape[1], obs_cam.shape[1], R.shape[1], xy.shape[2]
        for x, dt, nm in ((points, torch.float32, "points"), (n_points, torch.int32, "n_points"), (obs_offsets, torch.int32, "obs_offsets"),
                          (obs_cam, torch.int32, "obs_cam"), (obs_kp, torch.int32, "obs_kp"), (obs_desc, torch.uint8, "obs_desc"),
                          (R, torch.float64, "R"), (T, torch.float64, "T"), (n_cams, torch.int32, "n_cams"), (xy, torch.float32, "xy"),
                          (desc, torch.uint8, "desc"), (n_kp, torch.int32, "n_kp"), (cam_mask, torch.int32, "cam_mask")):
            self._dev(x, dt, nm)
        if tuple(obs_offsets.shape) != (B, S + 1):
            raise ValueError(f"obs_offsets has shape {tuple(obs_offsets.shape)}, not {(B, S + 1)}")
        Fs = O if found_stride is None else int(found_stride)
        shapes = {k: ((B, Fs), torch.int32) for k in ("found_point", "found_cam", "found_kp", "found_dist", "found_holder")}
        shapes.update(n_found=((B,), torch.int32))
        if want_stats:
            shapes.update(stats=((B, 6), torch.int32))
        o = self._outputs(out, shapes, points.device)
        prm = SearchParams.make(self.lib, **params)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        self._ready()
        self._check(self.lib.vslam_fuse_project(
            self.handle, _ptr(points), _ptr(n_points), C.c_int(S), _ptr(obs_offsets), _ptr(obs_cam), _ptr(obs_kp), _ptr(obs_desc), C.c_int(O),
            _ptr(R), _ptr(T), _ptr(n_cams), C.c_int(Cs), _ptr(xy), _ptr(desc), _ptr(n_kp), C.c_int(Kp), _ptr(cam_mask),
            Kh.ctypes.data_as(C.c_void_p), C.c_int(width), C.c_int(height), C.c_int(B), C.byref(prm), _ptr(o["found_point"]),
            _ptr(o["found_cam"]), _ptr(o["found_kp"]), _ptr(o["found_dist"]), _ptr(o["found_holder"]), C.c_int(Fs), _ptr(o["n_found"]),
            _ptr(o.get("stats"))))
        return o

    def triangulate_tracks(self, points, n_points, obs_offsets, obs_cam, obs_kp, R, T, n_cams, xy, K, out=None, want_counts=True,
                           want_info=True, **params):
        """vslam_triangulate_tracks (include/vslam_tracks.h): each of an item's points (B, S, 4) f32 triangulated from all its
        observations (CSR and cameras as cull_points takes them); params: fields of vslam_track_params over its defaults.  out: a dict
        of output tensors to write into (out_points may be `points` itself); missing ones are made, zero-filled.  Returns the dict:
        out_points (B, S, 4) f32; status (B, S) i32; counts (B, S, 2) i32 (want_counts); info (B, S, 3) f64 (want_info); stats (B, 4)
        i32."""
        import numpy as np
        torch = self.torch
        B, S, O, Cs, Kp = points.shape[0], points.shape[1], obs_cam.shape[1], R.shape[1], xy.shape[2]
        for x, dt, nm in ((points, torch.float32, "points"), (n_points, torch.int32, "n_points"), (obs_offsets, torch.int32, "obs_offsets"),
                          (obs_cam, torch.int32, "obs_cam"), (obs_kp, torch.int32, "obs_kp"), (R, torch.float64, "R"), (T, torch.float64, "T"),
                          (n_cams, torch.int32, "n_cams"), (xy, torch.float32, "xy")):
            self._dev(x, dt, nm)
        shapes = dict(out_points=((B, S, 4), torch.float32), status=((B, S), torch.int32), stats=((B, 4), torch.int32))
        if want_counts:
            shapes.update(counts=((B, S, 2), torch.int32))
        if want_info:
            shapes.update(info=((B, S, 3), torch.float64))
        o = self._outputs(out, shapes, points.device)
        prm = TrackParams.make(self.lib, **params)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        self._ready()
        self._check(self.lib.vslam_triangulate_tracks(
            self.handle, _ptr(points), _ptr(n_points), C.c_int(S), _ptr(obs_offsets), _ptr(obs_cam), _ptr(obs_kp), C.c_int(O), _ptr(R), _ptr(T),
            _ptr(n_cams), C.c_int(Cs), _ptr(xy), C.c_int(Kp), Kh.ctypes.data_as(C.c_void_p), C.c_int(B), C.byref(prm), _ptr(o["out_points"]),
            _ptr(o["status"]), _ptr(o.get("counts")), _ptr(o.get("info")), _ptr(o["stats"])))
        return o

    def places_assign(self, desc, n, vocab, out=None, want_dist=True):
        """vslam_places_assign (include/vslam_places.h): the nearest word of vocab (W, 32) u8 for every descriptor of desc
        (frames, kp_stride, 32) u8, n (frames,) i32 of them per frame.  Returns a dict: word, dist (want_dist) (frames, kp_stride) i32."""
        torch = self.torch
        Fr, Kp, W = desc.shape[0], desc.shape[1], vocab.shape[0]
        for x, dt, nm in ((desc, torch.uint8, "desc"), (n, torch.int32, "n"), (vocab, torch.uint8, "vocab")):
            self._dev(x, dt, nm)
        shapes = dict(word=((Fr, Kp), torch.int32))
        if want_dist:
            shapes.update(dist=((Fr, Kp), torch.int32))
        o = self._outputs(out, shapes, desc.device)
        self._ready()
        self._check(self.lib.vslam_places_assign(self.handle, _ptr(desc), _ptr(n), C.c_int(Kp), C.c_int(Fr), _ptr(vocab), C.c_int(W),
                                                 _ptr(o["word"]), _ptr(o.get("dist"))))
        return o

    def places_train(self, desc, n_words, iterations=4, out=None):
        """vslam_places_train (include/vslam_places.h): a vocabulary of n_words by k-majority from desc (n, 32) u8.  Returns a dict:
        vocab (n_words, 32) u8, sizes (n_words,) i32."""
        torch = self.torch
        self._dev(desc, torch.uint8, "desc")
        o = self._outputs(out, dict(vocab=((max(n_words, 0), 32), torch.uint8), sizes=((max(n_words, 0),), torch.int32)), desc.device)
        self._ready()
        self._check(self.lib.vslam_places_train(self.handle, _ptr(desc), C.c_int(desc.shape[0]), C.c_int(n_words), C.c_int(iterations),
                                                _ptr(o["vocab"]), _ptr(o["sizes"])))
        return o

    def kdtree_build(self, xy, n):
        torch = self.torch
        B, K, _ = xy.shape
        self._dev(xy, torch.float32, "xy"); self._dev(n, torch.int32, "n")
        nodes = torch.full((B, K), -1, dtype=torch.int32, device=xy.device)
        self._check(self.lib.vslam_kdtree_build(self.handle, _ptr(xy), _ptr(n), C.c_int(B), C.c_int(K), _ptr(nodes)))
        return nodes

    def kdtree_radius(self, nodes, xy, n, queries, nq, radius, hit_cap=8):
        torch = self.torch
        B, K, _ = xy.shape
        Q = queries.shape[1]
        self._dev(nodes, torch.int32, "nodes"); self._dev(xy, torch.float32, "xy"); self._dev(n, torch.int32, "n")
        self._dev(queries, torch.float32, "queries"); self._dev(nq, torch.int32, "nq")
        hits = torch.full((B, Q, hit_cap), -1, dtype=torch.int32, device=xy.device)
        counts = torch.zeros((B, Q), dtype=torch.int32, device=xy.device)
        self._check(self.lib.vslam_kdtree_radius(self.handle, _ptr(nodes), _ptr(xy), _ptr(n), C.c_int(B), C.c_int(K),
                                                 _ptr(queries), _ptr(nq), C.c_int(Q), C.c_float(radius),
                                                 _ptr(hits), _ptr(counts), C.c_int(hit_cap)))
        return hits, counts

    def kdtree_nearest(self, nodes, xy, n, queries, nq, max_distance_sq=float("inf")):
        torch = self.torch
        B, K, _ = xy.shape
        Q = queries.shape[1]
        best = torch.full((B, Q), -2, dtype=torch.int32, device=xy.device)
        self._check(self.lib.vslam_kdtree_nearest(self.handle, _ptr(nodes), _ptr(xy), _ptr(n), C.c_int(B), C.c_int(K),
                                                  _ptr(queries), _ptr(nq), C.c_int(Q), C.c_float(max_distance_sq),
                                                  _ptr(best)))
        return best

    def bgr2gray(self, bgr):
        torch = self.torch
        F, H, W, _ = bgr.shape
        self._dev(bgr, torch.uint8, "bgr")
        gray = torch.empty((F, H, W), dtype=torch.uint8, device=bgr.device)
        self._check(self.lib.vslam_bgr2gray(self.handle, _ptr(bgr), C.c_int(F), C.c_int(W), C.c_int(H), C.c_int(3 * W), _ptr(gray)))
        return gray

    def min_eigen(self, gray):
        torch = self.torch
        F, H, W = gray.shape
        self._dev(gray, torch.uint8, "gray")
        eig = torch.empty((F, H, W), dtype=torch.float32, device=gray.device)
        self._check(self.lib.vslam_min_eigen(self.handle, _ptr(gray), C.c_int(F), C.c_int(W), C.c_int(H), _ptr(eig)))
        return eig

    def good_features(self, gray, max_corners, quality=0.01, min_distance=3.0, kp_stride=None):
        torch = self.torch
        F, H, W = gray.shape
        K = kp_stride or max_corners
        self._dev(gray, torch.uint8, "gray")
        xy = torch.zeros((F, K, 2), dtype=torch.float32, device=gray.device)
        n = torch.zeros((F,), dtype=torch.int32, device=gray.device)
        self._check(self.lib.vslam_good_features(self.handle, _ptr(gray), C.c_int(F), C.c_int(W), C.c_int(H),
                                                 C.c_int(max_corners), C.c_double(quality), C.c_double(min_distance),
                                                 C.c_int(K), _ptr(xy), _ptr(n)))
        return xy, n

    def gaussian7(self, gray):
        torch = self.torch
        F, H, W = gray.shape
        self._dev(gray, torch.uint8, "gray")
        out = torch.empty_like(gray)
        self._check(self.lib.vslam_gaussian7(self.handle, _ptr(gray), C.c_int(F), C.c_int(W), C.c_int(H), _ptr(out)))
        return out

    def orb_describe(self, blurred, xy, n, cos_a, sin_a, pattern):
        torch = self.torch
        F, H, W = blurred.shape
        K = xy.shape[1]
        self._dev(blurred, torch.uint8, "blurred"); self._dev(xy, torch.float32, "xy"); self._dev(n, torch.int32, "n")
        self._dev(pattern, torch.int8, "pattern")
        xy_out = torch.zeros_like(xy)
        desc = torch.zeros((F, K, 32), dtype=torch.uint8, device=xy.device)
        n_out = torch.zeros_like(n)
        self._check(self.lib.vslam_orb_describe(self.handle, _ptr(blurred), C.c_int(F), C.c_int(W), C.c_int(H),
                                                _ptr(xy), _ptr(n), C.c_int(K), C.c_float(cos_a), C.c_float(sin_a),
                                                _ptr(pattern), _ptr(xy_out), _ptr(desc), _ptr(n_out)))
        return xy_out, desc, n_out

    def _params(self, max_corners, cos_a, sin_a, pattern, quality=0.01, min_distance=3.0):
        p = ExtractParams()
        p.max_corners = max_corners
        p.quality = quality
        p.min_distance = min_distance
        p.cos_a = cos_a
        p.sin_a = sin_a
        p.d_pattern = pattern.data_ptr() if pattern is not None else None   # NULL: ORB's learned table
        return p

    def extract_features(self, bgr, max_corners, cos_a, sin_a, pattern, kp_stride=None, out=None, width=None):
        """bgr: (F, H, W, 3), or rows with padding as (F, H, row_bytes) together with `width`."""
        torch = self.torch
        if bgr.dim() == 3:
            F, H, row_bytes = bgr.shape
            W = int(width)
            assert row_bytes >= 3 * W
        else:
            F, H, W, _ = bgr.shape
            row_bytes = 3 * W
        K = kp_stride or max_corners
        self._dev(bgr, torch.uint8, "bgr"); self._dev(pattern, torch.int8, "pattern")
        dev = bgr.device
        if out is None:
            out = dict(xy=torch.zeros((F, K, 2), dtype=torch.float32, device=dev),
                       desc=torch.zeros((F, K, 32), dtype=torch.uint8, device=dev),
                       nodes=torch.full((F, K), -1, dtype=torch.int32, device=dev),
                       n=torch.zeros((F,), dtype=torch.int32, device=dev),
                       n_detected=torch.zeros((F,), dtype=torch.int32, device=dev))
            self._ready()
        p = self._params(max_corners, cos_a, sin_a, pattern)
        self._check(self.lib.vslam_extract_features(self.handle, _ptr(bgr), C.c_int(F), C.c_int(W), C.c_int(H),
                                                    C.c_int(row_bytes), C.byref(p), C.c_int(K), _ptr(out["xy"]),
                                                    _ptr(out["desc"]), _ptr(out["nodes"]), _ptr(out["n"]),
                                                    _ptr(out["n_detected"])))
        return out

    def extract_features_grid(self, bgr, nrows, ncols, pattern, kp_stride, out=None):
        """extract_features(frame, nrows, ncols): bgr is modified in place (cell outlines)."""
        torch = self.torch
        F, H, W, _ = bgr.shape
        self._dev(bgr, torch.uint8, "bgr"); self._dev(pattern, torch.int8, "pattern")
        dev = bgr.device
        if out is None:
            out = dict(xy=torch.zeros((F, kp_stride, 2), dtype=torch.float32, device=dev),
                       desc=torch.zeros((F, kp_stride, 32), dtype=torch.uint8, device=dev),
                       angle_octave=torch.zeros((F, kp_stride, 2), dtype=torch.float32, device=dev),
                       n=torch.zeros((F,), dtype=torch.int32, device=dev))
            self._ready()
        self._check(self.lib.vslam_extract_features_grid(self.handle, _ptr(bgr), C.c_int(F), C.c_int(W), C.c_int(H),
                                                         C.c_int(3 * W), C.c_int(nrows), C.c_int(ncols), _ptr(pattern),
                                                         C.c_int(kp_stride), _ptr(out["xy"]), _ptr(out["desc"]),
                                                         _ptr(out["angle_octave"]), _ptr(out["n"])))
        return out

    def extract_Rt(self, F, best, K):
        import numpy as np
        torch = self.torch
        B = F.shape[0]
        Kh = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        R = torch.zeros((B, 9), dtype=torch.float32, device=F.device)
        t = torch.zeros((B, 3), dtype=torch.float32, device=F.device)
        c2 = torch.zeros((B, 12), dtype=torch.float32, device=F.device)
        self._check(self.lib.vslam_extract_Rt(self.handle, _ptr(F), _ptr(best), C.c_int(B), Kh.ctypes.data_as(C.c_void_p),
                                              _ptr(R), _ptr(t), _ptr(c2)))
        return R, t, c2

    def triangulate(self, xy1, xy2, matches, best, K, c2):
        import numpy as np
        torch = self.torch
        B, Kp, _ = xy1.shape
        Kh = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        pts = torch.zeros((B, Kp, 4), dtype=torch.float32, device=xy1.device)
        self._check(self.lib.vslam_triangulate(self.handle, _ptr(xy1), _ptr(xy2), _ptr(matches), _ptr(best), C.c_int(B),
                                               C.c_int(Kp), Kh.ctypes.data_as(C.c_void_p), _ptr(c2), _ptr(pts)))
        return pts

    def reprojection_filter(self, pts4d, xy1, xy2, matches, best, K, c2, ids, thr_sq=4.0):
        import numpy as np
        torch = self.torch
        B, Kp, _ = xy1.shape
        Kh = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        idx = torch.full((B, Kp), -1, dtype=torch.int32, device=xy1.device)
        n = torch.zeros((B,), dtype=torch.int32, device=xy1.device)
        err = torch.zeros((B,), dtype=torch.float64, device=xy1.device)
        self._check(self.lib.vslam_reprojection_filter(self.handle, _ptr(pts4d), _ptr(xy1), _ptr(xy2), _ptr(matches), _ptr(best),
                                                       C.c_int(B), C.c_int(Kp), Kh.ctypes.data_as(C.c_void_p), _ptr(c2), _ptr(ids),
                                                       C.c_float(thr_sq), _ptr(idx), _ptr(n), _ptr(err)))
        return idx, n, err

    def associate(self, map_points, n_map, c2, w, h, nodes, xy, desc, n, obs_offsets, obs_desc, ids, radius=2.0, thr=64, claim=None):
        torch = self.torch
        B, Mp, _ = map_points.shape
        Kp = xy.shape[1]
        if claim is None:
            claim = torch.full((B, Mp), -3, dtype=torch.int32, device=xy.device)
            self._ready()
        self._check(self.lib.vslam_associate_map_points(
            self.handle, _ptr(map_points), _ptr(n_map), C.c_int(B), C.c_int(Mp), _ptr(c2), C.c_int(w), C.c_int(h), _ptr(nodes),
            _ptr(xy), _ptr(desc), _ptr(n), C.c_int(Kp), _ptr(obs_offsets), _ptr(obs_desc), C.c_int(obs_desc.shape[1]),
            C.c_float(radius), C.c_uint32(thr), _ptr(ids), _ptr(claim)))
        return claim

    def match_features(self, xy1, desc1, n1, xy2, desc2, n2, seeds, hyp, threshold, out=None):
        torch = self.torch
        B, K, _ = xy1.shape
        dev = xy1.device
        if out is None:
            out = dict(matches=torch.zeros((B, K, 2), dtype=torch.int32, device=dev),
                       best=torch.zeros((B, 4), dtype=torch.int32, device=dev),
                       F=torch.zeros((B, 9), dtype=torch.float32, device=dev),
                       prelim_m=torch.zeros((B,), dtype=torch.int32, device=dev))
        self._check(self.lib.vslam_match_features(
            self.handle, _ptr(xy1), _ptr(desc1), _ptr(n1), _ptr(xy2), _ptr(desc2), _ptr(n2), C.c_int(B), C.c_int(K),
            _ptr(seeds), C.c_int(hyp), C.c_float(threshold), _ptr(out["matches"]), _ptr(out["best"]), _ptr(out["F"]),
            _ptr(out["prelim_m"])))
        return out

    def frontend_pairs(self, bgr, pairs, max_corners, cos_a, sin_a, pattern, seeds, hyp, threshold, kp_stride=None, out=None):
        torch = self.torch
        F, H, W, _ = bgr.shape
        assert F == 2 * pairs
        K = kp_stride or max_corners
        dev = bgr.device
        if out is None:
            out = dict(xy=torch.zeros((F, K, 2), dtype=torch.float32, device=dev),
                       desc=torch.zeros((F, K, 32), dtype=torch.uint8, device=dev),
                       nodes=torch.full((F, K), -1, dtype=torch.int32, device=dev),
                       n=torch.zeros((F,), dtype=torch.int32, device=dev),
                       matches=torch.zeros((pairs, K, 2), dtype=torch.int32, device=dev),
                       best=torch.zeros((pairs, 4), dtype=torch.int32, device=dev),
                       F=torch.zeros((pairs, 9), dtype=torch.float32, device=dev))
            self._ready()
        p = self._params(max_corners, cos_a, sin_a, pattern)
        self._check(self.lib.vslam_frontend_pairs(
            self.handle, _ptr(bgr), C.c_int(pairs), C.c_int(W), C.c_int(H), C.c_int(3 * W), C.byref(p), C.c_int(K),
            _ptr(seeds), C.c_int(hyp), C.c_float(threshold), _ptr(out["xy"]), _ptr(out["desc"]), _ptr(out["nodes"]),
            _ptr(out["n"]), _ptr(out["matches"]), _ptr(out["best"]), _ptr(out["F"])))
        return out

    def triangulate_points(self, p1, p2, c1, c2):
        """triangulate(p1, p2, c1, c2, points_4d) as the reference declares it: (n, 2) device points, host 3 x 4 matrices."""
        import numpy as np
        torch = self.torch
        n = p1.shape[0]
        pts = torch.zeros((n, 4), dtype=torch.float32, device=p1.device)
        c1h = np.ascontiguousarray(c1, dtype=np.float32).reshape(12)
        c2h = np.ascontiguousarray(c2, dtype=np.float32).reshape(12)
        self._check(self.lib.vslam_triangulate_points(self.handle, _ptr(p1), _ptr(p2), C.c_int(n), c1h.ctypes.data_as(C.c_void_p),
                                                      c2h.ctypes.data_as(C.c_void_p), _ptr(pts)))
        return pts

    def frontend_pairs_pose(self, bgr, pairs, max_corners, cos_a, sin_a, pattern, seeds, hyp, threshold, K, ids=None, thr_sq=4.0,
                            kp_stride=None, out=None):
        """frontend_pairs + extract_Rt + triangulate + reprojection filter in one call (vslam_frontend_pairs_pose)."""
        import numpy as np
        torch = self.torch
        F, H, W, _ = bgr.shape
        assert F == 2 * pairs
        Kp = kp_stride or max_corners
        dev = bgr.device
        if out is None:
            out = dict(xy=torch.zeros((F, Kp, 2), dtype=torch.float32, device=dev),
                       desc=torch.zeros((F, Kp, 32), dtype=torch.uint8, device=dev),
                       nodes=torch.full((F, Kp), -1, dtype=torch.int32, device=dev),
                       n=torch.zeros((F,), dtype=torch.int32, device=dev),
                       matches=torch.zeros((pairs, Kp, 2), dtype=torch.int32, device=dev),
                       best=torch.zeros((pairs, 4), dtype=torch.int32, device=dev),
                       F=torch.zeros((pairs, 9), dtype=torch.float32, device=dev),
                       R=torch.zeros((pairs, 9), dtype=torch.float32, device=dev),
                       t=torch.zeros((pairs, 3), dtype=torch.float32, device=dev),
                       c2=torch.zeros((pairs, 12), dtype=torch.float32, device=dev),
                       points4d=torch.zeros((pairs, Kp, 4), dtype=torch.float32, device=dev),
                       inlier_idx=torch.zeros((pairs, Kp), dtype=torch.int32, device=dev),
                       n_inliers=torch.zeros((pairs,), dtype=torch.int32, device=dev),
                       error=torch.zeros((pairs,), dtype=torch.float64, device=dev))
            self._ready()
        p = self._params(max_corners, cos_a, sin_a, pattern)
        po = PoseOutputs(*(C.c_void_p(out[k].data_ptr()) for k in ("R", "t", "c2", "points4d", "inlier_idx", "n_inliers", "error")))
        Kh = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        self._check(self.lib.vslam_frontend_pairs_pose(
            self.handle, _ptr(bgr), C.c_int(pairs), C.c_int(W), C.c_int(H), C.c_int(3 * W), C.byref(p), C.c_int(Kp),
            _ptr(seeds), C.c_int(hyp), C.c_float(threshold), _ptr(out["xy"]), _ptr(out["desc"]), _ptr(out["nodes"]),
            _ptr(out["n"]), _ptr(out["matches"]), _ptr(out["best"]), _ptr(out["F"]), Kh.ctypes.data_as(C.c_void_p), _ptr(ids),
            C.c_float(thr_sq), C.byref(po)))
        return out

    def pack_records(self, F, best, matches, out=None):
        """(P,9) f32, (P,4) i32, (P,K,2) i32 -> (P, 13 + K) i32 records (same layout as shard.pack_records)."""
        torch = self.torch
        P, K = matches.shape[0], matches.shape[1]
        if out is None:
            out = torch.empty((P, 13 + K), dtype=torch.int32, device=F.device)
        self._check(self.lib.vslam_pack_records(self.handle, _ptr(F), _ptr(best), _ptr(matches), C.c_int(P), C.c_int(K), _ptr(out)))
        return out

    def frontend_sequence(self, bgr, max_corners, cos_a, sin_a, pattern, seeds, hyp, threshold, kp_stride=None, out=None):
        """Consecutive frames: every frame extracted once, pair i = (frame i, frame i + 1); seeds has F - 1 entries."""
        torch = self.torch
        F, H, W, _ = bgr.shape
        assert F >= 2 and seeds.shape[0] == F - 1
        K = kp_stride or max_corners
        dev = bgr.device
        if out is None:
            out = dict(xy=torch.zeros((F, K, 2), dtype=torch.float32, device=dev),
                       desc=torch.zeros((F, K, 32), dtype=torch.uint8, device=dev),
                       nodes=torch.full((F, K), -1, dtype=torch.int32, device=dev),
                       n=torch.zeros((F,), dtype=torch.int32, device=dev),
                       matches=torch.zeros((F - 1, K, 2), dtype=torch.int32, device=dev),
                       best=torch.zeros((F - 1, 4), dtype=torch.int32, device=dev),
                       F=torch.zeros((F - 1, 9), dtype=torch.float32, device=dev))
            self._ready()
        p = self._params(max_corners, cos_a, sin_a, pattern)
        self._check(self.lib.vslam_frontend_sequence(
            self.handle, _ptr(bgr), C.c_int(F), C.c_int(W), C.c_int(H), C.c_int(3 * W), C.byref(p), C.c_int(K),
            _ptr(seeds), C.c_int(hyp), C.c_float(threshold), _ptr(out["xy"]), _ptr(out["desc"]), _ptr(out["nodes"]),
            _ptr(out["n"]), _ptr(out["matches"]), _ptr(out["best"]), _ptr(out["F"])))
        return out


    def track_sequences(self, pmap, bgr, max_corners, cos_a, sin_a, pattern, seeds, hyp, threshold, K, radius=2.0, dist_threshold=64,
                         thr_sq=4.0, out=None, width=None):
        """vslam_track_sequences: bgr (tracks, frames, H, W, 3), or (tracks, frames, H, row_bytes) together with `width`; seeds
        (tracks, frames - 1) int32 bit patterns.  Per-frame outputs have tracks * frames slots, per-pair outputs tracks * frames - 1
        (pair (t, f -> f + 1) at t * frames + f); the map itself is read through pmap.view() / pmap.observations()."""
        import numpy as np
        torch = self.torch
        if bgr.dim() == 4:
            T, Fr, H, row_bytes = bgr.shape
            W = int(width)
            assert row_bytes >= 3 * W
        else:
            T, Fr, H, W, _ = bgr.shape
            row_bytes = 3 * W
        assert T == pmap.tracks and tuple(seeds.shape) == (T, Fr - 1)
        Kp = pmap.kp_stride
        dev = bgr.device
        N = T * Fr
        if out is None:
            out = dict(xy=torch.zeros((N, Kp, 2), dtype=torch.float32, device=dev),
                       desc=torch.zeros((N, Kp, 32), dtype=torch.uint8, device=dev),
                       nodes=torch.full((N, Kp), -1, dtype=torch.int32, device=dev),
                       n=torch.zeros((N,), dtype=torch.int32, device=dev),
                       matches=torch.zeros((N - 1, Kp, 2), dtype=torch.int32, device=dev),
                       best=torch.zeros((N - 1, 4), dtype=torch.int32, device=dev),
                       F=torch.zeros((N - 1, 9), dtype=torch.float32, device=dev))
        self._ready()
        p = self._params(max_corners, cos_a, sin_a, pattern)
        Kh = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        self._check(self.lib.vslam_track_sequences(
            self.handle, pmap.handle, _ptr(bgr), C.c_int(Fr), C.c_int(W), C.c_int(H), C.c_int(row_bytes), C.byref(p), _ptr(seeds),
            C.c_int(hyp), C.c_float(threshold), Kh.ctypes.data_as(C.c_void_p), C.c_float(radius), C.c_uint32(dist_threshold),
            C.c_float(thr_sq), _ptr(out["xy"]), _ptr(out["desc"]), _ptr(out["nodes"]), _ptr(out["n"]), _ptr(out["matches"]),
            _ptr(out["best"]), _ptr(out["F"])))
        return out

    def render_points(self, points, colors, sizes, view, width, height, pose=None, frames=None, depth=False, row_stride=None,
                      out=None):
        """vslam_render_points: points (T, M, 4) f32, colors (T, M, 3) u8, sizes (T,) i32, pose (T, P, 16) f32 or None ->
        bgr (T, H, W, 3) u8 -- (T, H, row_stride) when row_stride is given -- and, with depth=True, (T, H, W) f32 as well.
        `out` = (bgr, depth or None) tensors to write into instead of new ones."""
        torch = self.torch
        T, M, _ = points.shape
        self._dev(points, torch.float32, "points"); self._dev(colors, torch.uint8, "colors"); self._dev(sizes, torch.int32, "sizes")
        self._dev(pose, torch.float32, "pose")
        P = pose.shape[1] if pose is not None else 0
        frames = P if frames is None else frames
        bgr, dep = self._render_outputs(T, width, height, depth, row_stride, out)
        self._check(self.lib.vslam_render_points(
            self.handle, _ptr(points), _ptr(colors), _ptr(sizes), C.c_int(T), C.c_int(M), _ptr(pose), C.c_int(frames), C.c_int(P),
            C.byref(view), C.c_int(width), C.c_int(height), C.c_int(row_stride or 3 * width), _ptr(bgr), _ptr(dep)))
        return (bgr, dep) if depth else bgr

    def _render_outputs(self, T, width, height, depth, row_stride, out):
        torch = self.torch
        if out is not None:
            return out
        shape = (T, height, width, 3) if row_stride is None else (T, height, row_stride)
        bgr = torch.empty(shape, dtype=torch.uint8, device=self.device)
        dep = torch.empty((T, height, width), dtype=torch.float32, device=self.device) if depth else None
        self._ready()
        return bgr, dep


class PointMap:
    """A vslam_map: the reference's PointMap and per-frame map_point_ids / R_t / pose for `tracks` sequences, resident on the
    context's device.  `ctx` is a Context (a Pipeline slot's context included)."""

    def __init__(self, ctx, tracks, max_frames, kp_stride, map_capacity, obs_capacity):
        self.ctx = ctx
        self.lib = ctx.lib
        self.tracks, self.max_frames, self.kp_stride = tracks, max_frames, kp_stride
        self.map_capacity, self.obs_capacity = map_capacity, obs_capacity
        self.world = None
        self.handle = C.c_void_p()
        ctx._check(self.lib.vslam_map_create(ctx.handle, C.c_int(tracks), C.c_int(max_frames), C.c_int(kp_stride),
                                             C.c_int(map_capacity), C.c_int(obs_capacity), C.byref(self.handle)))

    @classmethod
    def create(cls, ctx, tracks, max_frames, kp_stride, map_capacity, obs_capacity):
        return cls(ctx, tracks, max_frames, kp_stride, map_capacity, obs_capacity)

    def reset(self):
        self.ctx._check(self.lib.vslam_map_reset(self.ctx.handle, self.handle))

    def step(self, last, cur, pair, bgr_cur, K, radius=2.0, dist_threshold=64, thr_sq=4.0, width=None):
        """last / cur: dicts of xy, desc, nodes, n ([tracks][...] as extract_features returns them); pair: matches, best, F as
        match_features returns them; bgr_cur (tracks, H, W, 3), or (tracks, H, row_bytes) together with `width`."""
        import numpy as np
        if bgr_cur.dim() == 3:
            _, H, row_bytes = bgr_cur.shape
            W = int(width)
        else:
            _, H, W, _ = bgr_cur.shape
            row_bytes = 3 * W
        Kh = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_map_step(
            self.ctx.handle, self.handle, _ptr(last["xy"]), _ptr(last["desc"]), _ptr(last["n"]), _ptr(cur["xy"]), _ptr(cur["desc"]),
            _ptr(cur["nodes"]), _ptr(cur["n"]), _ptr(pair["matches"]), _ptr(pair["best"]), _ptr(pair["F"]), _ptr(bgr_cur),
            C.c_int(W), C.c_int(H), C.c_int(row_bytes), Kh.ctypes.data_as(C.c_void_p), C.c_float(radius),
            C.c_uint32(dist_threshold), C.c_float(thr_sq)))

    def attach_world(self, world=None, min_links=8, resection=None):
        """vslam_map_attach_world: from now on step() / track_sequences advance `world` (a new World of this map's shape when
        none is given) behind every map step and lift the appended points into its world_points; view() then carries the
        world's arrays as well.  resection: None, or a dict of vslam_resect_params fields ({} for the defaults) set on the
        world first (World.set_resection): every step then resects the frame's pose against the world's points, with the
        step's own keypoints and K.  Returns the world; it is closed after this map, or detached first (detach_world())."""
        if world is None:
            world = World(self.ctx, self.tracks, self.max_frames, self.kp_stride, min_links)
        if resection is not None:
            world.set_resection(**resection)
        self.ctx._check(self.lib.vslam_map_attach_world(self.handle, world.handle))
        self.world = world
        return world

    def detach_world(self):
        self.ctx._check(self.lib.vslam_map_attach_world(self.handle, C.c_void_p(0)))
        self.world = None

    def arrays(self):
        a = MapArrays()
        self.ctx._check(self.lib.vslam_map_view(self.handle, C.byref(a)))
        return a

    def view(self):
        """Host copies (numpy) of the state, after waiting for the context's stream (the error word is left alone)."""
        import numpy as np
        a = self.arrays()
        self.ctx._check(self.lib.vslam_ctx_wait(self.ctx.handle))
        T, Fr, Kp, M = self.tracks, self.max_frames, self.kp_stride, self.map_capacity

        def get(ptr, shape, dtype):
            h = np.empty(shape, dtype)
            self.ctx._check(self.lib.vslam_copy_d2h(self.ctx.handle, h.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(h.nbytes)))
            return h
        v = dict(frames=int(a.frames), points=get(a.d_points, (T, M, 4), np.float32), colors=get(a.d_colors, (T, M, 3), np.uint8),
                 sizes=get(a.d_sizes, (T,), np.int32), map_point_ids=get(a.d_map_point_ids, (T, Fr, Kp), np.int32),
                 R_t=get(a.d_R_t, (T, Fr, 16), np.float32), pose=get(a.d_pose, (T, Fr, 16), np.float32),
                 obs_counts=get(a.d_obs_counts, (T, M), np.int32), n_obs=get(a.d_n_obs, (T,), np.int32))
        if self.world is not None:   # the world frame beside it, under world_* names
            v.update({"world_" + k: x for k, x in self.world.view().items()})
        return v

    def render(self, view, width, height, tracks=None, depth=False, row_stride=None, out=None):
        """vslam_map_render: the map as images on the device, one per track -- all of them, or tracks = (lo, count).  Returns
        bgr (count, H, W, 3) u8 ((count, H, row_stride) when row_stride is given) and, with depth=True, (count, H, W) f32."""
        lo, count = (0, self.tracks) if tracks is None else tracks
        bgr, dep = self.ctx._render_outputs(max(count, 0), width, height, depth, row_stride, out)
        self.ctx._check(self.lib.vslam_map_render(self.ctx.handle, self.handle, C.c_int(lo), C.c_int(count), C.byref(view),
                                                  C.c_int(width), C.c_int(height), C.c_int(row_stride or 3 * width), _ptr(bgr),
                                                  _ptr(dep)))
        return (bgr, dep) if depth else bgr

    def observations(self):
        """(offsets [tracks][map_capacity + 1], frame_ids, point_ids [tracks][obs_capacity]) as cuda tensors, stream-ordered;
        slots past a track's total hold -1."""
        torch = self.ctx.torch
        dev = self.ctx.device
        off = torch.zeros((self.tracks, self.map_capacity + 1), dtype=torch.int32, device=dev)
        fr = torch.full((self.tracks, self.obs_capacity), -1, dtype=torch.int32, device=dev)
        pt = torch.full((self.tracks, self.obs_capacity), -1, dtype=torch.int32, device=dev)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_map_observations(self.ctx.handle, self.handle, _ptr(off), _ptr(fr), _ptr(pt)))
        return off, fr, pt

    def observation_descriptors(self):
        """vslam_map_observation_descriptors (include/vslam_search.h): (offsets [tracks][map_capacity + 1] i32, desc
        [tracks][obs_capacity][32] u8) as cuda tensors, stream-ordered: row o is the descriptor of the observation that
        observations() puts at row o; rows past a track's total are zero."""
        torch = self.ctx.torch
        dev = self.ctx.device
        off = torch.zeros((self.tracks, self.map_capacity + 1), dtype=torch.int32, device=dev)
        desc = torch.zeros((self.tracks, self.obs_capacity, 32), dtype=torch.uint8, device=dev)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_map_observation_descriptors(self.ctx.handle, self.handle, _ptr(off), _ptr(desc)))
        return off, desc

    def close(self):
        """Before the context's close(): vslam_map_destroy waits for the context's stream.  After it the map is not touched
        (the handle is dropped; a context that is gone cannot be waited for)."""
        if self.handle:
            if self.ctx.handle:
                self.lib.vslam_map_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class World:
    """A vslam_world: camera -> world poses, per-pair scales and the per-keypoint carry of `tracks` sequences in one coordinate
    system per track (include/vslam_amd.h, "the world frame"; tests/ref_world.py).  Stepped by hand with step() / lift(), or
    attached to a PointMap (PointMap.attach_world), which then steps it and fills world_points."""

    def __init__(self, ctx, tracks, max_frames, kp_stride, min_links=8):
        self.ctx = ctx
        self.lib = ctx.lib
        self.tracks, self.max_frames, self.kp_stride, self.min_links = tracks, max_frames, kp_stride, min_links
        self.resection = False
        self.handle = C.c_void_p()
        ctx._check(self.lib.vslam_world_create(ctx.handle, C.c_int(tracks), C.c_int(max_frames), C.c_int(kp_stride),
                                               C.c_int(min_links), C.byref(self.handle)))

    def reset(self):
        self.ctx._check(self.lib.vslam_world_reset(self.ctx.handle, self.handle))

    def adjust(self, pmap, xy, K, window=8, **params):
        """vslam_world_adjust (include/vslam_adjust.h): the last `window` frames of every track and the map points they observe
        adjusted together, in place in this world, which must be the one attached to `pmap`.  xy: the keypoints of every frame,
        (tracks * xy_frames, kp_stride, 2) or (tracks, xy_frames, kp_stride, 2) f32 as track_sequences leaves them; params: fields
        of vslam_adjust_params over its defaults.  Returns the statistics (tracks, 4) f64 (a cuda tensor)."""
        import numpy as np
        torch = self.ctx.torch
        self.ctx._dev(xy, torch.float32, "xy")
        xy_frames = xy.numel() // (self.tracks * self.kp_stride * 2)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        stats = torch.empty((self.tracks, 4), dtype=torch.float64, device=xy.device)
        prm = AdjustParams.make(self.lib, **params)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_adjust(self.ctx.handle, self.handle, pmap.handle, _ptr(xy), C.c_int(xy_frames),
                                                    Kh.ctypes.data_as(C.c_void_p), C.c_int(window), C.byref(prm), _ptr(stats)))
        return stats

    def fuse(self, pmap):
        """vslam_world_fuse (include/vslam_fuse.h): the map points of every track that share an observation fused into groups; this
        world must be the one attached to `pmap`.  Returns the statistics (tracks, 4) i32 (a cuda tensor): points taking part, groups
        with more than one member, points absorbed, entries kept."""
        torch = self.ctx.torch
        stats = torch.zeros((self.tracks, 4), dtype=torch.int32, device=self.ctx.device)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_fuse(self.ctx.handle, self.handle, pmap.handle, _ptr(stats)))
        return stats

    def cull(self, pmap, xy, K, **params):
        """vslam_world_cull (include/vslam_fuse.h): the world points their observations do not support culled; xy: the keypoints of
        every frame as adjust() takes them; params: fields of vslam_cull_params over its defaults.  Returns the statistics
        (tracks, 4) i32 (a cuda tensor): points taking part, kept, culled, good observations."""
        import numpy as np
        torch = self.ctx.torch
        self.ctx._dev(xy, torch.float32, "xy")
        xy_frames = xy.numel() // (self.tracks * self.kp_stride * 2)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        stats = torch.zeros((self.tracks, 4), dtype=torch.int32, device=xy.device)
        prm = CullParams.make(self.lib, **params)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_cull(self.ctx.handle, self.handle, pmap.handle, _ptr(xy), C.c_int(xy_frames),
                                                  Kh.ctypes.data_as(C.c_void_p), C.byref(prm), _ptr(stats)))
        return stats

    def fuse_project(self, pmap, xy, desc, n_kp, K, width, height, frames=None, search=None):
        """vslam_world_fuse_project (include/vslam_fuse_project.h): every world point searched by projection in every recorded frame
        that does not see it yet, the found pairs appended to the world's extra log, and the fusion run over the map's lists with the
        extras in them -- so that map points that never shared a keypoint become one track.  xy / desc / n_kp: the keypoints of every
        frame, (tracks, xy_frames, kp_stride, 2) f32, (.., kp_stride, 32) u8 and (tracks, xy_frames) i32; frames: (lo, hi), the
        cameras lo <= f < hi take part (None: every recorded frame); search: a dict of vslam_search_params fields over its defaults.
        Returns the statistics (tracks, 8) i32 (a cuda tensor): pairs tried, visible, proposing, found, found with a holder, written,
        extras appended by this call, extras held afterwards."""
        import numpy as np
        torch = self.ctx.torch
        self.ctx._dev(xy, torch.float32, "xy")
        self.ctx._dev(desc, torch.uint8, "desc")
        self.ctx._dev(n_kp, torch.int32, "n_kp")
        xy_frames = xy.numel() // (self.tracks * self.kp_stride * 2)
        if desc.numel() != self.tracks * xy_frames * self.kp_stride * 32 or n_kp.numel() != self.tracks * xy_frames:
            raise ValueError(f"desc / n_kp do not hold {self.tracks} x {xy_frames} frames of {self.kp_stride} keypoints")
        lo, hi = (0, int(self.arrays().frames)) if frames is None else frames
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        stats = torch.zeros((self.tracks, 8), dtype=torch.int32, device=xy.device)
        prm = SearchParams.make(self.lib, **(search or {}))
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_fuse_project(self.ctx.handle, self.handle, pmap.handle, _ptr(xy), _ptr(desc), _ptr(n_kp),
                                                          C.c_int(xy_frames), Kh.ctypes.data_as(C.c_void_p), C.c_int(width), C.c_int(height),
                                                          C.c_int(lo), C.c_int(hi), C.byref(prm), _ptr(stats)))
        return stats

    def retriangulate(self, pmap, xy, K, want_status=True, **params):
        """vslam_world_retriangulate (include/vslam_tracks.h): every world point triangulated anew from all the observations of its
        row of the world's CSR, in place; xy: the keypoints of every frame as adjust() takes them; params: fields of
        vslam_track_params over its defaults.  Returns (status (tracks, map_capacity) i32 or None, stats (tracks, 4) i32: points
        taking part, OK, low parallax, other refusals), cuda tensors."""
        import numpy as np
        torch = self.ctx.torch
        self.ctx._dev(xy, torch.float32, "xy")
        xy_frames = xy.numel() // (self.tracks * self.kp_stride * 2)
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        stats = torch.zeros((self.tracks, 4), dtype=torch.int32, device=xy.device)
        status = torch.zeros((self.tracks, pmap.map_capacity), dtype=torch.int32, device=xy.device) if want_status else None
        prm = TrackParams.make(self.lib, **params)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_retriangulate(self.ctx.handle, self.handle, pmap.handle, _ptr(xy), C.c_int(xy_frames),
                                                           Kh.ctypes.data_as(C.c_void_p), C.byref(prm), _ptr(status), _ptr(stats)))
        return status, stats

    def observations(self, pmap, desc=True):
        """vslam_world_observations (include/vslam_fuse.h): the CSR of the map's observations as this world sees it -- merged once a
        fusion exists, the map's own otherwise --: (offsets [tracks][map_capacity + 1], frame_ids, point_ids [tracks][obs_capacity]
        i32, desc [tracks][obs_capacity][32] u8 or None) as cuda tensors, stream-ordered; slots past a track's total hold -1 / 0."""
        torch = self.ctx.torch
        dev = self.ctx.device
        off = torch.zeros((self.tracks, pmap.map_capacity + 1), dtype=torch.int32, device=dev)
        fr = torch.full((self.tracks, pmap.obs_capacity), -1, dtype=torch.int32, device=dev)
        pt = torch.full((self.tracks, pmap.obs_capacity), -1, dtype=torch.int32, device=dev)
        d = torch.zeros((self.tracks, pmap.obs_capacity, 32), dtype=torch.uint8, device=dev) if desc else None
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_observations(self.ctx.handle, self.handle, pmap.handle, _ptr(off), _ptr(fr), _ptr(pt), _ptr(d)))
        return off, fr, pt, d

    def search(self, pmap, cur, K, width, height, resect=None, **params):
        """vslam_world_search (include/vslam_search.h): every track's world points searched by projection, from the pose of the last
        frame recorded, in the frame `cur` (a dict of xy (tracks, kp_stride, 2) f32, desc (tracks, kp_stride, 32) u8, n (tracks,)
        i32); this world must be the one attached to `pmap`.  params: fields of vslam_search_params over its defaults.  resect:
        None (search only: nothing but the outputs is written), or a dict of vslam_resect_params fields ({} for the defaults): the
        frame's pose is then resected against what was found and, where that moved it, written back with the carry.  Returns a
        dict of cuda tensors: corr_point, corr_kp (tracks, kp_stride) i32, n_corr (tracks,) i32 and, with resect, stats
        (tracks, 4) f64."""
        import numpy as np
        torch = self.ctx.torch
        xy, desc, n = (self.ctx._dev(cur[k], dt, k) for k, dt in (("xy", torch.float32), ("desc", torch.uint8), ("n", torch.int32)))
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        out = dict(corr_point=torch.zeros((self.tracks, self.kp_stride), dtype=torch.int32, device=xy.device),
                   corr_kp=torch.zeros((self.tracks, self.kp_stride), dtype=torch.int32, device=xy.device),
                   n_corr=torch.zeros((self.tracks,), dtype=torch.int32, device=xy.device))
        if resect is not None:
            out["stats"] = torch.zeros((self.tracks, 4), dtype=torch.float64, device=xy.device)
        sprm = SearchParams.make(self.lib, **params)
        rprm = ResectParams.make(self.lib, **resect) if resect is not None else None
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_search(
            self.ctx.handle, self.handle, pmap.handle, _ptr(xy), _ptr(desc), _ptr(n), Kh.ctypes.data_as(C.c_void_p), C.c_int(width),
            C.c_int(height), C.byref(sprm), C.byref(rprm) if rprm is not None else C.c_void_p(0), _ptr(out["corr_point"]),
            _ptr(out["corr_kp"]), _ptr(out["n_corr"]), _ptr(out.get("stats"))))
        return out

    def relocalise(self, pmap, cur, K, seeds=None, polish={}, match=None, **params):
        """vslam_world_relocalise (include/vslam_pnp.h): the pose of the frame `cur` (a dict of xy (tracks, kp_stride, 2) f32, desc
        (tracks, kp_stride, 32) u8, n (tracks,) i32) of every track found from the map alone -- the last recorded pose is not
        read --: the world's points matched to the keypoints by descriptor, P3P RANSAC over the matches, the polish (a dict of
        vslam_resect_params fields, {} for the defaults, None for none), and for the tracks that were found the write-back of
        search().  This world must be the one attached to `pmap`.  seeds: (tracks,) i32 bits, 1 .. tracks when None; params: fields of
        vslam_pnp_params over its defaults; match: a dict of vslam_match_params fields.  Returns a dict of cuda tensors: found,
        winner, n_inliers, n_corr (tracks,) i32; corr_point, corr_kp (tracks, kp_stride) i32; stats (tracks, 4) f64."""
        import numpy as np
        torch = self.ctx.torch
        xy, desc, n = (self.ctx._dev(cur[k], dt, k) for k, dt in (("xy", torch.float32), ("desc", torch.uint8), ("n", torch.int32)))
        if seeds is None:
            seeds = torch.arange(1, self.tracks + 1, dtype=torch.int32, device=xy.device)
        self.ctx._dev(seeds, torch.int32, "seeds")
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        i32 = dict(dtype=torch.int32, device=xy.device)
        out = dict(found=torch.zeros((self.tracks,), **i32), winner=torch.zeros((self.tracks,), **i32),
                   n_inliers=torch.zeros((self.tracks,), **i32), corr_point=torch.zeros((self.tracks, self.kp_stride), **i32),
                   corr_kp=torch.zeros((self.tracks, self.kp_stride), **i32), n_corr=torch.zeros((self.tracks,), **i32),
                   stats=torch.zeros((self.tracks, 4), dtype=torch.float64, device=xy.device))
        mprm = MatchParams.make(self.lib, **(match or {}))
        pprm = PnpParams.make(self.lib, **params)
        rprm = ResectParams.make(self.lib, **polish) if polish is not None else None
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_relocalise(
            self.ctx.handle, self.handle, pmap.handle, _ptr(xy), _ptr(desc), _ptr(n), Kh.ctypes.data_as(C.c_void_p), _ptr(seeds),
            C.byref(mprm), C.byref(pprm), C.byref(rprm) if rprm is not None else C.c_void_p(0), _ptr(out["found"]), _ptr(out["winner"]),
            _ptr(out["n_inliers"]), _ptr(out["corr_point"]), _ptr(out["corr_kp"]), _ptr(out["n_corr"]), _ptr(out["stats"])))
        return out

    def sim3(self, pmap, pairs, matches, n_matches, xy_a, xy_b, K, seeds=None, polish=None, want_points=True, **params):
        """vslam_world_sim3 (include/vslam_sim3.h): the similarity between two recorded frames' maps for each row (track_a, frame_a,
        track_b, frame_b) of pairs (items, 4) i32, from matches (items, kp_stride, 2) i32 / n_matches (items,) i32 as match_features
        writes them (first: a keypoint of frame a) and the two frames' keypoints xy_a, xy_b (items, kp_stride, 2) f32.  This world
        must be the one attached to `pmap`; nothing is written into either.  seeds: (items,) i32 bits, 1 .. items when None; polish:
        None (the default: no polish -- it cannot see the scale when both frames share a camera centre) or a dict of
        vslam_resect_params fields ({} the defaults); params: fields of vslam_sim3_params.  Returns a dict
        of cuda tensors: scale (items,), R (items, 9), T (items, 3) f64 camera a -> camera b; s_w, R_w, t_w likewise, world b ->
        world a (both written where found, zero elsewhere); found, n_corr, n_inliers, winner (items,) i32; point_a, point_b
        (items, kp_stride) i32 (want_points); stats (items, 4) f64."""
        import numpy as np
        torch = self.ctx.torch
        for x, dt, nm in ((pairs, torch.int32, "pairs"), (matches, torch.int32, "matches"), (n_matches, torch.int32, "n_matches"),
                          (xy_a, torch.float32, "xy_a"), (xy_b, torch.float32, "xy_b")):
            self.ctx._dev(x, dt, nm)
        items = pairs.shape[0]
        cols = [pairs[:, k].contiguous() for k in range(4)]
        if seeds is None:
            seeds = torch.arange(1, items + 1, dtype=torch.int32, device=pairs.device)
        self.ctx._dev(seeds, torch.int32, "seeds")
        Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        i32, f64 = dict(dtype=torch.int32, device=pairs.device), dict(dtype=torch.float64, device=pairs.device)
        out = dict(scale=torch.zeros((items,), **f64), R=torch.zeros((items, 9), **f64), T=torch.zeros((items, 3), **f64),
                   s_w=torch.zeros((items,), **f64), R_w=torch.zeros((items, 9), **f64), t_w=torch.zeros((items, 3), **f64),
                   found=torch.zeros((items,), **i32), n_corr=torch.zeros((items,), **i32), n_inliers=torch.zeros((items,), **i32),
                   winner=torch.zeros((items,), **i32), stats=torch.zeros((items, 4), **f64))
        if want_points:
            out.update(point_a=torch.full((items, self.kp_stride), -1, **i32), point_b=torch.full((items, self.kp_stride), -1, **i32))
        prm = Sim3Params.make(self.lib, **params)
        rprm = ResectParams.make(self.lib, **polish) if polish is not None else None
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_sim3(
            self.ctx.handle, self.handle, pmap.handle, *(_ptr(c) for c in cols), C.c_int(items), _ptr(matches), _ptr(n_matches), _ptr(xy_a),
            _ptr(xy_b), Kh.ctypes.data_as(C.c_void_p), _ptr(seeds), C.byref(prm), C.byref(rprm) if rprm is not None else C.c_void_p(0),
            _ptr(out["scale"]), _ptr(out["R"]), _ptr(out["T"]), _ptr(out["s_w"]), _ptr(out["R_w"]), _ptr(out["t_w"]), _ptr(out["found"]),
            _ptr(out["n_corr"]), _ptr(out["n_inliers"]), _ptr(out["winner"]), _ptr(out.get("point_a")), _ptr(out.get("point_b")),
            _ptr(out["stats"])))
        return out

    def apply_sim3(self, pmap, tracks, s, R, t, apply=None):
        """vslam_world_apply_sim3 (include/vslam_sim3.h): every listed track's world -- poses, scales, carry, world points --
        carried through X' = s R X + t, in place.  tracks: a host sequence of distinct track indices; s (items,), R (items, 9), t
        (items, 3) f64 and apply (items,) i32 (None: all ones) cuda tensors."""
        import numpy as np
        torch = self.ctx.torch
        h = np.ascontiguousarray(np.asarray(tracks, np.int32).reshape(-1))
        if apply is None:
            apply = torch.ones((len(h),), dtype=torch.int32, device=s.device)
        for x, dt, nm in ((s, torch.float64, "s"), (R, torch.float64, "R"), (t, torch.float64, "t"), (apply, torch.int32, "apply")):
            self.ctx._dev(x, dt, nm)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_apply_sim3(self.ctx.handle, self.handle, pmap.handle, h.ctypes.data_as(C.c_void_p), _ptr(s), _ptr(R),
                                                        _ptr(t), _ptr(apply), C.c_int(len(h))))

    def close_loops(self, pmap, loops, scale, R, T, use=None, seq_weight=None, loop_weight=None, **params):
        """vslam_world_close_loops (include/vslam_graph.h): every track's frames, scales, carry and world points moved so that the
        loops close, the error spread over the frames in between; this world must be the one attached to `pmap`.  loops: (items, 3)
        i32 rows (track, frame_a, frame_b); scale (items,), R (items, 9), T (items, 3) f64: the camera a -> camera b model of each, as
        sim3() returns it for a same-track item; use (items,) i32 (None: all ones); seq_weight / loop_weight: three host numbers each
        (None: 1 1 1); params: fields of vslam_graph_params.  Returns the statistics (tracks, 4) f64 (a cuda tensor)."""
        import numpy as np
        torch = self.ctx.torch
        items = loops.shape[0]
        if use is None:
            use = torch.ones((items,), dtype=torch.int32, device=loops.device)
        for x, dt, nm in ((loops, torch.int32, "loops"), (use, torch.int32, "use"), (scale, torch.float64, "scale"), (R, torch.float64, "R"),
                          (T, torch.float64, "T")):
            self.ctx._dev(x, dt, nm)
        cols = [loops[:, k].contiguous() for k in range(3)]
        wts = [None if w is None else np.ascontiguousarray(np.asarray(w, np.float64).reshape(3)) for w in (seq_weight, loop_weight)]
        stats = torch.empty((self.tracks, 4), dtype=torch.float64, device=loops.device)
        prm = GraphParams.make(self.lib, **params)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_close_loops(
            self.ctx.handle, self.handle, pmap.handle, *(_ptr(c) for c in cols), _ptr(use), _ptr(scale), _ptr(R), _ptr(T), C.c_int(items),
            *(w.ctypes.data_as(C.c_void_p) if w is not None else C.c_void_p(0) for w in wts), C.byref(prm), _ptr(stats)))
        return stats

    def set_resection(self, enable=True, **params):
        """vslam_world_set_resection (include/vslam_resect.h), allowed at frame 0 only: from now on step() takes xy_cur and K
        and resects each frame's pose against the carry; params: fields of vslam_resect_params over its defaults.
        enable=False clears it."""
        prm = ResectParams.make(self.lib, **params) if enable else None
        self.ctx._check(self.lib.vslam_world_set_resection(self.handle, C.byref(prm) if enable else C.c_void_p(0)))
        self.resection = bool(enable)

    def step(self, matches, best, points4d, R, t, n_last, n_cur, xy_cur=None, K=None):
        """vslam_world_step: matches (T, K, 2) i32, best (T, 4) i32, points4d (T, K, 4) f32, R (T, 9) f32, t (T, 3) f32,
        n_last / n_cur (T,) i32 -- cuda tensors (None is passed on as a null pointer).  With xy_cur (T, K, 2) f32 and K (the
        3 x 3 camera matrix, host): vslam_world_step_resect, the step of a world with resection set."""
        self.ctx._ready()
        if xy_cur is not None or K is not None:
            import numpy as np
            Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9)) if K is not None else None
            self.ctx._check(self.lib.vslam_world_step_resect(
                self.ctx.handle, self.handle, _ptr(matches), _ptr(best), _ptr(points4d), _ptr(R), _ptr(t), _ptr(n_last), _ptr(n_cur),
                _ptr(xy_cur), Kh.ctypes.data_as(C.c_void_p) if Kh is not None else C.c_void_p(0)))
            return
        self.ctx._check(self.lib.vslam_world_step(self.ctx.handle, self.handle, _ptr(matches), _ptr(best), _ptr(points4d), _ptr(R),
                                                  _ptr(t), _ptr(n_last), _ptr(n_cur)))

    def lift(self, frame, points, lo, hi, out=None):
        """vslam_world_lift: rows [lo[t], hi[t]) of points (T, N, 4) f32, points of pair (frame - 1 -> frame), into `out` (a new
        zero tensor when none is given); other rows keep their bits."""
        if out is None:
            out = self.ctx.torch.zeros_like(points)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_world_lift(self.ctx.handle, self.handle, C.c_int(frame), _ptr(points),
                                                  C.c_int(points.shape[1] if points is not None else 0), _ptr(lo), _ptr(hi),
                                                  _ptr(out)))
        return out

    def arrays(self):
        a = WorldArrays()
        self.ctx._check(self.lib.vslam_world_view(self.handle, C.byref(a)))
        return a

    def view(self):
        """Host copies (numpy) of the state, after waiting for the context's stream (the error word is left alone)."""
        import numpy as np
        a = self.arrays()
        self.ctx._check(self.lib.vslam_ctx_wait(self.ctx.handle))
        T, Fr, Kp = self.tracks, self.max_frames, self.kp_stride

        def get(ptr, shape, dtype):
            h = np.empty(shape, dtype)
            self.ctx._check(self.lib.vslam_copy_d2h(self.ctx.handle, h.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(h.nbytes)))
            return h
        v = dict(frames=int(a.frames), Twc=get(a.d_Twc, (T, Fr, 16), np.float64), pose=get(a.d_pose, (T, Fr, 16), np.float32),
                 scale=get(a.d_scale, (T, Fr), np.float64), links=get(a.d_links, (T, Fr), np.int32),
                 carry=get(a.d_carry, (T, Kp, 3), np.float64), carry_index=get(a.d_carry_index, (T, Kp), np.int32))
        if a.d_world_points:
            v["points"] = get(a.d_world_points, (T, int(a.map_capacity), 4), np.float32)
        stats = C.c_void_p()
        self.ctx._check(self.lib.vslam_world_resection_view(self.handle, C.byref(stats)))
        if stats.value:   # PointMap.view() shows it as world_resect_stats
            v["resect_stats"] = get(stats.value, (T, Fr, 4), np.float64)
        fuse_to = C.c_void_p()
        self.ctx._check(self.lib.vslam_world_fusion_view(self.handle, C.byref(fuse_to), C.c_void_p(0)))
        if fuse_to.value:   # only while a fusion exists; PointMap.view() shows it as world_fuse_to
            v["fuse_to"] = get(fuse_to.value, (T, int(a.map_capacity)), np.int32)
        log = [C.c_void_p() for _ in range(5)]
        cap = C.c_int32()
        self.ctx._check(self.lib.vslam_world_fuse_project_view(self.handle, *(C.byref(p) for p in log), C.byref(cap)))
        if log[4].value:   # only while extras exist (include/vslam_fuse_project.h); PointMap.view() shows it as world_extra
            O = int(cap.value)
            v["extra"] = dict(point=get(log[0].value, (T, O), np.int32), frame=get(log[1].value, (T, O), np.int32),
                              kp=get(log[2].value, (T, O), np.int32), desc=get(log[3].value, (T, O, 32), np.uint8),
                              n=get(log[4].value, (T,), np.int32))
        return v

    def render(self, pmap, view, width, height, tracks=None, depth=False, row_stride=None, out=None):
        """vslam_world_render: PointMap.render's images in the world frame (world_points, the map's colours, the world's poses)."""
        lo, count = (0, self.tracks) if tracks is None else tracks
        bgr, dep = self.ctx._render_outputs(max(count, 0), width, height, depth, row_stride, out)
        self.ctx._check(self.lib.vslam_world_render(self.ctx.handle, self.handle, pmap.handle, C.c_int(lo), C.c_int(count),
                                                    C.byref(view), C.c_int(width), C.c_int(height),
                                                    C.c_int(row_stride or 3 * width), _ptr(bgr), _ptr(dep)))
        return (bgr, dep) if depth else bgr

    def close(self):
        """After the map it is attached to and before the context's close()."""
        if self.handle:
            if self.ctx.handle:
                self.lib.vslam_world_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Places:
    """A vslam_places (include/vslam_places.h): an index of frames as bags of binary words, queried for the entries that look like a
    frame.  tests/ref_places.py restates it."""

    def __init__(self, ctx, n_words, capacity, max_kp):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_words, self.capacity, self.max_kp = n_words, capacity, max_kp
        self.handle = C.c_void_p()
        ctx._check(self.lib.vslam_places_create(ctx.handle, C.c_int(n_words), C.c_int(capacity), C.c_int(max_kp), C.byref(self.handle)))

    def _i32(self, t, name):
        return self.ctx._dev(t, self.ctx.torch.int32, name)

    def reset(self):
        self.ctx._check(self.lib.vslam_places_reset(self.ctx.handle, self.handle))

    def set_vocabulary(self, vocab, weights=None):
        """vocab (n_words, 32) u8; weights (n_words,) i32 or None (all 1).  Only while the index is empty."""
        self.ctx._dev(vocab, self.ctx.torch.uint8, "vocab")
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_places_set_vocabulary(self.ctx.handle, self.handle, _ptr(vocab), _ptr(self._i32(weights, "weights"))))

    def set_weights(self, weights=None):
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_places_set_weights(self.ctx.handle, self.handle, _ptr(self._i32(weights, "weights"))))

    def add(self, desc, n, tags=None, out=None):
        """desc (frames, kp_stride, 32) u8, n (frames,) i32, tags (frames, 2) i32 or None.  Returns the ids (frames,) i32."""
        torch = self.ctx.torch
        self.ctx._dev(desc, torch.uint8, "desc")
        Fr, Kp = desc.shape[0], desc.shape[1]
        ids = out if out is not None else torch.zeros((Fr,), dtype=torch.int32, device=desc.device)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_places_add(self.ctx.handle, self.handle, _ptr(desc), _ptr(self._i32(n, "n")), C.c_int(Kp), C.c_int(Fr),
                                                  _ptr(self._i32(tags, "tags")), _ptr(self._i32(ids, "ids"))))
        return ids

    def query(self, desc, n, top_k=1, below=None, out=None):
        """desc (queries, kp_stride, 32) u8, n (queries,) i32, below (queries,) i32 or None.  Returns a dict: best_id, best_score,
        best_den (queries, top_k) i32 and q_norm (queries,) i32."""
        torch = self.ctx.torch
        self.ctx._dev(desc, torch.uint8, "desc")
        Q, Kp, k = desc.shape[0], desc.shape[1], max(top_k, 0)
        o = self.ctx._outputs(out, dict(best_id=((Q, k), torch.int32), best_score=((Q, k), torch.int32), best_den=((Q, k), torch.int32),
                                        q_norm=((Q,), torch.int32)), desc.device)
        self.ctx._ready()
        self.ctx._check(self.lib.vslam_places_query(self.ctx.handle, self.handle, _ptr(desc), _ptr(self._i32(n, "n")), C.c_int(Kp), C.c_int(Q),
                                                    _ptr(self._i32(below, "below")), C.c_int(top_k), _ptr(o["best_id"]), _ptr(o["best_score"]),
                                                    _ptr(o["best_den"]), _ptr(o["q_norm"])))
        return o

    def arrays(self):
        a = PlacesArrays()
        self.ctx._check(self.lib.vslam_places_view(self.ctx.handle, self.handle, C.byref(a)))
        return a

    def view(self):
        """Host copies (numpy) of the index, after waiting for the context's stream: size, offsets (size + 1,), words, tf (nnz,),
        df (n_words,), norms (size,) under the current weights, tags (size, 2), weights (n_words,), vocab (n_words, 32)."""
        import numpy as np
        a = self.arrays()
        self.ctx._check(self.lib.vslam_ctx_wait(self.ctx.handle))

        def get(ptr, shape, dtype=np.int32):
            h = np.empty(shape, dtype)
            if h.nbytes:
                self.ctx._check(self.lib.vslam_copy_d2h(self.ctx.handle, h.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(h.nbytes)))
            return h
        size, W = int(a.size), int(a.n_words)
        offsets = get(a.d_offsets, (size + 1,))
        nnz = int(offsets[size])
        return dict(size=size, offsets=offsets, words=get(a.d_words, (nnz,)), tf=get(a.d_tf, (nnz,)), df=get(a.d_df, (W,)),
                    norms=get(a.d_norms, (size,)), tags=get(a.d_tags, (size, 2)), weights=get(a.d_weights, (W,)),
                    vocab=get(a.d_vocab, (W, 32), np.uint8))

    def close(self):
        """Before the context's close()."""
        if self.handle:
            if self.ctx.handle:
                self.lib.vslam_places_destroy(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiDevice:
    """ctypes stub of vslam_multi_* (include/vslam_amd.h): one process, several device slots, host arrays in and out."""

    def __init__(self, devices, lib=None):
        self.lib = lib or load_library()
        self.lib.vslam_multi_last_error.restype = C.c_char_p
        self.lib.vslam_multi_ctx.restype = C.c_void_p
        arr = (C.c_int * len(devices))(*devices)
        self.handle = C.c_void_p()
        rc = self.lib.vslam_multi_create(arr, C.c_int(len(devices)), C.byref(self.handle))
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: vslam_multi_create({list(devices)})")

    def size(self):
        return self.lib.vslam_multi_size(self.handle)

    def set_option(self, option, value):
        for i in range(self.size()):
            ctx = C.c_void_p(self.lib.vslam_multi_ctx(self.handle, C.c_int(i)))
            rc = self.lib.vslam_ctx_set_option(ctx, C.c_int(option), C.c_int(int(value)))
            if rc != OK:
                raise VslamError(f"{ERRORS.get(rc, rc)}: set_option")

    def frontend_pairs(self, last, cur, max_corners, cos_a, sin_a, pattern, base_seed, hyp, threshold):
        """last / cur: numpy uint8 (P, H, W, 3); pattern: numpy int8 (256, 4) or None.  Returns (records (P, 13 + K) int32,
        keypoint counts (2 P,) int32)."""
        import numpy as np
        P, H, W, _ = last.shape
        last = np.ascontiguousarray(last, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        p = ExtractParams()
        p.max_corners, p.quality, p.min_distance, p.cos_a, p.sin_a, p.d_pattern = max_corners, 0.01, 3.0, cos_a, sin_a, None
        rec = np.zeros((P, 13 + max_corners), np.int32)
        n = np.zeros(2 * P, np.int32)
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8)
        rc = self.lib.vslam_multi_frontend_pairs(
            self.handle, last.ctypes.data_as(C.c_void_p), cur.ctypes.data_as(C.c_void_p), C.c_int(P), C.c_int(W), C.c_int(H),
            C.c_int(3 * W), C.byref(p), pat.ctypes.data_as(C.c_void_p) if pat is not None else C.c_void_p(0), C.c_int(max_corners),
            C.c_uint32(base_seed & 0xFFFFFFFF), C.c_int(hyp), C.c_float(threshold), rec.ctypes.data_as(C.c_void_p),
            n.ctypes.data_as(C.c_void_p))
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: {self.lib.vslam_multi_last_error(self.handle).decode()}")
        return rec, n

    def frontend_pairs_resident(self, slices, pairs, max_corners, cos_a, sin_a, pattern, base_seed, hyp, threshold):
        """slices[r]: torch uint8 (2 * ps, H, W, 3) ALREADY on slot r's device = the slot's `last` frames then its `current` ones
        (None for an empty slice).  Returns (records, keypoint counts) like frontend_pairs."""
        import numpy as np
        shape = next(t.shape for t in slices if t is not None)
        H, W = int(shape[1]), int(shape[2])
        p = ExtractParams()
        p.max_corners, p.quality, p.min_distance, p.cos_a, p.sin_a, p.d_pattern = max_corners, 0.01, 3.0, cos_a, sin_a, None
        rec = np.zeros((pairs, 13 + max_corners), np.int32)
        n = np.zeros(2 * pairs, np.int32)
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8)
        ptrs = (C.c_void_p * len(slices))(*[(t.data_ptr() if t is not None else None) for t in slices])
        rc = self.lib.vslam_multi_frontend_pairs_resident(
            self.handle, ptrs, C.c_int(pairs), C.c_int(W), C.c_int(H), C.c_int(3 * W), C.byref(p),
            pat.ctypes.data_as(C.c_void_p) if pat is not None else C.c_void_p(0), C.c_int(max_corners),
            C.c_uint32(base_seed & 0xFFFFFFFF), C.c_int(hyp), C.c_float(threshold), rec.ctypes.data_as(C.c_void_p),
            n.ctypes.data_as(C.c_void_p))
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: {self.lib.vslam_multi_last_error(self.handle).decode()}")
        return rec, n

    def close(self):
        if self.handle:
            self.lib.vslam_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """ctypes stub of vslam_pipeline_* (include/vslam_amd.h): k contexts on one device, batches handed to them round-robin.

    `acquire()` returns (ticket, Context view of the slot's vslam_ctx); enqueue the batch on it, then `commit(ticket)`.
    `submit_pairs` is the one-call form.  Output tensors are the caller's: keep one set per batch in flight, alive until the
    batch has been waited for, and complete on torch's side before they are handed over (the contexts run on streams of their
    own that do not wait for torch's: `alloc_outputs` synchronizes, inputs made with torch kernels need the same)."""

    class _Borrowed(Context):
        """A Context object over a vslam_ctx the pipeline owns (never destroyed from here)."""

        def __init__(self, lib, handle, device):   # noqa: no super().__init__: nothing is created
            import torch
            self.torch = torch
            self.lib = lib
            self.handle = C.c_void_p(handle)
            self.device = torch.device("cuda", device)

        def close(self):
            self.handle = C.c_void_p()

    def __init__(self, device=0, n_ctx=3, lib=None):
        self.lib = lib or load_library()
        self.lib.vslam_pipeline_last_error.restype = C.c_char_p
        self.lib.vslam_pipeline_ctx.restype = C.c_void_p
        self.handle = C.c_void_p()
        rc = self.lib.vslam_pipeline_create(C.c_int(device), C.c_int(n_ctx), C.byref(self.handle))
        if rc != OK:
            raise VslamError(f"vslam_pipeline_create({device}, {n_ctx}) failed: {ERRORS.get(rc, rc)}")
        self.device = device
        self.contexts = [self._Borrowed(self.lib, self.lib.vslam_pipeline_ctx(self.handle, C.c_int(i)), device)
                         for i in range(self.size())]

    def size(self):
        return self.lib.vslam_pipeline_size(self.handle)

    def _check(self, rc):
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: {self.lib.vslam_pipeline_last_error(self.handle).decode()}")

    def set_option(self, option, value):
        self._check(self.lib.vslam_pipeline_set_option(self.handle, C.c_int(option), C.c_int(int(value))))

    def acquire(self):
        ctx = C.c_void_p()
        t = C.c_int64()
        self._check(self.lib.vslam_pipeline_acquire(self.handle, C.byref(ctx), C.byref(t)))
        return t.value, self.contexts[t.value % len(self.contexts)]

    def commit(self, ticket):
        self._check(self.lib.vslam_pipeline_commit(self.handle, C.c_int64(ticket)))

    def submit_pairs(self, bgr, pairs, max_corners, cos_a, sin_a, pattern, seeds, hyp, threshold, out, records=None, kp_stride=None):
        F, H, W, _ = bgr.shape
        assert F == 2 * pairs
        K = kp_stride or max_corners
        p = self.contexts[0]._params(max_corners, cos_a, sin_a, pattern)
        t = C.c_int64()
        self._check(self.lib.vslam_pipeline_submit_pairs(
            self.handle, _ptr(bgr), C.c_int(pairs), C.c_int(W), C.c_int(H), C.c_int(3 * W), C.byref(p), C.c_int(K), _ptr(seeds),
            C.c_int(hyp), C.c_float(threshold), _ptr(out["xy"]), _ptr(out["desc"]), _ptr(out.get("nodes")), _ptr(out["n"]),
            _ptr(out["matches"]), _ptr(out["best"]), _ptr(out["F"]), _ptr(records), C.byref(t)))
        return t.value

    def submit_pairs_pose(self, bgr, pairs, max_corners, cos_a, sin_a, pattern, seeds, hyp, threshold, K, out, ids=None, thr_sq=4.0,
                          records=None, kp_stride=None):
        """vslam_pipeline_submit_pairs_pose: `out` = alloc_outputs(...) plus the pose arrays (alloc_pose_outputs)."""
        import numpy as np
        F, H, W, _ = bgr.shape
        assert F == 2 * pairs
        Kp = kp_stride or max_corners
        p = self.contexts[0]._params(max_corners, cos_a, sin_a, pattern)
        po = PoseOutputs(*(C.c_void_p(out[k].data_ptr()) for k in ("R", "t", "c2", "points4d", "inlier_idx", "n_inliers", "error")))
        Kh = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        t = C.c_int64()
        self._check(self.lib.vslam_pipeline_submit_pairs_pose(
            self.handle, _ptr(bgr), C.c_int(pairs), C.c_int(W), C.c_int(H), C.c_int(3 * W), C.byref(p), C.c_int(Kp), _ptr(seeds),
            C.c_int(hyp), C.c_float(threshold), _ptr(out["xy"]), _ptr(out["desc"]), _ptr(out.get("nodes")), _ptr(out["n"]),
            _ptr(out["matches"]), _ptr(out["best"]), _ptr(out["F"]), Kh.ctypes.data_as(C.c_void_p), _ptr(ids), C.c_float(thr_sq),
            C.byref(po), _ptr(records), C.byref(t)))
        return t.value

    @staticmethod
    def alloc_pose_outputs(torch, frames, pairs, K, device):
        """alloc_outputs + the arrays of vslam_pose_outputs, ready for a context's own stream."""
        out = Pipeline._alloc_outputs(torch, frames, pairs, K, device)
        out.update(R=torch.zeros((pairs, 9), dtype=torch.float32, device=device), t=torch.zeros((pairs, 3), dtype=torch.float32, device=device),
                   c2=torch.zeros((pairs, 12), dtype=torch.float32, device=device),
                   points4d=torch.zeros((pairs, K, 4), dtype=torch.float32, device=device),
                   inlier_idx=torch.zeros((pairs, K), dtype=torch.int32, device=device),
                   n_inliers=torch.zeros((pairs,), dtype=torch.int32, device=device),
                   error=torch.zeros((pairs,), dtype=torch.float64, device=device))
        torch.cuda.current_stream(device).synchronize()
        return out

    def submit_sequence(self, bgr, max_corners, cos_a, sin_a, pattern, seeds, hyp, threshold, out, records=None, kp_stride=None):
        F, H, W, _ = bgr.shape
        K = kp_stride or max_corners
        p = self.contexts[0]._params(max_corners, cos_a, sin_a, pattern)
        t = C.c_int64()
        self._check(self.lib.vslam_pipeline_submit_sequence(
            self.handle, _ptr(bgr), C.c_int(F), C.c_int(W), C.c_int(H), C.c_int(3 * W), C.byref(p), C.c_int(K), _ptr(seeds),
            C.c_int(hyp), C.c_float(threshold), _ptr(out["xy"]), _ptr(out["desc"]), _ptr(out.get("nodes")), _ptr(out["n"]),
            _ptr(out["matches"]), _ptr(out["best"]), _ptr(out["F"]), _ptr(records), C.byref(t)))
        return t.value

    @staticmethod
    def alloc_outputs(torch, frames, pairs, K, device):
        """One set of output tensors, READY for a context's own stream: torch fills them with kernels on ITS stream, which the
        pipeline's streams do not wait for -- without the synchronize below a fill can land after the batch has written its
        results (seen: keypoint counts reading 0 with five batches in flight)."""
        out = Pipeline._alloc_outputs(torch, frames, pairs, K, device)
        torch.cuda.current_stream(device).synchronize()
        return out

    @staticmethod
    def _alloc_outputs(torch, frames, pairs, K, device):
        return dict(xy=torch.zeros((frames, K, 2), dtype=torch.float32, device=device),
                    desc=torch.zeros((frames, K, 32), dtype=torch.uint8, device=device),
                    nodes=torch.full((frames, K), -1, dtype=torch.int32, device=device),
                    n=torch.zeros((frames,), dtype=torch.int32, device=device),
                    matches=torch.zeros((pairs, K, 2), dtype=torch.int32, device=device),
                    best=torch.zeros((pairs, 4), dtype=torch.int32, device=device),
                    F=torch.zeros((pairs, 9), dtype=torch.float32, device=device))

    def poll(self, ticket):
        rc = self.lib.vslam_pipeline_poll(self.handle, C.c_int64(ticket))
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def wait(self, ticket):
        self._check(self.lib.vslam_pipeline_wait(self.handle, C.c_int64(ticket)))

    def wait_status(self, ticket):
        """(rc, message) instead of raising."""
        rc = self.lib.vslam_pipeline_wait(self.handle, C.c_int64(ticket))
        return rc, (self.lib.vslam_pipeline_last_error(self.handle).decode() if rc else "")

    def batches_redone(self):
        """Batches submit_pairs / submit_sequence queued that the pipeline queued a second time with whole-image corner lists."""
        self.lib.vslam_pipeline_batches_redone.restype = C.c_int64
        return int(self.lib.vslam_pipeline_batches_redone(self.handle))

    def drain(self):
        self._check(self.lib.vslam_pipeline_drain(self.handle))

    def workspace_bytes(self):
        return sum(c.workspace_bytes() for c in self.contexts)

    def close(self):
        if self.handle:
            for c in self.contexts:
                c.close()
            self.lib.vslam_pipeline_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id(lib=None):
    """128 bytes from vslam_comm_unique_id (rank 0 makes it, every rank passes the same bytes to Comm)."""
    lib = lib or load_library()
    uid = (C.c_ubyte * 128)()
    rc = lib.vslam_comm_unique_id(uid)
    if rc != OK:
        raise VslamError(f"{ERRORS.get(rc, rc)}: vslam_comm_unique_id (is librccl.so there?)")
    return bytes(uid)


class Comm:
    """ctypes stub of vslam_comm_* / vslam_gather_records*: the library's own RCCL communicator, made on a context's device."""

    def __init__(self, ctx, uid, world, rank):
        self.lib = ctx.lib
        self.world, self.rank = world, rank
        self.handle = C.c_void_p()
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        ctx._check(self.lib.vslam_comm_create(ctx.handle, buf, C.c_int(world), C.c_int(rank), C.byref(self.handle)))

    def info(self):
        w, r = C.c_int(-1), C.c_int(-1)
        rc = self.lib.vslam_comm_info(self.handle, C.byref(w), C.byref(r))
        if rc != OK:
            raise VslamError(f"{ERRORS.get(rc, rc)}: vslam_comm_info")
        return w.value, r.value

    def gather(self, ctx, rec, out):
        """Equal blocks: ncclAllGather of rec (this rank's records) into out (world x rec), on ctx's stream."""
        ctx._check(self.lib.vslam_gather_records(ctx.handle, self.handle, _ptr(rec), C.c_size_t(rec.numel()), _ptr(out)))

    def gather_v(self, ctx, rec, words, out, root=-1):
        arr = (C.c_size_t * len(words))(*words)
        ctx._check(self.lib.vslam_gather_records_v(ctx.handle, self.handle, _ptr(rec), arr, C.c_int(root), _ptr(out)))

    def close(self):
        if self.handle:
            self.lib.vslam_comm_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
