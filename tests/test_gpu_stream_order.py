"""The stream-order contract of include/vslam_amd.h ("Stream order"), entry point by entry point.

Every entry point queues its work on the context's stream, but inside the library part of that work runs on other streams:
the 7 x 7 blur, the rBRIEF table rotation, the deferred k-d build (VSLAM_OPT_TREE_FORK) and the mt19937 prefetch on an
auxiliary stream, uploads on a copy stream -- tied to the context's stream by hand-placed events.  A missing or misplaced wait
is invisible to a test whose inputs are complete before the call and whose outputs are read after a wait, which is every other
test of this suite.  Here each Call of tests/entry_calls.py runs behind a STALLED stream (tests/stream_order.py): the inputs
hold decoys until the stall ends and the context's workspaces hold what a run on the decoys left in them (so that a stage
which is not ordered behind the stage that fills its workspace -- the blur behind the gray plane, the describe stage behind the
blur and the rotated table, the set mapping behind the raw generator outputs -- does not find the right bits there from an
earlier run), the real values are copied in behind the stall on the same stream, host arguments are
overwritten with decoys the moment the call returns, and the next work on the stream snapshots the outputs and puts the decoys
back.  The snapshots and the resident state must equal the plain, fully synchronised run bit for bit, and -- for every entry
point that is not declared to wait for the device (stream_order.BLOCKING) -- the stall must still be pending when the call
returns: a host synchronisation that creeps into the hot path fails here.

  * sensitivity: with the decoys left in place the result differs (per call), and so it does with any single argument
    exchanged (per argument), except for the counts and structural arrays of entry_calls.EXEMPT, which keep their real
    values so that any mixture of real and decoy arguments stays a valid call -- the list is held to exactly that set;
  * every Call behind a stall on a side stream, and on the legacy default stream (what capi.Context() binds to: the auxiliary
    and copy streams are non-blocking, the default stream's implicit synchronisation does not cover them);
  * the front end's branches: every fork point of the k-d build, with and without VSLAM_OPT_RANSAC_ALL_SUMS (fork point 4 is
    never passed with it), d_nodes NULL, per-kernel timing on, VSLAM_OPT_POSE_REFIT / _REFINE each and both;
  * vslam_map_step with a world attached; upload -> fence -> front end -> download on page-locked buffers; a context that is
    rebound from its private stream to a borrowed one and on to another.

What is deterministic and what is not.  A FORK is held deterministically: work on the auxiliary stream that is not ordered
behind the context's stream, or behind the stage whose workspace it reads, runs during the stall and reads decoys or what the
decoys left, whatever its timing.  A JOIN (the main stream waiting for the auxiliary one: behind the blur and the table
rotation, the ev_raw wait in front of the set mapping, the k-d build's join at the end of the call) and the output side (a
writer that lands after the snapshot, a reader of an input the caller has recycled) are opportunistic: the auxiliary stream
is the library's own and cannot be held back from outside, so a missing join shows only if the auxiliary work outlasts the
main stream's way to its reader.  Measured with three variants of the library, one wait removed in each: without the fork
in front of the blur (select.hip) 10 of the 12 front-end cases of the two per-stream tests fail; without the join behind the
blur, or without the ev_raw wait, all 12 pass -- the blur and the generator are done long before corner selection is.  The stall is bounded work of one wave (torch.cuda._sleep) that leaves the chip
free, sized once per module (stream_order.Sizing) and never retried; no bar is derived from it.

Not covered: the wait of vslam_upload_fence itself (the copy stream cannot be stalled from outside: the upload case holds the
path's results and its asynchrony only); the pipeline's private streams (their inputs are ordered by the caller's contract -- resident, or uploaded through
the acquired context -- and a caller cannot queue foreign work on them), and vslam_multi_* / vslam_comm_*, which need more
than one device.

Measured on an MI355X (first device run): the longest plain call takes 0.35 ms on the device and 0.23 ms on the host, so
T_wait = 10.0 ms and the stall = 64.5 ms (153.6 M cycles of torch.cuda._sleep at 2.38 M per ms); the 222 tests of this file
take 12 s, fixtures included.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from entry_calls import (ENTRIES, EXEMPT, KP, PAIRS, SEED, STRUCTURAL, _same, build_decoys, build_scene, canonical, close_scene,
                         close_stream_order_calls, decoy_scene, map_state, marshal, run, stream_order_calls)
from offset_views import sentinel_fill
from stream_order import BLOCKING, choose_sizing, run_behind_stall
from vslam_amd import capi

pytestmark = pytest.mark.gpu

FRONT = ["vslam_frontend_pairs", "vslam_frontend_pairs_pose", "vslam_frontend_sequence", "vslam_track_sequences"]
TAKES_NO_TREES = FRONT[:3]                   # d_nodes may be NULL
POSE = ["vslam_frontend_pairs_pose", "vslam_track_sequences"]
READS_RESIDENT_STATE_ONLY = {"vslam_map_observations"}     # no input a decoy could stand in for
OPT = capi.Context
DEFAULTS = {OPT.OPT_TREE_FORK: -1, OPT.OPT_RANSAC_ALL_SUMS: 0, OPT.OPT_POSE_REFIT: 0, OPT.OPT_POSE_REFINE: 0}


class Bound:
    """A context bound to `stream` with the scene, calls and decoys made on it."""

    def __init__(self, ctx, stream, other=None):
        self.ctx, self.stream = ctx, stream
        with torch.cuda.stream(stream):
            self.scene = build_scene(ctx, SEED)
            self.calls = stream_order_calls(ctx, self.scene)
            self.own_other = other is None
            self.other = decoy_scene(ctx) if other is None else other
            self.other_calls = stream_order_calls(ctx, self.other, resident=False)
            self.decoys = build_decoys(self.calls, self.other_calls, self.other)
            torch.cuda.synchronize()

    def plain(self, call):
        with torch.cuda.stream(self.stream):
            rc, msg, got, _ = run(self.ctx, call)
        assert rc == 0, (call.entry, msg)
        return canonical(call.entry, got)

    def stalled(self, call, decoys, sizing, expected=None):
        return run_behind_stall(self.ctx, call, self.stream, decoys, sizing, expected)

    def close(self):
        close_stream_order_calls(self.scene)
        close_scene(self.scene)
        if self.own_other:
            close_scene(self.other)
        self.ctx.close()


@pytest.fixture(scope="module")
def side():
    t0 = time.time()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = capi.Context(0)
    b = Bound(ctx, stream)
    yield b
    b.close()
    print(f"tests/test_gpu_stream_order.py: {time.time() - t0:.1f} s from the first fixture to the last test")


@pytest.fixture(scope="module")
def dflt(side):
    stream = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == stream
    b = Bound(capi.Context(0), stream, other=side.other)
    yield b
    b.close()


@pytest.fixture(scope="module")
def sizing(side):
    s = choose_sizing(side.ctx, list(side.calls.values()), side.stream)
    print("stream order:", s)
    return s


def _raw(h):
    return h.tobytes() if isinstance(h, np.ndarray) else bytes(h)


def hold(res, entry):
    assert res.rc == 0, (entry, res.msg)
    if entry not in BLOCKING:
        assert res.pending_at_return, f"{entry} waited for the device before it returned"
        assert res.pending_after_tail and res.pending_after_wait, f"{entry}: the stall ended before T_wait had passed"
    assert res.dump_untouched, f"{entry} read vslam_pose_outputs after it returned"
    diff = _same(canonical(entry, res.expected), canonical(entry, res.got))
    assert not diff, f"{entry} behind a stalled stream differs from its plain run in {diff}"


# ------------------------------------------------------------------------------------------------------------- the scenario
def test_every_entry_point_of_build_calls_is_parametrised(side):
    assert set(side.calls) == set(ENTRIES), sorted(set(side.calls) ^ set(ENTRIES))
    assert not set(side.calls) & set(BLOCKING), "an entry point that waits for the device has no place in the asynchrony check"


def test_the_exception_list_is_exactly_the_counts_and_structural_arrays(side):
    kept_real = {(entry, name) for entry, d in side.decoys.items() for name in d.same}
    listed = {(entry, name) for entry, names in EXEMPT.items() for name in names}
    assert kept_real == listed, sorted(kept_real ^ listed)
    assert {name for _, name in listed} == set(STRUCTURAL), "every exempt name is a count or a structural array, with its reason"
    for entry, d in side.decoys.items():
        call = side.calls[entry]
        for name, real in list(call.ins.items()) + list(call.inouts.items()):
            assert torch.equal(d.tensors[name], real) == (name in EXEMPT.get(entry, ())), (entry, name)
        for name, real in call.hosts.items():
            assert _raw(d.hosts[name]) != _raw(real), (entry, name)


@pytest.mark.parametrize("entry", ENTRIES)
def test_decoys_left_in_place_change_the_result(side, entry):
    call, d = side.calls[entry], side.decoys[entry]
    if not (set(d.tensors) - d.same or d.hosts or d.params):
        assert entry in READS_RESIDENT_STATE_ONLY, entry
        return
    assert entry not in READS_RESIDENT_STATE_ONLY
    expected = side.plain(call)
    got = side.plain(d.call_with(call, hosts=list(d.hosts), params=d.params is not None))
    assert _same(expected, got), f"{entry}: every input exchanged for its decoy and no compared output differs"


@pytest.mark.parametrize("entry", ENTRIES)
def test_each_argument_alone_changes_the_result(side, entry):
    call, d = side.calls[entry], side.decoys[entry]
    expected = side.plain(call)
    blind = []
    for name in d.tensors:
        if name not in EXEMPT.get(entry, ()) and not _same(expected, side.plain(d.call_with(call, names=[name]))):
            blind.append(name)
    for name in d.hosts:
        if not _same(expected, side.plain(d.call_with(call, names=[], hosts=[name]))):
            blind.append(name)
    if d.params is not None and not _same(expected, side.plain(d.call_with(call, names=[], params=True))):
        blind.append("params")
    assert not blind, f"{entry}: no compared output depends on {blind}"
    assert not _same(expected, side.plain(call)), "the plain run repeats"


# ---------------------------------------------------------------------------------------------------- every call, two streams
@pytest.mark.parametrize("entry", ENTRIES)
def test_order_behind_a_side_stream(side, sizing, entry):
    hold(side.stalled(side.calls[entry], side.decoys[entry], sizing), entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_order_behind_the_legacy_default_stream(dflt, sizing, entry):
    assert dflt.stream.cuda_stream == 0
    hold(dflt.stalled(dflt.calls[entry], dflt.decoys[entry], sizing), entry)


# ------------------------------------------------------------------------------------------------ the front end's branches
@pytest.mark.parametrize("all_sums", [0, 1])
@pytest.mark.parametrize("fork", [-1, 0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("entry", FRONT)
def test_front_end_fork_points(side, sizing, entry, fork, all_sums):
    try:
        side.ctx.set_option(OPT.OPT_TREE_FORK, fork)
        side.ctx.set_option(OPT.OPT_RANSAC_ALL_SUMS, all_sums)
        res = side.stalled(side.calls[entry], side.decoys[entry], sizing)
    finally:
        for k, v in DEFAULTS.items():
            side.ctx.set_option(k, v)
    hold(res, entry)
    assert res.got["d_nodes"].view(np.int32).max() >= 0, "trees were built"


@pytest.mark.parametrize("entry", TAKES_NO_TREES)
def test_front_end_without_trees(side, sizing, entry):
    base = side.calls[entry]
    call = base.replaced(outs={k: v for k, v in base.outs.items() if k != "d_nodes"}, absent=base.absent | {"d_nodes"})
    res = side.stalled(call, side.decoys[entry], sizing)
    hold(res, entry)
    full = side.plain(base)
    assert not _same(res.got, {k: full[k] for k in res.got}), "without trees every other output is what it is with them"


@pytest.mark.parametrize("entry", FRONT)
def test_front_end_with_per_kernel_timing_on(side, sizing, entry):
    expected = side.plain(side.calls[entry])
    side.ctx.prof_enable(True)
    try:
        res = side.stalled(side.calls[entry], side.decoys[entry], sizing)
    finally:
        side.ctx.prof_enable(False)
        side.ctx.prof_reset()
    hold(res, entry)
    assert not _same(expected, res.got), "timing changes no result"


@pytest.mark.parametrize("refit,refine", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("entry", POSE)
def test_pose_options(side, sizing, entry, refit, refine):
    plain = side.plain(side.calls[entry])
    try:
        side.ctx.set_option(OPT.OPT_POSE_REFIT, refit)
        side.ctx.set_option(OPT.OPT_POSE_REFINE, refine)
        res = side.stalled(side.calls[entry], side.decoys[entry], sizing)
    finally:
        for k, v in DEFAULTS.items():
            side.ctx.set_option(k, v)
    hold(res, entry)
    if refit or entry == "vslam_frontend_pairs_pose":     # (on this fixture the adjustment leaves the tracks' poses as they are)
        assert _same(plain, res.expected), "the options change the result"


def test_map_step_with_a_world_attached(side, sizing):
    base = side.calls["vslam_map_step"]
    with torch.cuda.stream(side.stream):
        pmap = capi.PointMap(side.ctx, PAIRS, 3, KP, KP, 4 * KP)
        world = pmap.attach_world(min_links=1)
    try:
        call = base.replaced(argv=[pmap.handle] + base.argv[1:], before=pmap.reset, state=map_state(pmap))
        res = side.stalled(call, side.decoys["vslam_map_step"], sizing)
        hold(res, "vslam_map_step")
        lifted = res.got["state:world_points"].view(np.float32)
        assert "state:world_Twc" in res.got and lifted.any(), "the world was stepped and points were lifted"
    finally:
        pmap.close()
        world.close()


# --------------------------------------------------------------------------------------------------------------- upload path
def _pinned(ctx, nbytes):
    p = C.c_void_p()
    ctx._check(ctx.lib.vslam_host_alloc(ctx.handle, C.c_size_t(nbytes), C.byref(p)))
    return p, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))


def test_upload_fence_front_end_download(side, sizing):
    """vslam_upload_async -> vslam_upload_fence -> vslam_frontend_pairs -> vslam_download_async as the header describes them,
    on page-locked buffers: the frames arrive over the copy stream, everything else behind the stall.  What is held: the
    path's results (the download is ordered behind the front end, the front end behind the stream) and its asynchrony.  NOT
    held: the fence itself.  The copy stream is not stalled, so the upload has landed long before the front end starts, with or
    without ev_upload."""
    ctx, lib, stream = side.ctx, side.ctx.lib, side.stream
    call, d = side.calls["vslam_frontend_pairs"], side.decoys["vslam_frontend_pairs"]
    frames, decoy_frames = call.ins["d_bgr"], d.tensors["d_bgr"]
    nbytes = frames.numel()
    sizes = {name: int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size() for name, (shape, dtype) in call.outs.items()}
    h_in_p, h_in = _pinned(ctx, nbytes)
    h_out = {name: _pinned(ctx, n) for name, n in sizes.items()}
    fn = lib.vslam_frontend_pairs

    def queue(c, t):
        argv, live = marshal(c, t)
        ctx._check(lib.vslam_upload_async(ctx.handle, C.c_void_p(t["d_bgr"].data_ptr()), h_in_p, C.c_size_t(nbytes)))
        ctx._check(lib.vslam_upload_fence(ctx.handle))
        ctx._check(fn(ctx.handle, *argv))
        for name, n in sizes.items():
            ctx._check(lib.vslam_download_async(ctx.handle, h_out[name][0], C.c_void_p(t[name].data_ptr()), C.c_size_t(n)))
        return live

    try:
        with torch.cuda.stream(stream):
            rest = [k for k in call.ins if k != "d_bgr"]
            buf = {k: d.tensors[k].clone() for k in call.ins}
            out = {k: sentinel_fill(torch.empty(shape, dtype=dtype, device="cuda")) for k, (shape, dtype) in call.outs.items()}
            t = dict(buf, **out)
            # the plain run: real inputs in place, the host waits before it looks
            for k in rest:
                buf[k].copy_(call.ins[k])
            h_in[:] = frames.cpu().numpy().reshape(-1)
            decoy_bytes = decoy_frames.cpu().numpy().reshape(-1)
            torch.cuda.synchronize()
            queue(call, t)
            ctx.synchronize()
            expected = {k: v[1].copy() for k, v in h_out.items()}
            device_path = {k: v.reshape(-1) for k, v in side.plain(call).items() if k in expected}
            assert not _same(expected, device_path), "the upload path gives what the device path gives"
            # the same path on the decoys: the workspaces then hold what the decoys give (stream_order.run_behind_stall)
            for k in call.ins:
                buf[k].copy_(d.tensors[k])
            h_in[:] = decoy_bytes
            torch.cuda.synchronize()
            queue(d.call_with(call, names=[], hosts=list(d.hosts), params=True), t)
            ctx.synchronize()
            # behind the stall
            h_in[:] = frames.cpu().numpy().reshape(-1)
            for k, v in h_out.items():
                v[1][:] = 0xA5
            for k in out:
                sentinel_fill(out[k])
            stall_end = torch.cuda.Event()
            torch.cuda.synchronize()
            torch.cuda._sleep(sizing.stall_cycles)
            stall_end.record(stream)
            for k in rest:
                buf[k].copy_(call.ins[k], non_blocking=True)
            live = queue(call, t)
            assert not stall_end.query(), "the upload path waited for the device"
            ctx._check(lib.vslam_upload_wait(ctx.handle))        # the copy stream only: the host buffer may be refilled
            assert not stall_end.query(), "vslam_upload_wait waited for the compute stream"
            h_in[:] = decoy_bytes
            p = live["params"]
            p.max_corners, p.quality, p.min_distance, p.cos_a, p.sin_a = d.params
            for k in call.ins:
                buf[k].copy_(d.tensors[k], non_blocking=True)
            for k in out:
                sentinel_fill(out[k])
            held = not stall_end.query()
            time.sleep(sizing.t_wait_ms / 1e3)
            held = held and not stall_end.query()
            torch.cuda.synchronize()
            ctx.synchronize()
            assert held, "the stall ended before T_wait had passed"
            got = {k: v[1].copy() for k, v in h_out.items()}
        assert not _same(expected, got), f"downloaded bytes differ from the plain run's in {_same(expected, got)}"
    finally:
        for p, _ in [(h_in_p, None)] + list(h_out.values()):
            lib.vslam_host_free(ctx.handle, p)


# ----------------------------------------------------------------------------------------------------------------- rebinding
def test_rebinding_from_the_private_stream_to_borrowed_ones(side, sizing):
    entry = "vslam_frontend_pairs_pose"
    call, d = side.calls[entry], side.decoys[entry]
    reference = side.plain(call)
    ctx = capi.Context(0, use_torch_stream=False)      # runs on its own private non-blocking stream
    try:
        rc, msg, private, _ = run(ctx, call)
        assert rc == 0, msg
        assert not _same(reference, private)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ctx._check(ctx.lib.vslam_ctx_set_stream(ctx.handle, C.c_void_p(s1.cuda_stream)))
        with torch.cuda.stream(s1):
            rc, msg, first, _ = run(ctx, call)
        assert rc == 0, msg
        assert not _same(reference, first)
        ctx._check(ctx.lib.vslam_ctx_set_stream(ctx.handle, C.c_void_p(s2.cuda_stream)))
        res = run_behind_stall(ctx, call, s2, d, sizing, expected=reference)
        hold(res, entry)
    finally:
        ctx.close()
