"""Run one Call (tests/entry_calls.py) on a stream that is stalled in front of it, with decoys where a kernel that ran too
early would read and where a kernel that ran too late would write.  tests/test_gpu_stream_order.py holds every entry point
to the stream-order contract of include/vslam_amd.h ("Stream order") with it.

What the caller of run_behind_stall sees of one run:

    stream:  [stall ..................][inputs <- real][ the entry point's work ][snapshots <- outputs][inputs <- decoys][outputs <- sentinel]
    host:     arm | call | host arguments <- decoys | tail | query, sleep T_wait, query | synchronise | compare

Until the stall ends every input holds its decoy, and the context's workspaces hold what a plain run on the decoys left in
them (made just before the stall is armed).  Work the library queues on another stream of its own (the auxiliary stream, the
copy stream) without ordering it behind the context's stream has an idle chip to run on for the whole stall and reads the
decoys; a stage that is not ordered behind the stage that fills its workspace reads what the decoys gave.  Either way the
bits differ from the plain run's: for work that starts too EARLY (a missing fork) the check is deterministic.  Work that is
waited for too LATE or not at all (a missing join of the auxiliary stream, a writer that lands after the snapshot, a reader
that outlives the call and meets the decoys again) shows only if it outlasts what the main stream does in the meantime: the
library's own streams cannot be held back from outside.  That side is opportunistic; it costs nothing and is kept.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from entry_calls import POSE_MEMBERS, _bytes, marshal, run, state_bytes
from offset_views import sentinel_fill

# Entry points that are documented to wait for the device before they return, with the line that blocks (found by reading
# vslam_amd/csrc for hipStreamSynchronize / hipEventSynchronize / hipMemcpy / hipFree).  For every OTHER entry point the stall
# must still be pending when the call returns: a host synchronisation that creeps into one of them fails the test.
BLOCKING = {
    "vslam_ctx_synchronize": "capi.hip vslam_ctx_synchronize: hipStreamSynchronize(ctx->stream), then hipMemcpy of the error word",
    "vslam_ctx_wait": "capi.hip vslam_ctx_wait: hipStreamSynchronize(ctx->stream)",
    "vslam_ctx_set_stream": "capi.hip vslam_ctx_set_stream: hipStreamSynchronize(ctx->stream) on the stream it leaves",
    "vslam_ctx_destroy": "capi.hip vslam_ctx_destroy: hipStreamSynchronize on the main, auxiliary and copy streams, hipFree",
    "vslam_corner_stats": "capi.hip vslam_corner_stats: hipStreamSynchronize(ctx->stream), then two hipMemcpy",
    "vslam_prof_enable": "capi.hip vs_prof_fold: hipStreamSynchronize(ctx->stream) when timed launches are pending",
    "vslam_prof_reset": "capi.hip vs_prof_fold",
    "vslam_prof_count": "capi.hip vs_prof_fold",
    "vslam_copy_h2d": "capi.hip vslam_copy_h2d: hipStreamSynchronize(ctx->stream) behind the copy",
    "vslam_copy_d2h": "capi.hip vslam_copy_d2h: hipStreamSynchronize(ctx->stream) behind the copy",
    "vslam_upload_wait": "capi.hip vslam_upload_wait: hipStreamSynchronize(ctx->copy_stream) -- the copy stream only",
    "vslam_dev_free": "capi.hip vslam_dev_free: hipFree",
    "vslam_host_free": "capi.hip vslam_host_free: hipHostFree",
    "vslam_map_destroy": "map.hip vslam_map_destroy: hipStreamSynchronize(map->ctx->stream), hipFree",
    "vslam_world_destroy": "world.hip vslam_world_destroy: hipStreamSynchronize(world->ctx->stream), hipFree",
    "vslam_pipeline_wait": "pipeline.hip: hipEventSynchronize(slot.done)",
    "vslam_pipeline_drain": "pipeline.hip: waits for every ticket in flight",
    "vslam_pipeline_acquire": "pipeline.hip retire: hipEventSynchronize on the slot's previous batch",
    "vslam_pipeline_submit_pairs": "pipeline.hip: acquires its slot, see vslam_pipeline_acquire",
    "vslam_pipeline_submit_pairs_pose": "pipeline.hip: acquires its slot",
    "vslam_pipeline_submit_sequence": "pipeline.hip: acquires its slot",
    "vslam_pipeline_destroy": "pipeline.hip: hipStreamSynchronize of every slot's stream",
    # and, on ANY entry point, the first call at a larger shape: vs_arena_get (capi.hip) waits for the stream before it frees a
    # workspace that has to grow.  The plain run in front of every stalled run has grown them already.
}

PROBE_CYCLES = 2_000_000
STALL_CAP_MS = 2000.0


class Sizing:
    """How long the stall lasts and how long the host waits behind the tail, chosen once:
    T_wait = max(10 ms, 10 x the longest device time of any call's plain run)
    stall  = T_wait + 20 x the longest host time of any plain call + 50 ms, at most 2 s."""

    def __init__(self, cycles_per_ms, longest_device_ms, longest_host_ms):
        self.cycles_per_ms = cycles_per_ms
        self.longest_device_ms, self.longest_host_ms = longest_device_ms, longest_host_ms
        self.t_wait_ms = max(10.0, 10.0 * longest_device_ms)
        self.stall_ms = min(self.t_wait_ms + 20.0 * longest_host_ms + 50.0, STALL_CAP_MS)
        self.stall_cycles = int(self.stall_ms * cycles_per_ms)

    def __str__(self):
        return (f"stall {self.stall_ms:.1f} ms ({self.stall_cycles} cycles at {self.cycles_per_ms:.0f} per ms), T_wait "
                f"{self.t_wait_ms:.1f} ms; longest plain call: {self.longest_device_ms:.3f} ms on the device, "
                f"{self.longest_host_ms:.3f} ms on the host")


def sleep_cycles_per_ms(stream):
    """torch.cuda._sleep counts cycles of the device's clock: one probe between two events gives their length."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1000)            # the kernel's first launch is not the one that is timed
        e0.record(stream)
        torch.cuda._sleep(PROBE_CYCLES)
        e1.record(stream)
    e1.synchronize()
    return PROBE_CYCLES / e0.elapsed_time(e1)


def time_plain(ctx, call, stream):
    """-> (host ms inside the entry point, device ms between two events around it) of one plain run (arenas warm)."""
    with torch.cuda.stream(stream):
        t = dict(call.ins)
        for name, src in call.inouts.items():
            t[name] = src.clone()
        for name, (shape, dtype) in call.outs.items():
            t[name] = sentinel_fill(torch.empty(shape, dtype=dtype, device="cuda"))
        if call.before:
            call.before()
        argv, _live = marshal(call, t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn = getattr(ctx.lib, call.entry)
        torch.cuda.synchronize()
        e0.record(stream)
        t0 = time.perf_counter()
        rc = fn(ctx.handle, *argv)
        t1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        assert rc == 0, (call.entry, rc)
        assert ctx.lib.vslam_ctx_synchronize(ctx.handle) == 0
    return (t1 - t0) * 1e3, e0.elapsed_time(e1)


def choose_sizing(ctx, calls, stream):
    cycles = sleep_cycles_per_ms(stream)
    host = dev = 0.0
    for call in calls:
        with torch.cuda.stream(stream):
            rc, msg, _, _ = run(ctx, call)      # grows the arenas: never part of a timed call
        assert rc == 0, (call.entry, msg)
        h, d = time_plain(ctx, call, stream)
        host, dev = max(host, h), max(dev, d)
    return Sizing(cycles, dev, host)


class Stalled:
    """What run_behind_stall saw: rc / msg of the call, `expected` and `got` {name: bytes}, and whether the stall was still
    pending when the call returned, when the tail was queued, and T_wait after that."""


def _host_copy(h):
    return h.copy() if isinstance(h, np.ndarray) else type(h).from_buffer_copy(h)


def run_behind_stall(ctx, call, stream, decoys, sizing, expected=None):
    """`call` on `ctx`, which is bound to `stream`, behind a stall on that stream (module docstring).  expected: the outputs of
    the plain run under the same options; taken from run() on the same context when not given (which also grows the context's
    workspaces, so that the run under test allocates and frees nothing)."""
    res = Stalled()
    with torch.cuda.stream(stream):
        if expected is None:
            rc, msg, expected, _ = run(ctx, call)
            assert rc == 0, (call.entry, msg)
        res.expected = expected
        # The context's workspaces (gray and blurred planes, the rotated table, the raw generator outputs, detected corners,
        # pairs, sets ...) must not already hold what the run under test will compute, or a reader that is not ordered behind
        # their writer meets the right bits anyway: one plain run with every decoy in place leaves them holding what the decoys
        # give -- and as large as they were.
        rc, msg, _, _ = run(ctx, decoys.call_with(call, hosts=list(decoys.hosts), params=decoys.params is not None))
        assert rc == 0, (call.entry, "with every decoy in place", msg)
        # prepare: resident state as the plain run found it, private inputs that hold the decoys, outputs that hold the sentinel
        if call.before:
            call.before()
        real = dict(call.ins, **call.inouts)
        buf = {name: decoys.tensors[name].clone() for name in real}
        out = {name: sentinel_fill(torch.empty(shape, dtype=dtype, device="cuda")) for name, (shape, dtype) in call.outs.items()}
        t = dict(buf, **out)
        written = list(call.outs) + list(call.inouts)
        snap = {name: sentinel_fill(torch.empty_like(t[name])) for name in written}
        dump = {name: sentinel_fill(torch.empty_like(out[name])) for name in out if name.startswith("pose->")}
        hosts = {name: _host_copy(h) for name, h in call.hosts.items()}
        argv, live = marshal(call, t, hosts)
        fn = getattr(ctx.lib, call.entry)
        stall_end = torch.cuda.Event()
        torch.cuda.synchronize()
        # arm: from here to the comparison the host waits for nothing
        torch.cuda._sleep(sizing.stall_cycles)
        stall_end.record(stream)
        for name in real:
            buf[name].copy_(real[name], non_blocking=True)
        res.rc = fn(ctx.handle, *argv)
        res.pending_at_return = not stall_end.query()
        res.msg = (ctx.lib.vslam_last_error(ctx.handle) or b"").decode() if res.rc else ""
        # host arguments are consumed before the call returns: whatever is read from now on is a decoy
        for name, h in hosts.items():
            d = decoys.hosts[name]
            if isinstance(h, np.ndarray):
                h[...] = d
            else:
                C.memmove(C.addressof(h), C.addressof(d), C.sizeof(h))
        if "params" in live:
            p = live["params"]
            p.max_corners, p.quality, p.min_distance, p.cos_a, p.sin_a = decoys.params
            p.d_pattern = decoys.tensors["params->d_pattern"].data_ptr()
        if "pose" in live:
            for k in POSE_MEMBERS:
                setattr(live["pose"], "d_" + k, dump["pose->d_" + k].data_ptr())
        # the tail: what the caller's next work on the stream does with the arrays
        for name in written:
            snap[name].copy_(t[name], non_blocking=True)
        for name in real:
            buf[name].copy_(decoys.tensors[name], non_blocking=True)
        for name in out:
            sentinel_fill(out[name])
        res.pending_after_tail = not stall_end.query()
        time.sleep(sizing.t_wait_ms / 1e3)
        res.pending_after_wait = not stall_end.query()
        torch.cuda.synchronize()
        status = ctx.lib.vslam_ctx_synchronize(ctx.handle)
        if status == -2:     # VSLAM_ERR_HIP: nothing more is started on a device that has just faulted
            pytest.exit(f"HIP error behind {call.entry} behind a stall: {(ctx.lib.vslam_last_error(ctx.handle) or b'').decode()}",
                        returncode=3)
        assert status == 0, (call.entry, status)
        res.got = {name: _bytes(snap[name]) for name in written if name not in call.scratch}
        res.got.update(state_bytes(call))
        res.dump_untouched = all(bool((d.view(torch.uint8) == 0xA5).all()) for d in dump.values())
    return res
