"""The Calls (tests/entry_calls.Call) of the entry points include/vslam_places.h declares that queue work on the context's stream, as
tests/tracks_calls.py has them for vslam_tracks.h: the argument list of the C prototype with every device tensor named as the header
names it."""
import ctypes as C

import numpy as np
import torch

from entry_calls import Call, P
from vslam_amd import capi

i32, u8 = torch.int32, torch.uint8

ENTRIES = ["vslam_places_assign", "vslam_places_train", "vslam_places_set_vocabulary", "vslam_places_set_weights", "vslam_places_add",
           "vslam_places_query", "vslam_places_reset", "vslam_places_view"]


def assign(desc, n, vocab, want_dist=True):
    Fr, Kp, W = desc.shape[0], desc.shape[1], vocab.shape[0]
    argv = [P("d_desc"), P("d_n"), Kp, Fr, P("d_vocab"), W, P("d_word"), P("d_dist")]
    outs = {"d_word": ((Fr, Kp), i32)}
    if want_dist:
        outs["d_dist"] = ((Fr, Kp), i32)
    return Call("vslam_places_assign", argv, ins={"d_desc": desc, "d_n": n, "d_vocab": vocab}, outs=outs, absent=() if want_dist else ("d_dist",))


def train(desc, n_words, iterations):
    argv = [P("d_desc"), desc.shape[0], n_words, iterations, P("d_vocab"), P("d_sizes")]
    return Call("vslam_places_train", argv, ins={"d_desc": desc}, outs={"d_vocab": ((n_words, 32), u8), "d_sizes": ((n_words,), i32)})


def _state(idx):
    def state():
        return {k: v for k, v in idx.view().items() if k != "size"}
    return state


def set_vocabulary(idx, vocab, weights=None):
    """on an index that `before` empties"""
    ins = {"d_vocab": vocab}
    if weights is not None:
        ins["d_weights"] = weights
    return Call("vslam_places_set_vocabulary", [idx.handle, P("d_vocab"), P("d_weights")], ins=ins, absent=() if weights is not None else ("d_weights",),
                before=idx.reset, state=_state(idx))


def set_weights(idx, weights):
    return Call("vslam_places_set_weights", [idx.handle, P("d_weights")], ins={"d_weights": weights}, state=_state(idx))


def add(idx, desc, n, tags=None, before=None):
    """before: what puts the index into the state the call starts from (idx.reset for an add into an empty index)"""
    Fr, Kp = desc.shape[0], desc.shape[1]
    ins = {"d_desc": desc, "d_n": n}
    if tags is not None:
        ins["d_tags"] = tags
    return Call("vslam_places_add", [idx.handle, P("d_desc"), P("d_n"), Kp, Fr, P("d_tags"), P("d_ids")], ins=ins, outs={"d_ids": ((Fr,), i32)},
                absent=() if tags is not None else ("d_tags",), before=before or idx.reset, state=_state(idx))


def query(idx, desc, n, top_k, below=None):
    Q, Kp = desc.shape[0], desc.shape[1]
    ins = {"d_desc": desc, "d_n": n}
    if below is not None:
        ins["d_below"] = below
    outs = {"d_best_id": ((Q, top_k), i32), "d_best_score": ((Q, top_k), i32), "d_best_den": ((Q, top_k), i32), "d_q_norm": ((Q,), i32)}
    return Call("vslam_places_query", [idx.handle, P("d_desc"), P("d_n"), Kp, Q, P("d_below"), top_k, P("d_best_id"), P("d_best_score"),
                                       P("d_best_den"), P("d_q_norm")], ins=ins, outs=outs, absent=() if below is not None else ("d_below",),
                state=_state(idx))


def reset(idx, before):
    """before: what fills the index in front of the call"""
    return Call("vslam_places_reset", [idx.handle], before=before, state=_state(idx))


def view(idx, before):
    """before: what leaves the index with norms the call has to form anew.  The state is what the call's OWN struct points at, read
    without another call of the entry point: the sizes and the norms its launch wrote."""
    arr = capi.PlacesArrays()
    ctx = idx.ctx

    def state():
        ctx._check(ctx.lib.vslam_ctx_wait(ctx.handle))
        norms = np.empty(int(arr.size), np.int32)
        if norms.nbytes:
            ctx._check(ctx.lib.vslam_copy_d2h(ctx.handle, norms.ctypes.data_as(C.c_void_p), C.c_void_p(arr.d_norms), C.c_size_t(norms.nbytes)))
        return {"norms": norms, "sizes": np.array([arr.n_words, arr.capacity, arr.max_kp, arr.size], np.int32)}
    return Call("vslam_places_view", [idx.handle, C.byref(arr)], before=before, state=state)
