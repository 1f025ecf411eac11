"""Device arrays that do NOT start where their allocation starts: what a caller with an arena, a ring buffer or a slice of a
larger batch hands the C ABI.  Every other GPU test takes its arrays straight from torch's allocator (256-byte aligned)."""
import torch

GUARD_ELEMS = 64          # sentinel elements in front of the offset and behind the view
SENTINEL_BYTE = 0xA5


def sentinel_fill(t):
    """Every byte of `t` = SENTINEL_BYTE, whatever its dtype."""
    t.view(torch.uint8).fill_(SENTINEL_BYTE)
    return t


def offset_view(shape, dtype, offset_elems, device="cuda"):
    """(view, whole, check): a contiguous `view` of `shape` that starts GUARD_ELEMS + offset_elems elements into the 1-D
    allocation `whole`, all of it (the view included) filled with SENTINEL_BYTE; check() asserts that the bytes of `whole` on
    both sides of the view still hold the sentinel.  The allocation's own base is 256-byte aligned and GUARD_ELEMS elements are
    a multiple of 64 bytes, so the view's address is offset_elems elements off a 64-byte boundary -- and nothing more aligned
    than that offset allows."""
    n = 1
    for s in shape:
        n *= int(s)
    lo = GUARD_ELEMS + int(offset_elems)
    whole = sentinel_fill(torch.empty((lo + n + GUARD_ELEMS,), dtype=dtype, device=device))
    assert whole.data_ptr() % 256 == 0
    view = whole[lo:lo + n].view(*shape)
    assert view.is_contiguous() and view.data_ptr() == whole.data_ptr() + lo * whole.element_size()

    def check(what=""):
        raw = whole.view(torch.uint8)
        e = whole.element_size()
        front, back = raw[:lo * e], raw[(lo + n) * e:]
        assert bool((front == SENTINEL_BYTE).all()) and bool((back == SENTINEL_BYTE).all()), f"guard band overwritten {what}"

    return view, whole, check
