"""Poisoned query outputs: every tensor the library writes into is born full of a value no query can produce.

The GPU suite compares launches with the oracle bit for bit, and the buffers it reads come from torch.empty:
the caching allocator hands the blocks of launch k to launch k + 2 of the same shape, which then already hold
the right answer for the same rays.  A launch that never reaches a block -- an order that is not a permutation,
a counter that is not reset, a tile map that skips the ragged edge, a miss whose zeros are forgotten -- leaves
those bytes alone and passes.  With this module installed the bytes it leaves alone are poison:

    dtype          poison                               why it is no valid output
    bool / uint8   every byte 0xA5                      valid bytes are 0 or 1
    int32          0xA5A5A5A5 = -1515870811             triangle, slot, count, ray index are >= -1
    int64          0xA5A5A5A5A5A5A5A5                   offsets and totals are >= 0
    float32        the bits 0x7FA5A5A5 (a NaN)          no computed output carries this payload

install() swaps the allocation seam of triro.backend.ops and triro.ray.sharded (`_new_output`) for one that
fills, on the current stream -- the stream ops.py launches on, so ordering is free, and inside a graph capture
the fill is captured: every replay re-poisons.  It also wraps the ops-level entry points RayMeshIntersector
calls: after each eager call assert_written() runs on what came back.  (Tensors handed in as `outs=` are caught
when the caller poisoned them: fill().)  While the stream is capturing the check is skipped -- it synchronises --
and the graph tests call assert_written() themselves after replay().

What this net catches is elements NOT WRITTEN.  Elements written with wrong data are the oracle comparison's.

A module turns it on with   from poison import poisoned_outputs  # noqa: F401   (an autouse fixture).
"""
import functools

import pytest
import torch

BYTE = 0xA5
INT32 = 0xA5A5A5A5 - (1 << 32)                      # -1515870811
INT64 = 0xA5A5A5A5A5A5A5A5 - (1 << 64)
FLOAT32_BITS = 0x7FA5A5A5                           # a NaN: compared as bits, never with isnan
_CHUNK = 1 << 26                                    # elements checked at a time: the masks of a 2^31-ray output stay small

# the ops-level functions RayMeshIntersector calls: everything they return is a library-written tensor (or None)
ENTRY_POINTS = ("intersects_any", "intersects_first", "intersects_closest", "intersects_count", "intersects_location",
                "intersects_closest_packed", "intersects_closest_slots", "closest_from_slots", "closest_expand",
                "closest_expand_slots", "compact_closest")

_installed = None       # (module, name, original) of everything install() replaced


def _bits(t: torch.Tensor):
    """(integer view of t, its poison, what a stale element satisfies)"""
    if t.dtype == torch.bool:
        return t.view(torch.uint8), BYTE, "gt1"
    if t.dtype == torch.uint8:
        return t, BYTE, "eq"
    if t.dtype == torch.int32:
        return t, INT32, "eq"
    if t.dtype == torch.int64:
        return t, INT64, "eq"
    if t.dtype == torch.float32:
        return t.view(torch.int32), FLOAT32_BITS, "eq"
    # no output of the library has another type; a gather buffer of triro.ray.sharded takes the type of what it gathers
    return t.contiguous().view(torch.uint8).reshape(*t.shape, t.element_size()), BYTE, "bytes"


def _mask(view, value, how):
    if how == "gt1":
        return view > 1
    if how == "bytes":
        return (view == value).all(-1)
    return view == value


def fill(t: torch.Tensor) -> torch.Tensor:
    """poison t in place (on the current stream of its device); returns t"""
    view, value, how = _bits(t)
    if how == "bytes" and not t.is_contiguous():
        raise TypeError(f"poison.fill: a {t.dtype} tensor must be contiguous")
    view.fill_(value)
    return t


def poisoned(shape, dtype, device) -> torch.Tensor:
    """the allocator install() puts into the seam"""
    return fill(torch.empty(shape, dtype=dtype, device=device))


def stale_mask(t: torch.Tensor) -> torch.Tensor:
    """bool tensor of t's shape: which elements still hold their poison (bitwise; a bool byte above 1)"""
    return _mask(*_bits(t))


def _stale(t: torch.Tensor):
    """(number of stale elements, flat index of the first one or None)"""
    view, value, how = _bits(t)
    flat = view.reshape(-1, view.shape[-1]) if how == "bytes" else view.reshape(-1)
    count, first = 0, None
    for lo in range(0, flat.shape[0], _CHUNK):
        mask = _mask(flat[lo:lo + _CHUNK], value, how)
        c = int(mask.sum())
        if c and first is None:
            first = lo + int(mask.to(torch.uint8).argmax())
        count += c
    return count, first


def assert_written(*tensors, what="output"):
    """raises if any element of any tensor still holds its poison; None entries (outputs not asked for) are skipped"""
    for k, t in enumerate(tensors):
        if t is None:
            continue
        count, first = _stale(t)
        if count:
            name = what if len(tensors) == 1 else f"{what}[{k}]"
            raise AssertionError(f"{name} ({t.dtype}, shape {tuple(t.shape)}): {count} of {t.numel()} elements were never "
                                 f"written (they still hold the poison), the first at flat index {first}")


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _checked(fn, name):
    @functools.wraps(fn)
    def call(*args, **kwargs):
        res = fn(*args, **kwargs)
        if not _capturing():
            outs = res if isinstance(res, (tuple, list)) else (res,)
            assert_written(*outs, what=f"ops.{name}")
        return res
    call.__wrapped_by_poison__ = True
    return call


def install():
    """poisoning allocators into both seams, written-checks around the ops entry points.  Idempotent."""
    global _installed
    if _installed is not None:
        return
    import triro.backend.ops as ops
    import triro.ray.sharded as sharded
    saved = []
    for mod in (ops, sharded):
        saved.append((mod, "_new_output", mod._new_output))
        mod._new_output = poisoned
    for name in ENTRY_POINTS:
        saved.append((ops, name, getattr(ops, name)))
        setattr(ops, name, _checked(getattr(ops, name), name))
    _installed = saved


def uninstall():
    global _installed
    if _installed is None:
        return
    for mod, name, original in reversed(_installed):
        setattr(mod, name, original)
    _installed = None


def installed() -> bool:
    return _installed is not None


@pytest.fixture(autouse=True)
def poisoned_outputs():
    """autouse in every module that imports it: each test of that module runs with poisoned outputs"""
    install()
    try:
        yield
    finally:
        uninstall()
