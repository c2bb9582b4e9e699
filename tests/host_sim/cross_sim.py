"""ctypes front-end of tests/host_sim/libcross_sim.so (TEST-ONLY: csrc/tr_cross.h built for the host, cross_sim.cpp).
brute() applies the per-triangle predicate of the range contract (tr_range_tri) to every triangle and orders each ray's
rows with numpy.lexsort on (face, t) -- an ordering that shares nothing with the heapsort of tr_cross.h; walk() runs
tr_cross_query (the count, then the fill) and tr_cross_rows on a sim.SimBVH.  Both return a Result."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
SOURCE = os.path.join(_HERE, "cross_sim.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-mfma", "-Wno-unknown-pragmas"]

# count int32 [n], offsets int64 [n + 1], faces int32 [h], t float32 [h], front bool [h], loc float32 [h, 3], uv float32 [h, 2],
# ray int64 [h] (the ray of each row, + ray_base)
Result = collections.namedtuple("Result", "count offsets faces t front loc uv ray")
ROW_KEYS = ("faces", "t", "front", "loc", "uv", "ray")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libcross_sim.so")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(SOURCE)] + [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_range.h", "tr_cross.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", so, SOURCE])
        L = C.CDLL(so)
        L.sim_cross_brute.restype = None
        L.sim_cross_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 7
        L.sim_cross_walk.restype = None
        L.sim_cross_walk.argtypes = [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 3 + \
            [C.c_int64] + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p]
        L.sim_cross_sort.restype = None
        L.sim_cross_sort.argtypes = [C.c_void_p] * 3 + [C.c_int32]
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_cross_stack_capacity())


def _rays(origins, directions, tmin, tmax):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    n = len(o)
    lo = None if tmin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,)))
    hi = None if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
    return o, d, lo, hi


def _ptr(a):
    return None if a is None else a.ctypes.data


def offsets_of(count):
    off = np.zeros(len(count) + 1, np.int64)
    np.cumsum(count, out=off[1:])
    return off


def _rows(h):
    return dict(faces=np.full(h, -7, np.int32), t=np.zeros(h, np.float32), front=np.zeros(h, np.uint8), loc=np.zeros((h, 3), np.float32),
                uv=np.zeros((h, 2), np.float32))


def brute(vertices, faces, origins, directions, tmin=None, tmax=None, ray_base=0):
    """Result by testing every triangle; the rows of a ray ordered by numpy.lexsort on (ray, t, face)"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    o, d, lo, hi = _rays(origins, directions, tmin, tmax)
    n = len(o)
    L = lib()
    count = np.zeros(n, np.int32)
    L.sim_cross_brute(v.ctypes.data, f.ctypes.data, len(f), o.ctypes.data, d.ctypes.data, _ptr(lo), _ptr(hi), n, count.ctypes.data, *([None] * 6))
    off = offsets_of(count)
    h = int(off[-1])
    r = _rows(h)
    L.sim_cross_brute(v.ctypes.data, f.ctypes.data, len(f), o.ctypes.data, d.ctypes.data, _ptr(lo), _ptr(hi), n, None, off.ctypes.data,
                      *(r[k].ctypes.data for k in ("faces", "t", "front", "loc", "uv")))
    ray = np.repeat(np.arange(n, dtype=np.int64), count)
    order = np.lexsort((r["faces"], r["t"], ray))
    return Result(count, off, r["faces"][order], r["t"][order], r["front"][order].astype(bool), r["loc"][order], r["uv"][order], ray + ray_base)


def walk(B, origins, directions, tmin=None, tmax=None, stack_entries=0, want_lost=False, ray_base=0, count=None, total=None):
    """Result of the walk on the sim.SimBVH `B` at `stack_entries`: the count walk, then the fill and the rows function.
    count / total (default: the count walk's own): what the fill is handed instead.  want_lost: (Result, lost [n] bool of
    the count walk)"""
    o, d, lo, hi = _rays(origins, directions, tmin, tmax)
    n = len(o)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    L = lib()

    def run(mode, out, cnt=None, off=None, tot=0, rows=(None,) * 7, lost=None):
        L.sim_cross_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, o.ctypes.data, d.ctypes.data, _ptr(lo), _ptr(hi), n,
                         int(stack_entries), mode, _ptr(out), _ptr(cnt), _ptr(off), tot, *(_ptr(x) for x in rows), int(ray_base), _ptr(lost))
    own, lost = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    run(0, own, lost=lost)
    cnt = own if count is None else np.ascontiguousarray(count, np.int32)
    off = offsets_of(cnt)
    h = int(off[-1]) if total is None else int(total)
    r = _rows(h)
    slot, ray = np.full(h, -7, np.int32), np.full(h, -7, np.int64)
    run(1, None, cnt, off, h, (r["faces"], r["t"], slot, r["front"], r["loc"], r["uv"], ray))
    res = Result(own, off, r["faces"], r["t"], r["front"].astype(bool), r["loc"], r["uv"], ray)
    return (res, lost.astype(bool)) if want_lost else res


def sort(t, face, slot=None):
    """tr_cross_sort on copies of the rows -> (t, face, slot)"""
    t, face = np.array(t, np.float32), np.array(face, np.int32)
    slot = None if slot is None else np.array(slot, np.int32)
    lib().sim_cross_sort(t.ctypes.data, face.ctypes.data, _ptr(slot), len(t))
    return t, face, slot
