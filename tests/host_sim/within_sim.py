"""ctypes front-end of tests/host_sim/libwithin_sim.so (TEST-ONLY: csrc/tr_within.h built for the host, within_sim.cpp).
brute() keeps every active triangle with d2 <= R2 of the per-triangle function, in face order; walk() is the fixed-radius
walk (any, count, fill + ordering) and the bounded nearest walk on a sim.SimBVH.  Both return a Result."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# any bool [n], count int32 [n], offsets int64 [n + 1], faces int32 [h], distance float32 [h], closest float32 [h, 3],
# nearest = (closest [n, 3], distance [n], tri [n]) of the bounded nearest
Result = collections.namedtuple("Result", "any count offsets faces distance closest nearest")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libwithin_sim.so")
        src = os.path.join(_HERE, "within_sim.cpp")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_nearest.h", "tr_within.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sim_within_brute.restype = None
        L.sim_within_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        L.sim_within_brute_closest.restype = None
        L.sim_within_brute_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.sim_within_walk.restype = None
        L.sim_within_walk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int] + \
            [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 5
        L.sim_within_walk_closest.restype = None
        L.sim_within_walk_closest.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_within_stack_capacity())


def radii(radius, n):
    """a scalar or [n] radius as the dense float32 [n] the library reads"""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), (n,)))


def _offsets(count):
    off = np.zeros(len(count) + 1, np.int64)
    np.cumsum(count, out=off[1:])
    return off


def brute(vertices, faces, points, radius):
    """Result by evaluating every triangle; nearest carries a fourth entry, the winner's float64 d2 (+Inf: none)"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    r = radii(radius, n)
    count = np.zeros(n, np.int32)
    L = lib()
    L.sim_within_brute(v.ctypes.data, f.ctypes.data, len(f), p.ctypes.data, n, r.ctypes.data, count.ctypes.data, None, None, None, None)
    off = _offsets(count)
    h = int(off[-1])
    face, dist, clo = np.full(h, -7, np.int32), np.zeros(h, np.float32), np.zeros((h, 3), np.float32)
    L.sim_within_brute(v.ctypes.data, f.ctypes.data, len(f), p.ctypes.data, n, r.ctypes.data, None, off.ctypes.data, face.ctypes.data,
                       dist.ctypes.data, clo.ctypes.data)
    nc, nd, nt, nd2 = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    L.sim_within_brute_closest(v.ctypes.data, f.ctypes.data, len(f), p.ctypes.data, n, r.ctypes.data, nc.ctypes.data, nd.ctypes.data,
                               nt.ctypes.data, nd2.ctypes.data)
    return Result(count > 0, count, off, face, dist, clo, (nc, nd, nt, nd2))


def walk(B, points, radius, stack_entries=0, want_lost=False, nearest_entries=None):
    """Result of the walks on the sim.SimBVH `B`: any, count and the fill each walk on their own, at `stack_entries`; the
    bounded nearest at `nearest_entries` (default: the same).  want_lost: (Result, lost [n] bool of the count walk)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    r = radii(radius, n)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    L = lib()

    def run(mode, out, count=None, off=None, total=0, rows=(None,) * 4, lost=None):
        L.sim_within_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, p.ctypes.data, n, r.ctypes.data,
                          int(stack_entries), mode, None if out is None else out.ctypes.data,
                          None if count is None else count.ctypes.data, None if off is None else off.ctypes.data, total,
                          *(None if x is None else x.ctypes.data for x in rows), None if lost is None else lost.ctypes.data)
    any_, count, lost = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    run(0, any_)
    run(1, count, lost=lost)
    off = _offsets(count)
    h = int(off[-1])
    face, slot, dist, clo = np.full(h, -7, np.int32), np.full(h, -7, np.int32), np.zeros(h, np.float32), np.zeros((h, 3), np.float32)
    run(2, None, count, off, h, (face, slot, dist, clo))
    nc, nd, nt = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    L.sim_within_walk_closest(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, p.ctypes.data, n, r.ctypes.data,
                              int(stack_entries if nearest_entries is None else nearest_entries), nc.ctypes.data, nd.ctypes.data, nt.ctypes.data)
    res = Result(any_ != 0, count, off, face, dist, clo, (nc, nd, nt))
    return (res, lost.astype(bool)) if want_lost else res
