"""ctypes front-end of tests/host_sim/libtris_sim.so (TEST-ONLY: csrc/tr_tris.h built for the host, tris_sim.cpp).
brute() keeps every active triangle that the predicate tr_tris_meets says meets the query triangle, in face order; walk() is
the set walk (any, count, fill + ordering) on a sim.SimBVH.  Both return a Result."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# any bool [n], count int32 [n], offsets int64 [n + 1], faces int32 [h]
Result = collections.namedtuple("Result", "any count offsets faces")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libtris_sim.so")
        src = os.path.join(_HERE, "tris_sim.cpp")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr, h))
                                                for h in ("tr_math.h", "tr_bvh.h", "tr_nearest.h", "tr_within.h", "tr_boxes.h", "tr_tris.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sim_tris_brute.restype = None
        L.sim_tris_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        L.sim_tris_walk.restype = None
        L.sim_tris_walk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int] + \
            [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 2
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_tris_stack_capacity())


def triangles(tri):
    """the query triangles as the dense float32 [n, 9] array the library reads"""
    return np.ascontiguousarray(tri, np.float32).reshape(-1, 9)


def _offsets(count):
    off = np.zeros(len(count) + 1, np.int64)
    np.cumsum(count, out=off[1:])
    return off


def brute(vertices, faces, tri):
    """Result by evaluating every triangle"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    tri = triangles(tri)
    n = len(tri)
    count = np.zeros(n, np.int32)
    L = lib()
    L.sim_tris_brute(v.ctypes.data, f.ctypes.data, len(f), tri.ctypes.data, n, count.ctypes.data, None, None)
    off = _offsets(count)
    h = int(off[-1])
    face = np.full(h, -7, np.int32)
    L.sim_tris_brute(v.ctypes.data, f.ctypes.data, len(f), tri.ctypes.data, n, None, off.ctypes.data, face.ctypes.data)
    return Result(count > 0, count, off, face)


def walk(B, tri, stack_entries=0, want_lost=False):
    """Result of the walk on the sim.SimBVH `B`: any, count and the fill each walk on their own, at `stack_entries`.
    want_lost: (Result, lost [n] bool of the count walk)"""
    tri = triangles(tri)
    n = len(tri)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    L = lib()

    def run(mode, out, count=None, off=None, total=0, face=None, lost=None):
        L.sim_tris_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, tri.ctypes.data, n, int(stack_entries), mode,
                        None if out is None else out.ctypes.data, None if count is None else count.ctypes.data,
                        None if off is None else off.ctypes.data, total, None if face is None else face.ctypes.data,
                        None if lost is None else lost.ctypes.data)
    any_, count, lost = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    run(0, any_)
    run(1, count, lost=lost)
    off = _offsets(count)
    h = int(off[-1])
    face = np.full(h, -7, np.int32)
    run(2, None, count, off, h, face)
    res = Result(any_ != 0, count, off, face)
    return (res, lost.astype(bool)) if want_lost else res
