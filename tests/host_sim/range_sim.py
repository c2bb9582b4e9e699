"""ctypes front-end of tests/host_sim/librange_sim.so (TEST-ONLY: csrc/tr_range.h built for the host, range_sim.cpp).
brute() applies the per-triangle predicate of the range contract to every triangle: any, and the lexicographic closest
with all its outputs; walk() runs tr_range_query on a sim.SimBVH.  Both return a dict of numpy arrays:
any bool[n]; hit bool[n], front bool[n], tri int32[n], loc float32[n, 3], uv float32[n, 2], t float32[n] of the closest
query; brute adds count int32[n] (accepted triangles) and, with cap > 0, accepted int32[n, cap] (their face indices, -1
beyond the count); walk adds lost_any / lost bool[n] (the first walk of the any / closest query overflowed its stack)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "librange_sim.so")
        src = os.path.join(_HERE, "range_sim.cpp")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_range.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sim_range_brute.restype = None
        L.sim_range_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 9 + [C.c_int32]
        L.sim_range_walk.restype = None
        L.sim_range_walk.argtypes = [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_int] + [C.c_void_p] * 9
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_range_stack_capacity())


def _rays(origins, directions, tmin, tmax):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    n = len(o)
    lo = None if tmin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,)))
    hi = None if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
    return o, d, lo, hi


def _outputs(n):
    return dict(any=np.zeros(n, np.uint8), hit=np.zeros(n, np.uint8), front=np.zeros(n, np.uint8), tri=np.zeros(n, np.int32),
                t=np.zeros(n, np.float32), loc=np.zeros((n, 3), np.float32), uv=np.zeros((n, 2), np.float32))


def _finish(out):
    for k in ("any", "hit", "front", "lost", "lost_any"):
        if k in out:
            out[k] = out[k].astype(bool)
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data


def brute(vertices, faces, origins, directions, tmin=None, tmax=None, cap=0):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    o, d, lo, hi = _rays(origins, directions, tmin, tmax)
    n = len(o)
    out = _outputs(n)
    out["count"] = np.zeros(n, np.int32)
    acc = np.zeros((n, cap), np.int32) if cap > 0 else None
    lib().sim_range_brute(v.ctypes.data, f.ctypes.data, len(f), o.ctypes.data, d.ctypes.data, _ptr(lo), _ptr(hi), n,
                          *(out[k].ctypes.data for k in ("any", "hit", "front", "tri", "t", "loc", "uv", "count")), _ptr(acc), cap)
    if acc is not None:
        out["accepted"] = acc
    return _finish(out)


def walk(B, origins, directions, tmin=None, tmax=None, stack_entries=0):
    o, d, lo, hi = _rays(origins, directions, tmin, tmax)
    n = len(o)
    out = _outputs(n)
    out["lost_any"] = np.zeros(n, np.uint8)
    out["lost"] = np.zeros(n, np.uint8)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    lib().sim_range_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, o.ctypes.data, d.ctypes.data, _ptr(lo), _ptr(hi),
                         n, int(stack_entries),
                         *(out[k].ctypes.data for k in ("any", "hit", "front", "tri", "t", "loc", "uv", "lost_any", "lost")))
    return _finish(out)
