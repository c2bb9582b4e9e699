"""ctypes front-end of tests/host_sim/libnearest_sim.so (TEST-ONLY: csrc/tr_nearest.h built for the host, nearest_sim.cpp).
brute() is the per-triangle function over every triangle with the lexicographic minimum; walk() is the nearest-triangle
walk on a sim.SimBVH."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libnearest_sim.so")
        src = os.path.join(_HERE, "nearest_sim.cpp")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_nearest.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sim_nearest_brute.restype = None
        L.sim_nearest_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        L.sim_nearest_walk.restype = None
        L.sim_nearest_walk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 4
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_nearest_stack_capacity())


def _outputs(n):
    return np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)


def brute(vertices, faces, points):
    """(closest [n, 3] float32, distance [n] float32, tri [n] int32) by evaluating every triangle"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    closest, distance, tri = _outputs(len(p))
    lib().sim_nearest_brute(v.ctypes.data, f.ctypes.data, len(f), p.ctypes.data, len(p), closest.ctypes.data,
                            distance.ctypes.data, tri.ctypes.data)
    return closest, distance, tri


def walk(B, points, stack_entries=0, want_lost=False):
    """the walk on the sim.SimBVH `B` (its nodes, links and tris): (closest, distance, tri[, lost])"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    closest, distance, tri = _outputs(len(p))
    lost = np.zeros(len(p), np.uint8)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    lib().sim_nearest_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, p.ctypes.data, len(p), int(stack_entries),
                           closest.ctypes.data, distance.ctypes.data, tri.ctypes.data, lost.ctypes.data)
    return (closest, distance, tri, lost.astype(bool)) if want_lost else (closest, distance, tri)
