"""ctypes front-end of tests/host_sim/libpoints_sim.so (TEST-ONLY: points_sim.cpp = host_sim.cpp plus the per-point routine of
contains_points).  Hierarchies are built with sim.SimBVH; contains() runs both rays of every point and the decision function
of csrc/tr_points.h."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libpoints_sim.so")
        srcs = [os.path.join(_HERE, "points_sim.cpp"), os.path.join(_HERE, "host_sim.cpp")]
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(s) for s in srcs] +
                     [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_lbvh.h", "tr_wide.h", "tr_points.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.sim_set_qnodes.argtypes = [C.c_void_p] * 2
        L.sim_contains_points.restype = None
        L.sim_contains_points.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 7
        _LIB = L
    return _LIB


def contains(B, points, direction, box=None):
    """both rays of every point on the sim.SimBVH `B` -> dict(inside, broken, counts [2, n], summary [2]); box = (lo, hi) or
    None for no box test"""
    L = lib()
    L.sim_set_qnodes(B.qnodes.ctypes.data, B.frame.ctypes.data)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(direction, np.float32).reshape(3)
    n = len(p)
    lo = hi = None
    if box is not None:
        lo, hi = (np.ascontiguousarray(b, np.float32).reshape(3) for b in box)
    inside = np.zeros(n, np.uint8); broken = np.zeros(n, np.uint8)
    counts = np.zeros((2, n), np.int32); summary = np.zeros(2, np.int64)
    L.sim_contains_points(B.nodes.ctypes.data, B.links.ctypes.data, B.tris.ctypes.data, B.nf, p.ctypes.data, n, d.ctypes.data,
                          lo.ctypes.data if lo is not None else None, hi.ctypes.data if hi is not None else None,
                          inside.ctypes.data, broken.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    return dict(inside=inside.astype(bool), broken=broken.astype(bool), counts=counts, summary=summary)
