"""ctypes front-end of tests/host_sim/libtrip_model.so (TEST-ONLY: trip_model.cpp = plain_sim.cpp plus the fused trip with the
plain far-child stack by LDS byte address, with per-ray trip counters).  Hierarchies are built with sim.SimBVH."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
PER_RAY = ("trips", "nodes", "stalls", "leaf_only", "first_hit", "entries_at_first_hit")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libtrip_model.so")
        srcs = [os.path.join(_HERE, s) for s in ("trip_model.cpp", "plain_sim.cpp", "host_sim.cpp")]
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(s) for s in srcs] +
                     [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_lbvh.h", "tr_wide.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.sim_set_qnodes.argtypes = [C.c_void_p] * 2
        L.sim_addr_query.restype = C.c_int
        L.sim_addr_query.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 7
        L.sim_addr_lost.restype = C.c_int64
        L.sim_addr_lost.argtypes = []
        _LIB = L
    return _LIB


def query(B, q, o, d, per_ray=False):
    """q = 0 any, 1 first, 2 closest on the sim.SimBVH `B` through the address form -> the dict of plain_sim.query; with
    per_ray also `per_ray`: an (n, 6) int32 array of PER_RAY"""
    L = lib()
    L.sim_set_qnodes(B.qnodes.ctypes.data, B.frame.ctypes.data)
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    n = len(o)
    hit = np.zeros(n, np.uint8); front = np.zeros(n, np.uint8); tri = np.zeros(n, np.int32)
    loc = np.zeros((n, 3), np.float32); uv = np.zeros((n, 2), np.float32)
    stats = np.zeros(4, np.uint64)
    pr = np.zeros((n, 6), np.int32) if per_ray else None
    rc = L.sim_addr_query(q, B.nodes.ctypes.data, B.links.ctypes.data, B.tris.ctypes.data, B.nf, o.ctypes.data, d.ctypes.data,
                          n, hit.ctypes.data, front.ctypes.data, tri.ctypes.data, loc.ctypes.data, uv.ctypes.data,
                          stats.ctypes.data, pr.ctypes.data if per_ray else None)
    if rc != 0:
        raise ValueError(f"the plain walk runs closest / first / any, not query {q}")
    out = dict(hit=hit.astype(bool), front=front.astype(bool), tri=tri, loc=loc, uv=uv, stats=stats, lost=int(L.sim_addr_lost()))
    if per_ray:
        out["per_ray"] = pr
    return out
