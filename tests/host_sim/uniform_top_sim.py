"""ctypes front-end of tests/host_sim/libuniform_top_model.so (TEST-ONLY: uniform_top_model.cpp = descent_model.cpp plus the
uniform top of wave_traverse_steal -- the loop in front of the descent phase that walks while all visiting lanes of a wave
are at one node and its rays share an octant -- driven through the product's own tr_uniform_test, tr_uniform_wave and
tr_lane_in).  Hierarchies are built with sim.SimBVH."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
PHASE, UNIFORM_TOP, WRONG_NO_OCTANT_TEST, WRONG_GOES_ON_AFTER_A_SPLIT = 0, 1, 2, 3      # the variants of uniform_top_model.cpp
PER_RAY = ("nodes", "tris", "lost")
PER_GROUP = ("first_leaf_trip", "uniform_trips", "longest_lane_trips", "phase_trips", "loop_trips", "octant_fail")
STEAL_MIN, STEAL_EARLY = 64, 4      # the give-away thresholds of a coherent and of an incoherent wave (kernels_direct.inc)


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libuniform_top_model.so")
        srcs = [os.path.join(_HERE, s) for s in ("uniform_top_model.cpp", "descent_model.cpp", "plain_sim.cpp", "host_sim.cpp")]
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(s) for s in srcs] +
                     [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_lbvh.h", "tr_wide.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.sim_set_qnodes.argtypes = [C.c_void_p] * 2
        L.sim_uniform_top_query.restype = C.c_int
        L.sim_uniform_top_query.argtypes = ([C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 3 +
                                            [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 8)
        L.sim_uniform_top_lost.restype = C.c_int64
        _LIB = L
    return _LIB


def query(B, q, o, d, variant=UNIFORM_TOP, steal_min=STEAL_MIN):
    """q = 0 any, 1 first, 2 closest on the sim.SimBVH `B`, rays in groups of 64 in the order given -> the outputs of
    plain_sim.query plus per_ray (n, 3) PER_RAY, per_group (groups, 6) PER_GROUP, lost (rays)"""
    L = lib()
    L.sim_set_qnodes(B.qnodes.ctypes.data, B.frame.ctypes.data)
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    n = len(o)
    hit = np.zeros(n, np.uint8); front = np.zeros(n, np.uint8); tri = np.zeros(n, np.int32)
    loc = np.zeros((n, 3), np.float32); uv = np.zeros((n, 2), np.float32)
    stats = np.zeros(4, np.uint64)
    pr = np.zeros((n, 3), np.int32)
    pg = np.zeros(((n + 63) // 64, 6), np.int32)
    rc = L.sim_uniform_top_query(q, variant, steal_min, B.nodes.ctypes.data, B.links.ctypes.data, B.tris.ctypes.data, B.nf,
                                 o.ctypes.data, d.ctypes.data, n, hit.ctypes.data, front.ctypes.data, tri.ctypes.data,
                                 loc.ctypes.data, uv.ctypes.data, stats.ctypes.data, pr.ctypes.data, pg.ctypes.data)
    if rc != 0:
        raise ValueError(f"the plain walk runs closest / first / any, not query {q}")
    return dict(hit=hit.astype(bool), front=front.astype(bool), tri=tri, loc=loc, uv=uv, stats=stats, per_ray=pr, per_group=pg,
                lost=int(L.sim_uniform_top_lost()))
