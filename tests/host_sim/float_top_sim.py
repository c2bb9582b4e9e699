"""ctypes front-end of tests/host_sim/libfloat_top_model.so (TEST-ONLY: float_top_model.cpp = uniform_top_model.cpp plus the
table loop of the float top -- the wave-uniform top of the tree walked from per-octant tables of pre-selected float planes,
tr_bvh.h: tr_top_rec, tr_top_fill, tr_top_test, tr_top_build_slot).  Hierarchies are built with sim.SimBVH."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
# the variants of float_top_model.cpp: uniform_top_model.cpp's four, the table loop, and its three wrong forms
PHASE, UNIFORM_TOP, WRONG_NO_OCTANT_TEST, WRONG_GOES_ON_AFTER_A_SPLIT = 0, 1, 2, 3
FLOAT_TOP, WRONG_OCTANT_0_FOR_ALL, WRONG_STALE_TABLE, WRONG_GOES_ON_INTO_AN_ABSENT_SLOT = 4, 5, 6, 7
PER_RAY = ("nodes", "tris", "lost")
PER_GROUP = ("first_leaf_trip", "uniform_trips", "longest_lane_trips", "phase_trips", "loop_trips", "octant_fail", "table_trips")
STEAL_MIN, STEAL_EARLY = 64, 4
REC = 64            # bytes of a record
LEVELS = 12         # TR_TOP_LEVELS (tr_bvh.h)


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libfloat_top_model.so")
        srcs = [os.path.join(_HERE, s) for s in ("float_top_model.cpp", "uniform_top_model.cpp", "descent_model.cpp", "plain_sim.cpp",
                                                 "host_sim.cpp")]
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(s) for s in srcs] +
                     [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_lbvh.h", "tr_wide.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.sim_set_qnodes.argtypes = [C.c_void_p] * 2
        L.sim_float_top_build.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.sim_float_top_record.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.sim_float_top_tests.restype = C.c_int
        L.sim_float_top_tests.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
        L.sim_float_top_query.restype = C.c_int
        L.sim_float_top_query.argtypes = ([C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_uint32] +
                                          [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 8)
        L.sim_float_top_lost.restype = C.c_int64
        _LIB = L
    return _LIB


def slots_of(levels):
    return (1 << levels) - 1


def table(qnodes, levels=LEVELS):
    """the eight tables of the grid nodes `qnodes` (an array of 32-byte records of a hierarchy of >= 2 triangles), as
    tr_top_build_slot defines them: uint8 (8, 2^levels - 1, 64)"""
    q = np.ascontiguousarray(qnodes)
    out = np.full((8, slots_of(levels), REC), 0xAB, np.uint8)
    if q.nbytes >= 32:
        lib().sim_float_top_build(q.ctypes.data, q.nbytes // 32, levels, out.ctypes.data)
    else:
        out[:] = 0
    return out


def record(qnode, octant):
    """tr_top_fill of one 32-byte grid node: 16 dwords as uint32"""
    q = np.ascontiguousarray(qnode)
    out = np.zeros(16, np.uint32)
    lib().sim_float_top_record(q.ctypes.data, octant, out.ctypes.data)
    return out


def tests(qnode, frame, o, d, best_t=np.inf):
    """per ray: the planes of the record of the ray's octant (12 floats), the octant, and {a0, a1, lt} of tr_uniform_test
    on the grid node and of tr_top_test on the record"""
    q = np.ascontiguousarray(qnode)
    od = np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)
    n = len(od)
    planes = np.zeros((n, 13), np.float32)
    out = np.zeros((n, 6), np.uint8)
    f6 = np.ascontiguousarray(frame, np.float32)
    rc = lib().sim_float_top_tests(q.ctypes.data, f6.ctypes.data, od.ctypes.data, n, best_t, planes.ctypes.data, out.ctypes.data)
    assert rc == 0, "an invalid ray"
    return planes[:, :12], planes[:, 12].astype(np.int64), out[:, :3].astype(bool), out[:, 3:].astype(bool)


def query(B, q, o, d, variant=FLOAT_TOP, steal_min=STEAL_MIN, levels=LEVELS, top=None):
    """q = 0 any, 1 first, 2 closest on the sim.SimBVH `B`, rays in groups of 64 in the order given -> the outputs of
    uniform_top_sim.query with seven figures per group (PER_GROUP).  The table is B's own of `levels` levels unless `top`
    hands one in (WRONG_STALE_TABLE: one of the hierarchy before a refit)."""
    L = lib()
    L.sim_set_qnodes(B.qnodes.ctypes.data, B.frame.ctypes.data)
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    n = len(o)
    if variant == WRONG_STALE_TABLE:
        assert top is not None, "the stale table is the caller's"
    if top is None and variant >= FLOAT_TOP and B.nf >= 2:
        top = table(B.qnodes, levels)
    tp, slots = (top.ctypes.data, top.shape[1]) if top is not None and variant >= FLOAT_TOP else (None, 0)
    hit = np.zeros(n, np.uint8); front = np.zeros(n, np.uint8); tri = np.zeros(n, np.int32)
    loc = np.zeros((n, 3), np.float32); uv = np.zeros((n, 2), np.float32)
    stats = np.zeros(4, np.uint64)
    pr = np.zeros((n, 3), np.int32)
    pg = np.zeros(((n + 63) // 64, 7), np.int32)
    rc = L.sim_float_top_query(q, variant, steal_min, B.nodes.ctypes.data, B.links.ctypes.data, B.tris.ctypes.data, B.nf,
                               tp, slots, o.ctypes.data, d.ctypes.data, n, hit.ctypes.data, front.ctypes.data, tri.ctypes.data,
                               loc.ctypes.data, uv.ctypes.data, stats.ctypes.data, pr.ctypes.data, pg.ctypes.data)
    if rc != 0:
        raise ValueError(f"the plain walk runs closest / first / any, not query {q}")
    return dict(hit=hit.astype(bool), front=front.astype(bool), tri=tri, loc=loc, uv=uv, stats=stats, per_ray=pr, per_group=pg,
                lost=int(L.sim_float_top_lost()))
