"""ctypes front-end of tests/host_sim/libplanes_sim.so (TEST-ONLY: csrc/tr_planes.h built for the host, planes_sim.cpp).
brute() keeps every active triangle that the predicate (tr_plane_meets, or tr_plane_cut with cut=True) says, in face order, with
the segments of the cut faces; walk() is the walk of k_planes<> for a simulated wave of 64 lanes (any, count, fill + ordering +
segments) on a sim.SimBVH.  Both return a Result; order() is the ordering network alone."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# any bool [n], count int32 [n], offsets int64 [n + 1], faces int32 [h], segments float32 [h, 2, 3] (cut only, else None)
Result = collections.namedtuple("Result", "any count offsets faces segments")
# per plane of a walk: rounds of the frontier, steps of the subtree walks, pushes that did not fit
Stats = collections.namedtuple("Stats", "rounds sub_steps overflows")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libplanes_sim.so")
        src = os.path.join(_HERE, "planes_sim.cpp")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr, h))
                                                for h in ("tr_math.h", "tr_bvh.h", "tr_nearest.h", "tr_within.h", "tr_planes.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sim_planes_brute.restype = None
        L.sim_planes_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 4
        L.sim_planes_signed.restype = None
        L.sim_planes_signed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.sim_planes_walk.restype = None
        L.sim_planes_walk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int] + \
            [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3
        L.sim_planes_order.restype = None
        L.sim_planes_order.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.sim_planes_network_pairs.restype = C.c_int64
        L.sim_planes_network_pairs.argtypes = [C.c_uint32, C.c_void_p]
        _LIB = L
    return _LIB


def frontier_capacity():
    return int(lib().sim_planes_frontier_capacity())


def planes(origins, normals):
    """origins, normals as the dense float32 [n, 3] arrays the library reads"""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    assert o.shape == n.shape
    return o, n


def _offsets(count):
    off = np.zeros(len(count) + 1, np.int64)
    np.cumsum(count, out=off[1:])
    return off


def brute(vertices, faces, origins, normals, cut=False):
    """Result by evaluating every triangle"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    o, nr = planes(origins, normals)
    n = len(o)
    count = np.zeros(n, np.int32)
    L = lib()
    L.sim_planes_brute(v.ctypes.data, f.ctypes.data, len(f), o.ctypes.data, nr.ctypes.data, n, int(cut), count.ctypes.data, None, None, None)
    off = _offsets(count)
    h = int(off[-1])
    face = np.full(h, -7, np.int32)
    seg = np.full((h, 2, 3), np.nan, np.float32) if cut else None
    L.sim_planes_brute(v.ctypes.data, f.ctypes.data, len(f), o.ctypes.data, nr.ctypes.data, n, int(cut), None, off.ctypes.data,
                       face.ctypes.data, None if seg is None else seg.ctypes.data)
    return Result(count > 0, count, off, face, seg)


def signed(vertices, faces, origins, normals):
    """float64 [n, F, 3]: tr_plane_s of the three vertices of every face for every plane"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    o, nr = planes(origins, normals)
    s = np.zeros((len(o), len(f), 3), np.float64)
    lib().sim_planes_signed(v.ctypes.data, f.ctypes.data, len(f), o.ctypes.data, nr.ctypes.data, len(o), s.ctypes.data)
    return s


def walk(B, origins, normals, cut=False, frontier_entries=0, want_stats=False):
    """Result of the simulated wave on the sim.SimBVH `B`: any, count and the fill each walk on their own, at `frontier_entries`.
    want_stats: (Result, Stats of the count walk, arrays [n])"""
    o, nr = planes(origins, normals)
    n = len(o)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    L = lib()

    def run(mode, out, count=None, off=None, total=0, rows=(None, None), stats=None):
        L.sim_planes_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, o.ctypes.data, nr.ctypes.data, n, int(cut),
                          int(frontier_entries), mode, None if out is None else out.ctypes.data,
                          None if count is None else count.ctypes.data, None if off is None else off.ctypes.data, total,
                          *(None if x is None else x.ctypes.data for x in rows), None if stats is None else stats.ctypes.data)
    any_, count, stats = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.int64)
    run(0, any_)
    run(1, count, stats=stats)
    off = _offsets(count)
    h = int(off[-1])
    face = np.full(h, -7, np.int32)
    seg = np.full((h, 2, 3), np.nan, np.float32) if cut else None
    run(2, None, count, off, h, (face, seg))
    res = Result(any_ != 0, count, off, face, seg)
    return (res, Stats(stats[:, 0], stats[:, 1], stats[:, 2])) if want_stats else res


def fill(B, origins, normals, count, offsets, total, face, segments=None, cut=True, frontier_entries=0):
    """the fill alone into the caller's arrays, with the caller's count / offsets / total (the misuse tests)"""
    o, nr = planes(origins, normals)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    count, offsets = np.ascontiguousarray(count, np.int32), np.ascontiguousarray(offsets, np.int64)
    lib().sim_planes_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, o.ctypes.data, nr.ctypes.data, len(o), int(cut),
                          int(frontier_entries), 2, None, count.ctypes.data, offsets.ctypes.data, int(total), face.ctypes.data,
                          None if segments is None else segments.ctypes.data, None)


def order(keys, count, offsets, total=None):
    """the ordering network on a copy of int32 `keys`: segment i = keys[offsets[i] : offsets[i] + count[i]] cut to [0, total)"""
    keys = np.array(keys, np.int32)
    count, offsets = np.ascontiguousarray(count, np.int32), np.ascontiguousarray(offsets, np.int64)
    lib().sim_planes_order(len(count), count.ctypes.data, offsets.ctypes.data, len(keys) if total is None else int(total), keys.ctypes.data)
    return keys


def network_pairs(m):
    """(number of compare-exchanges the network makes on m keys, the largest index it forms)"""
    mx = C.c_uint32(0)
    pairs = lib().sim_planes_network_pairs(int(m), C.byref(mx))
    return int(pairs), int(mx.value)
