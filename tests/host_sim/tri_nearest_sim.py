"""ctypes front-end of tests/host_sim/libtri_nearest_sim.so (TEST-ONLY: csrc/tr_tri_nearest.h built for the host,
tri_nearest_sim.cpp).  pair() is the distance function of one query triangle and one face in float64; brute() is that function
over every active face with the lexicographic minimum among those within the bound; walk() is the nearest-face walk on a
sim.SimBVH.  brute() and walk() return (tri int32 [n], distance float32 [n], closest_mesh float32 [n, 3], closest_query
float32 [n, 3])."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libtri_nearest_sim.so")
        src = os.path.join(_HERE, "tri_nearest_sim.cpp")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr, h)) for h in
                                                ("tr_math.h", "tr_bvh.h", "tr_walk.h", "tr_nearest.h", "tr_within.h", "tr_boxes.h", "tr_tris.h",
                                                 "tr_tri_nearest.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        L.sim_tri_nearest_pair.restype = None
        L.sim_tri_nearest_pair.argtypes = [C.c_void_p] * 5
        L.sim_tri_nearest_brute.restype = None
        L.sim_tri_nearest_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.sim_tri_nearest_walk.restype = None
        L.sim_tri_nearest_walk.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_tri_nearest_stack_capacity())


def triangles(tri):
    """the query triangles as the dense float32 [n, 9] array the library reads"""
    return np.ascontiguousarray(tri, np.float32).reshape(-1, 9)


def _radii(max_distance, n):
    """None (unbounded), a number or [n] values -> a float32 [n] array or None"""
    if max_distance is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(max_distance, np.float32), (n,)), np.float32)


def _outputs(n):
    return np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)


def pair(query, face):
    """(d2 float64, on_query float64 [3], on_face float64 [3]) of one finite query triangle [3, 3] and one finite face [3, 3]"""
    q, t = triangles(query), triangles(face)
    assert q.shape == (1, 9) and t.shape == (1, 9)
    d2, x, y = C.c_double(), np.zeros(3), np.zeros(3)
    lib().sim_tri_nearest_pair(q.ctypes.data, t.ctypes.data, C.addressof(d2), x.ctypes.data, y.ctypes.data)
    return d2.value, x, y


def pairs_d2(queries, faces):
    """[n, F] float64: pair()'s d2 of every (query, face)"""
    q, t = triangles(queries), triangles(faces)
    out = np.zeros((len(q), len(t)))
    d2, x, y = C.c_double(), np.zeros(3), np.zeros(3)
    fn, ad, ax, ay = lib().sim_tri_nearest_pair, C.addressof(d2), x.ctypes.data, y.ctypes.data
    for i in range(len(q)):
        qi = q[i].ctypes.data
        for j in range(len(t)):
            fn(qi, t[j].ctypes.data, ad, ax, ay)
            out[i, j] = d2.value
    return out


def brute(vertices, faces, tri, max_distance=None):
    """by evaluating every face"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    tri = triangles(tri)
    r = _radii(max_distance, len(tri))
    out = _outputs(len(tri))
    lib().sim_tri_nearest_brute(v.ctypes.data, f.ctypes.data, len(f), tri.ctypes.data, len(tri), None if r is None else r.ctypes.data,
                                *(a.ctypes.data for a in out))
    return out


def walk(B, tri, max_distance=None, stack_entries=0, want_lost=False):
    """the walk on the sim.SimBVH `B` (its nodes, links and tris): (tri, distance, closest_mesh, closest_query[, lost])"""
    tri = triangles(tri)
    r = _radii(max_distance, len(tri))
    out = _outputs(len(tri))
    lost = np.zeros(len(tri), np.uint8)
    nodes, links, tris = (np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris))
    lib().sim_tri_nearest_walk(nodes.ctypes.data, links.ctypes.data, tris.ctypes.data, B.nf, tri.ctypes.data, len(tri),
                               None if r is None else r.ctypes.data, int(stack_entries), *(a.ctypes.data for a in out), lost.ctypes.data)
    return (*out, lost.astype(bool)) if want_lost else out
