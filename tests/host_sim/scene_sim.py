"""ctypes front-end of tests/host_sim/libscene_sim.so (TEST-ONLY: csrc/tr_scene.h built for the host, scene_sim.cpp).

record(M)                 -> (W float32 [n, 12], valid bool [n], flip bool [n]): the inverse and the flags of placements
transform(M, o, d)        -> (o', d', ok): rays in the frame of ONE placement, by the header's functions
points(A, p)              -> p through the 3 x 4 map A by the contract's fmaf order
brute(members, ...)       -> tr_range_tri on every triangle of every instance, reduced by (t, instance, face)
walk(hierarchies, ...)    -> tr_scene_query, the per-lane instance loop, on sim.SimBVH trees

members: a list of (vertices [nv, 3], faces [nf, 3]); hierarchies: a list of sim.SimBVH; mesh_of_instance int32 [ninst];
M: [ninst, 3, 4], [ninst, 4, 4] (the last row is dropped) or [ninst, 12].  brute and walk return a dict of numpy arrays:
any bool[n]; hit bool[n], front bool[n], instance int32[n], tri int32[n], loc float32[n, 3], uv float32[n, 2], t float32[n]
of the closest query; brute adds count int32[n] (accepted (instance, triangle) pairs), walk adds lost_any / lost bool[n]
(some instance's first walk of the any / closest query overflowed its stack)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

KEYS_ANY = ("any",)
KEYS_CLOSEST = ("hit", "front", "instance", "tri", "loc", "uv", "t")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libscene_sim.so")
        src = os.path.join(_HERE, "scene_sim.cpp")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr, h)) for h in ("tr_math.h", "tr_bvh.h", "tr_range.h", "tr_scene.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-mfma", "-Wno-unknown-pragmas", "-o", so, src])
        L = C.CDLL(so)
        vp, i64 = C.c_void_p, C.c_int64
        L.sim_scene_record.restype = None
        L.sim_scene_record.argtypes = [vp, i64, vp, vp]
        L.sim_scene_transform.restype = None
        L.sim_scene_transform.argtypes = [vp, vp, vp, i64, vp, vp, vp]
        L.sim_scene_points.restype = None
        L.sim_scene_points.argtypes = [vp, vp, i64, vp]
        L.sim_scene_brute.restype = None
        L.sim_scene_brute.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64] + [vp] * 9
        L.sim_scene_walk.restype = None
        L.sim_scene_walk.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, i64, C.c_int] + [vp] * 10
        _LIB = L
    return _LIB


def mat12(M):
    """placements as float32 [n, 12]"""
    M = np.asarray(M, np.float32)
    if M.ndim == 3 and M.shape[1:] == (4, 4):
        M = M[:, :3, :]
    return np.ascontiguousarray(M.reshape(-1, 12))


def record(M):
    M = mat12(M)
    W = np.zeros_like(M)
    flags = np.zeros(len(M), np.int32)
    lib().sim_scene_record(M.ctypes.data, len(M), W.ctypes.data, flags.ctypes.data)
    return W, (flags & 1) != 0, (flags & 2) != 0


def transform(M, origins, directions):
    M = np.asarray(M, np.float32)
    M = mat12(M[None] if M.ndim == 2 else M.reshape(1, 12))      # one placement: [4, 4], [3, 4] or [12]
    assert M.shape == (1, 12)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    o2, d2, ok = np.zeros_like(o), np.zeros_like(d), np.zeros(len(o), np.uint8)
    lib().sim_scene_transform(M.ctypes.data, o.ctypes.data, d.ctypes.data, len(o), o2.ctypes.data, d2.ctypes.data, ok.ctypes.data)
    return o2, d2, ok.astype(bool)


def points(A, p):
    A = np.ascontiguousarray(np.asarray(A, np.float32).reshape(-1)[:12])
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    out = np.zeros_like(p)
    lib().sim_scene_points(A.ctypes.data, p.ctypes.data, len(p), out.ctypes.data)
    return out


def _rays(origins, directions, tmin, tmax):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    n = len(o)
    lo = None if tmin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,)))
    hi = None if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
    return o, d, lo, hi


def _outputs(n):
    return dict(any=np.zeros(n, np.uint8), hit=np.zeros(n, np.uint8), front=np.zeros(n, np.uint8), instance=np.zeros(n, np.int32),
                tri=np.zeros(n, np.int32), t=np.zeros(n, np.float32), loc=np.zeros((n, 3), np.float32), uv=np.zeros((n, 2), np.float32))


def _finish(out):
    for k in ("any", "hit", "front", "lost", "lost_any"):
        if k in out:
            out[k] = out[k].astype(bool)
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data


def _ptrs(arrays):
    return (C.c_void_p * max(len(arrays), 1))(*(a.ctypes.data for a in arrays))


def _instances(mesh_of_instance, M, nmesh):
    mesh_of = np.ascontiguousarray(mesh_of_instance, np.int32).reshape(-1)
    M = mat12(M) if len(mesh_of) else np.zeros((0, 12), np.float32)
    assert len(M) == len(mesh_of) and (len(mesh_of) == 0 or (0 <= mesh_of.min() and mesh_of.max() < nmesh))
    return mesh_of, M


def brute(members, mesh_of_instance, M, origins, directions, tmin=None, tmax=None):
    vs = [np.ascontiguousarray(v, np.float32).reshape(-1, 3) for v, _ in members]
    fs = [np.ascontiguousarray(f, np.int32).reshape(-1, 3) for _, f in members]
    nf = np.array([len(f) for f in fs] + [0], np.int64)
    mesh_of, M = _instances(mesh_of_instance, M, len(members))
    o, d, lo, hi = _rays(origins, directions, tmin, tmax)
    n = len(o)
    out = _outputs(n)
    out["count"] = np.zeros(n, np.int32)
    lib().sim_scene_brute(_ptrs(vs), _ptrs(fs), nf.ctypes.data, len(members), mesh_of.ctypes.data, M.ctypes.data, len(mesh_of),
                          o.ctypes.data, d.ctypes.data, _ptr(lo), _ptr(hi), n,
                          *(out[k].ctypes.data for k in ("any", "hit", "front", "instance", "tri", "t", "loc", "uv", "count")))
    return _finish(out)


def walk(hierarchies, mesh_of_instance, M, origins, directions, tmin=None, tmax=None, stack_entries=0, order=None):
    arrays = [[np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris)] for B in hierarchies]
    nf = np.array([B.nf for B in hierarchies] + [0], np.int64)
    mesh_of, M = _instances(mesh_of_instance, M, len(hierarchies))
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    assert order is None or sorted(order.tolist()) == list(range(len(mesh_of)))
    o, d, lo, hi = _rays(origins, directions, tmin, tmax)
    n = len(o)
    out = _outputs(n)
    out["lost_any"] = np.zeros(n, np.uint8)
    out["lost"] = np.zeros(n, np.uint8)
    lib().sim_scene_walk(_ptrs([a[0] for a in arrays]), _ptrs([a[1] for a in arrays]), _ptrs([a[2] for a in arrays]), nf.ctypes.data,
                         len(hierarchies), mesh_of.ctypes.data, M.ctypes.data, len(mesh_of), _ptr(order), o.ctypes.data, d.ctypes.data,
                         _ptr(lo), _ptr(hi), n, int(stack_entries),
                         *(out[k].ctypes.data for k in ("any", "hit", "front", "instance", "tri", "t", "loc", "uv", "lost_any", "lost")))
    return _finish(out)
