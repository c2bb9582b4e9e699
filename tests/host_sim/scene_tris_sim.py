"""ctypes front-end of tests/host_sim/libscene_tris_sim.so (TEST-ONLY: csrc/tr_scene_tris.h built for the host,
scene_tris_sim.cpp), and the brute force of the triangle queries on instanced scenes.

brute(members, ...)     -> a SECOND computation: scene_nearest_sim.bake (the placed copies as one float32 mesh, by the scene's
                           fmaf chain), then tris_sim.brute on the baked mesh, and the baked face index mapped back to
                           (instance, face): ascending baked index is ascending (instance, face)
walk(hierarchies, ...)  -> tr_scene_tris_query, the per-lane instance loop, on sim.SimBVH trees: any, count and the fill each
                           walk on their own, at a stack limit, in a visiting order
apart / meets           -> the culling test and the predicate on placed vertices on their own (the culling proof)

members: a list of (vertices [nv, 3], faces [nf, 3]); hierarchies: a list of sim.SimBVH; mesh_of_instance int32 [ninst];
M: [ninst, 3, 4], [ninst, 4, 4] or [ninst, 12]; tri [n, 3, 3].  walk and brute return a Result."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import cross_sim
import scene_nearest_sim
import scene_sim
import tris_sim

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
SOURCE = os.path.join(_HERE, "scene_tris_sim.cpp")
FLAGS = cross_sim.FLAGS
HEADERS = ("tr_math.h", "tr_bvh.h", "tr_walk.h", "tr_range.h", "tr_scene.h", "tr_nearest.h", "tr_within.h", "tr_boxes.h", "tr_tris.h",
           "tr_scene_nearest.h", "tr_scene_tris.h")

# any bool [n], count int32 [n], offsets int64 [n + 1], instance int32 [h], face int32 [h]
Result = collections.namedtuple("Result", "any count offsets instance face")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libscene_tris_sim.so")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(SOURCE)] + [os.path.getmtime(os.path.join(hdr, h)) for h in HEADERS])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", so, SOURCE])
        _LIB = bind(C.CDLL(so))
    return _LIB


def bind(L):
    vp, i64 = C.c_void_p, C.c_int64
    L.sim_scene_tris_walk.restype = None
    L.sim_scene_tris_walk.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, C.c_int, C.c_int, vp, vp, vp, i64, vp, vp, vp]
    L.sim_scene_tris_apart.restype = None
    L.sim_scene_tris_apart.argtypes = [vp, vp, vp, vp, i64, vp]
    L.sim_scene_tris_meets.restype = None
    L.sim_scene_tris_meets.argtypes = [vp, vp, vp, i64, vp]
    return L


def stack_capacity():
    return int(lib().sim_scene_tris_stack_capacity())


_ptr = cross_sim._ptr
triangles = tris_sim.triangles
bake = scene_nearest_sim.bake


def brute(members, mesh_of_instance, M, tri):
    """Result by baking and evaluating every placed triangle: see the module docstring"""
    v, f, inst_of, tri_of = bake(members, mesh_of_instance, M)
    r = tris_sim.brute(v, f, tri)
    return Result(r.any, r.count, r.offsets, inst_of[r.faces].astype(np.int32), tri_of[r.faces].astype(np.int32))


def walk(hierarchies, mesh_of_instance, M, tri, stack_entries=0, order=None, want_lost=False, L=None):
    """Result of the per-lane query on the sim.SimBVH trees at `stack_entries`, instances visited in `order` (None: ascending).
    want_lost: (Result, lost bool [n]: some instance's first walk of the COUNT query overflowed its stack).  L: another build
    of the library (a mutant)"""
    arrays = [[np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris)] for B in hierarchies]
    nf = np.array([B.nf for B in hierarchies] + [0], np.int64)
    mesh_of, M12 = scene_sim._instances(mesh_of_instance, M, len(hierarchies))
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    assert order is None or sorted(order.tolist()) == list(range(len(mesh_of)))
    tri = triangles(tri)
    n = len(tri)
    pn, pl, pt = (scene_sim._ptrs([a[j] for a in arrays]) for j in range(3))
    L = L or lib()

    def run(mode, out, count=None, off=None, total=0, inst=None, face=None, lost=None):
        L.sim_scene_tris_walk(pn, pl, pt, nf.ctypes.data, len(hierarchies), mesh_of.ctypes.data, M12.ctypes.data, len(mesh_of), _ptr(order),
                              tri.ctypes.data, n, int(stack_entries), mode, _ptr(out), _ptr(count), _ptr(off), total, _ptr(inst), _ptr(face),
                              _ptr(lost))
    any_, count, lost = np.full(n, 7, np.int32), np.full(n, -7, np.int32), np.full(n, 7, np.uint8)
    run(0, any_)
    run(1, count, lost=lost)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(count, out=off[1:])
    h = int(off[-1])
    inst, face = np.full(h, -7, np.int32), np.full(h, -7, np.int32)
    run(2, None, count, off, h, inst, face)
    res = Result(any_ != 0, count, off, inst, face)
    return (res, lost.astype(bool)) if want_lost else res


def _m12(M):
    return np.ascontiguousarray(np.asarray(M, np.float32).reshape(-1)[:12])


def apart(M, tri, lo, hi, L=None):
    """bool [n]: tr_scene_tris_apart -- the object-space box i placed by the 3 x 4 map M is proven apart from the box of
    query triangle i"""
    tri = triangles(tri)
    lo = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
    assert len(lo) == len(hi) == len(tri)
    out = np.full(len(tri), 7, np.uint8)
    M = _m12(M)
    (L or lib()).sim_scene_tris_apart(M.ctypes.data, tri.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(tri), out.ctypes.data)
    return out.astype(bool)


def meets(M, tri, abc, L=None):
    """bool [n]: contract 2 -- query triangle i meets the member triangle abc[i] ([n, 3, 3], object space) placed by M"""
    tri, abc = triangles(tri), triangles(abc)
    assert len(tri) == len(abc)
    out = np.full(len(tri), 7, np.uint8)
    M = _m12(M)
    (L or lib()).sim_scene_tris_meets(M.ctypes.data, tri.ctypes.data, abc.ctypes.data, len(tri), out.ctypes.data)
    return out.astype(bool)
