"""ctypes front-end of tests/host_sim/libscene_nearest_sim.so (TEST-ONLY: csrc/tr_scene_nearest.h built for the host,
scene_nearest_sim.cpp), and the brute force of closest_point on instanced scenes.

walk(hierarchies, ...)  -> tr_scene_near_query, the per-lane instance loop, on sim.SimBVH trees, at a stack limit, in a
                           visiting order
bake(members, ...)      -> the baked mesh of the contract: in instance order, the faces of every valid instance with vertices
                           placed by scene_sim.points (the scene's fmaf chain) in float32
brute(members, ...)     -> a SECOND computation: bake, then nearest_sim.brute (unbounded) or within_sim's bounded nearest by
                           brute force on the baked mesh, and the baked face index mapped back to (instance, tri)
place / bound / d2      -> the placed box, its bound and the per-triangle function on their own (the culling proof)

members: a list of (vertices [nv, 3], faces [nf, 3]); hierarchies: a list of sim.SimBVH; mesh_of_instance int32 [ninst];
M: [ninst, 3, 4], [ninst, 4, 4] or [ninst, 12]; points [n, 3]; max_distance: None (unbounded), a number or [n].
walk and brute return a Result."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import cross_sim
import nearest_sim
import scene_sim
import within_sim

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
SOURCE = os.path.join(_HERE, "scene_nearest_sim.cpp")
FLAGS = cross_sim.FLAGS
HEADERS = ("tr_math.h", "tr_bvh.h", "tr_range.h", "tr_scene.h", "tr_nearest.h", "tr_within.h", "tr_scene_nearest.h")

# closest float32 [n, 3], distance float32 [n], instance int32 [n], tri int32 [n]
Result = collections.namedtuple("Result", "closest distance instance tri")
KEYS = Result._fields


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libscene_nearest_sim.so")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(SOURCE)] + [os.path.getmtime(os.path.join(hdr, h)) for h in HEADERS])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", so, SOURCE])
        _LIB = bind(C.CDLL(so))
    return _LIB


def bind(L):
    vp, i64 = C.c_void_p, C.c_int64
    L.sim_scene_nearest_walk.restype = None
    L.sim_scene_nearest_walk.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, i64, C.c_int] + [vp] * 5
    L.sim_scene_nearest_place.restype = None
    L.sim_scene_nearest_place.argtypes = [vp, vp, vp, i64, vp, vp]
    L.sim_scene_nearest_bound.restype = None
    L.sim_scene_nearest_bound.argtypes = [vp, vp, vp, vp, i64, vp]
    L.sim_scene_nearest_d2.restype = None
    L.sim_scene_nearest_d2.argtypes = [vp, vp, i64, vp]
    return L


def stack_capacity():
    return int(lib().sim_scene_nearest_stack_capacity())


_ptr = cross_sim._ptr


def radii(max_distance, n):
    """None (unbounded), a scalar or [n] as the dense float32 [n] the library reads"""
    return within_sim.radii(np.inf if max_distance is None else max_distance, n)


def bake(members, mesh_of_instance, M):
    """(v float32 [nv, 3], f int32 [F, 3], inst_of_face int32 [F], tri_of_face int32 [F]) of the baked mesh"""
    mesh_of, M12 = scene_sim._instances(mesh_of_instance, M, len(members))
    valid = scene_sim.record(M12)[1] if len(mesh_of) else []
    vs, fs, inst, tri = [np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.int32)], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)]
    nv = 0
    for k in range(len(mesh_of)):
        v, f = members[mesh_of[k]]
        if not valid[k] or len(f) == 0:
            continue
        with np.errstate(all="ignore"):
            vs.append(scene_sim.points(M12[k], v))
        fs.append(np.asarray(f, np.int32) + nv)
        inst.append(np.full(len(f), k, np.int32))
        tri.append(np.arange(len(f), dtype=np.int32))
        nv += len(v)
    return np.concatenate(vs), np.concatenate(fs), np.concatenate(inst), np.concatenate(tri)


def brute(members, mesh_of_instance, M, points, max_distance=None, want_d2=False):
    """Result by baking and evaluating every placed triangle: see the module docstring.  want_d2: (Result, the winner's float64
    squared distance [n], +Inf for none)"""
    v, f, inst_of, tri_of = bake(members, mesh_of_instance, M)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    if max_distance is None and not want_d2:
        closest, distance, t = nearest_sim.brute(v, f, p)
        d2 = None
    else:
        r = radii(max_distance, n)
        closest, distance, t, d2 = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float64)
        within_sim.lib().sim_within_brute_closest(v.ctypes.data, f.ctypes.data, len(f), p.ctypes.data, n, r.ctypes.data, closest.ctypes.data,
                                                  distance.ctypes.data, t.ctypes.data, d2.ctypes.data)
    hit = t >= 0
    safe = np.maximum(t, 0)
    res = Result(closest, distance, np.where(hit, inst_of[safe] if len(inst_of) else -1, -1).astype(np.int32),
                 np.where(hit, tri_of[safe] if len(tri_of) else -1, -1).astype(np.int32))
    return (res, d2) if want_d2 else res


def walk(hierarchies, mesh_of_instance, M, points, max_distance=None, stack_entries=0, order=None, want_lost=False, outputs=KEYS, L=None):
    """Result of the per-lane query on the sim.SimBVH trees at `stack_entries`, instances visited in `order` (None: ascending).
    outputs: the optional ones (closest, distance) not named are left out (None in the Result).  want_lost: (Result, lost bool
    [n]: some instance's first walk overflowed its stack).  L: another build of the library (a mutant)"""
    arrays = [[np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris)] for B in hierarchies]
    nf = np.array([B.nf for B in hierarchies] + [0], np.int64)
    mesh_of, M12 = scene_sim._instances(mesh_of_instance, M, len(hierarchies))
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    assert order is None or sorted(order.tolist()) == list(range(len(mesh_of)))
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    r = radii(max_distance, n)
    pn, pl, pt = (scene_sim._ptrs([a[j] for a in arrays]) for j in range(3))
    closest = np.full((n, 3), 7, np.float32) if "closest" in outputs else None
    distance = np.full(n, 7, np.float32) if "distance" in outputs else None
    inst, tri, lost = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, 7, np.uint8)
    (L or lib()).sim_scene_nearest_walk(pn, pl, pt, nf.ctypes.data, len(hierarchies), mesh_of.ctypes.data, M12.ctypes.data, len(mesh_of),
                                        _ptr(order), p.ctypes.data, r.ctypes.data, n, int(stack_entries), _ptr(closest), _ptr(distance),
                                        inst.ctypes.data, tri.ctypes.data, lost.ctypes.data)
    res = Result(closest, distance, inst, tri)
    return (res, lost.astype(bool)) if want_lost else res


def _boxes(M, lo, hi):
    M = np.ascontiguousarray(np.asarray(M, np.float32).reshape(-1)[:12])
    lo = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
    assert lo.shape == hi.shape
    return M, lo, hi


def place(M, lo, hi, L=None):
    """(LO, HI) float32 [n, 3]: the object-space boxes [lo, hi] placed by the 3 x 4 map M (tr_scene_near_place)"""
    M, lo, hi = _boxes(M, lo, hi)
    LO, HI = np.zeros_like(lo), np.zeros_like(hi)
    (L or lib()).sim_scene_nearest_place(M.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(lo), LO.ctypes.data, HI.ctypes.data)
    return LO, HI


def bound(M, points, lo, hi, L=None):
    """float64 [n]: tr_scene_near_bound of point i against the object-space box i placed by M"""
    M, lo, hi = _boxes(M, lo, hi)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    assert p.shape == lo.shape
    out = np.zeros(len(p), np.float64)
    (L or lib()).sim_scene_nearest_bound(M.ctypes.data, p.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(p), out.ctypes.data)
    return out


def d2(points, abc):
    """float64 [n]: tr_near_tri(point i, triangle i).d2 for triangles abc [n, 3, 3] (float32), +Inf for an inactive one"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(abc, np.float32).reshape(-1, 9)
    assert len(p) == len(t)
    out = np.zeros(len(p), np.float64)
    lib().sim_scene_nearest_d2(p.ctypes.data, t.ctypes.data, len(p), out.ctypes.data)
    return out
