"""ctypes front-end of tests/host_sim/libscene_points_sim.so (TEST-ONLY: csrc/tr_scene_points.h built for the host,
scene_points_sim.cpp), and the brute force of contains_points on instanced scenes.

walk(hierarchies, ...)  -> tr_scene_points_query (any, count, then the fill), the per-lane instance loop with its two passes,
                           on sim.SimBVH trees, at a stack limit, in a visiting order, with or without the shortcut
brute(members, ...)     -> a SECOND computation, in numpy, composed of two brute forces that exist without this feature:
                           the counts of cross_sim.brute (tr_range_tri on every triangle of one mesh, default bounds) per
                           instance on the rays of scene_sim.transform for +d and for -d, then the parity in numpy
counts(members, ...)    -> the per-instance counts (c+ [ninst, n], c- [ninst, n]) that brute() reduces

members: a list of (vertices [nv, 3], faces [nf, 3]); hierarchies: a list of sim.SimBVH; mesh_of_instance int32 [ninst];
M: [ninst, 3, 4], [ninst, 4, 4] or [ninst, 12]; points [n, 3]; direction [3].  Both return a Result."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import cross_sim
import scene_sim

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
SOURCE = os.path.join(_HERE, "scene_points_sim.cpp")
FLAGS = cross_sim.FLAGS

# any bool [n], count int32 [n], offsets int64 [n + 1], instance int32 [h]
Result = collections.namedtuple("Result", "any count offsets instance")
KEYS = Result._fields


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libscene_points_sim.so")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(SOURCE)] + [os.path.getmtime(os.path.join(hdr, h)) for h in
                                                   ("tr_math.h", "tr_bvh.h", "tr_range.h", "tr_cross.h", "tr_scene.h", "tr_scene_cross.h",
                                                    "tr_points.h", "tr_scene_points.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", so, SOURCE])
        L = C.CDLL(so)
        vp, i64 = C.c_void_p, C.c_int64
        L.sim_scene_points_walk.restype = None
        L.sim_scene_points_walk.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, i64, C.c_int, C.c_int, C.c_int] + [vp] * 4 + [i64, vp, vp]
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_scene_points_stack_capacity())


_ptr = cross_sim._ptr
offsets_of = cross_sim.offsets_of


def _query(points, direction):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(direction, np.float32).reshape(3)
    return p, d


def counts(members, mesh_of_instance, M, points, direction):
    """(c+ int32 [ninst, n], c- int32 [ninst, n]): the counts of cross_sim.brute per instance on the transformed rays of
    (p, d) and (p, -d); zero where the instance is invalid, the member has no face, or the world or the transformed ray has
    a non-finite component"""
    p, d = _query(points, direction)
    n = len(p)
    mesh_of, M12 = scene_sim._instances(mesh_of_instance, M, len(members))
    valid = scene_sim.record(M12)[1] if len(mesh_of) else []
    with np.errstate(invalid="ignore"):
        world_ok = np.isfinite(p).all(1) & bool(np.isfinite(d).all())
    out = np.zeros((2, len(mesh_of), n), np.int32)
    for s, dd in enumerate((d, -d)):      # (the exact negation of the world direction, before the transform)
        dirs = np.ascontiguousarray(np.broadcast_to(dd, (n, 3)))
        for k in range(len(mesh_of)):
            v, f = members[mesh_of[k]]
            if not valid[k] or len(f) == 0:
                continue
            o2, d2, ok = scene_sim.transform(M12[k], p, dirs)
            out[s, k] = np.where(ok & world_ok, cross_sim.brute(v, f, o2, d2).count, 0)
    return out[0], out[1]


def reduce(cp, cm):
    """the parity rule in numpy on counts [ninst, n] -> Result"""
    inside = ((cp & 1) == 1) & ((cm & 1) == 1)                      # [ninst, n]
    count = inside.sum(0).astype(np.int32)
    pt, inst = np.nonzero(inside.T)                                # ordered by (point, instance)
    return Result(count > 0, count, offsets_of(count), inst.astype(np.int32))


def brute(members, mesh_of_instance, M, points, direction):
    """Result by counting every triangle of every instance on both rays: see the module docstring"""
    return reduce(*counts(members, mesh_of_instance, M, points, direction))


def walk(hierarchies, mesh_of_instance, M, points, direction, stack_entries=0, order=None, both=False, want_lost=False, count=None, total=None):
    """Result of the per-lane query on the sim.SimBVH trees at `stack_entries`, instances visited in `order` (None:
    ascending): the any query, the count query, then the fill.  both: the second pass walked whatever the first count.
    count / total (default: the count query's own): what the fill is handed instead; rows nobody wrote hold -7.
    want_lost: (Result, lost_inst int32 [n] of the count query: the last instance visited in which a pass overflowed, -1 none)"""
    arrays = [[np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris)] for B in hierarchies]
    nf = np.array([B.nf for B in hierarchies] + [0], np.int64)
    mesh_of, M12 = scene_sim._instances(mesh_of_instance, M, len(hierarchies))
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    assert order is None or sorted(order.tolist()) == list(range(len(mesh_of)))
    p, d = _query(points, direction)
    n = len(p)
    L = lib()
    pn, pl, pt = (scene_sim._ptrs([a[j] for a in arrays]) for j in range(3))

    def run(mode, out8=None, out32=None, cnt=None, off=None, tot=0, inst=None, lost=None):
        L.sim_scene_points_walk(pn, pl, pt, nf.ctypes.data, len(hierarchies), mesh_of.ctypes.data, M12.ctypes.data, len(mesh_of), _ptr(order),
                                p.ctypes.data, d.ctypes.data, n, int(stack_entries), int(bool(both)), mode, _ptr(out8), _ptr(out32), _ptr(cnt),
                                _ptr(off), tot, _ptr(inst), _ptr(lost))
    any_, own, lost = np.full(n, 7, np.uint8), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    run(0, out8=any_)
    run(1, out32=own, lost=lost)
    assert (any_ <= 1).all()
    cnt = own if count is None else np.ascontiguousarray(count, np.int32)
    off = offsets_of(cnt)
    h = int(off[-1]) if total is None else int(total)
    inst = np.full(h, -7, np.int32)
    run(2, cnt=cnt, off=off, tot=h, inst=inst)
    res = Result(any_.astype(bool), own, off, inst)
    return (res, lost) if want_lost else res
