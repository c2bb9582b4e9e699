"""ctypes front-end of tests/host_sim/libscene_cross_sim.so (TEST-ONLY: csrc/tr_scene_cross.h built for the host,
scene_cross_sim.cpp), and the brute force of the instanced crossing queries.

walk(hierarchies, ...)  -> tr_scene_cross_query (the count, then the fill) and tr_scene_cross_rows, the per-lane instance loop,
                           on sim.SimBVH trees, at a stack limit and in a visiting order
brute(members, ...)     -> a SECOND computation, in numpy, composed of two brute forces that exist without this feature:
                           cross_sim.brute (tr_range_tri on every triangle, the rows of one mesh) per instance on the rays of
                           scene_sim.transform, the rows of all instances concatenated and ordered by numpy.lexsort on
                           (ray, t, instance, face), front inverted under a mirror, loc through scene_sim.points
sort(t, inst, face)     -> tr_scene_cross_sort on rows handed in

members: a list of (vertices [nv, 3], faces [nf, 3]); hierarchies: a list of sim.SimBVH; mesh_of_instance int32 [ninst];
M: [ninst, 3, 4], [ninst, 4, 4] or [ninst, 12].  Both return a Result."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import cross_sim
import scene_sim

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
SOURCE = os.path.join(_HERE, "scene_cross_sim.cpp")
FLAGS = cross_sim.FLAGS

# count int32 [n], offsets int64 [n + 1], instance int32 [h], faces int32 [h] (the index in the member mesh), t float32 [h],
# front bool [h], loc float32 [h, 3], uv float32 [h, 2], ray int64 [h] (the ray of each row, + ray_base)
Result = collections.namedtuple("Result", "count offsets instance faces t front loc uv ray")
ROW_KEYS = ("instance", "faces", "t", "front", "loc", "uv", "ray")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libscene_cross_sim.so")
        hdr = os.path.join(_HERE, "..", "..", "trimesh-ray-optix_amd", "csrc")
        newest = max([os.path.getmtime(SOURCE)] + [os.path.getmtime(os.path.join(hdr, h)) for h in
                                                   ("tr_math.h", "tr_bvh.h", "tr_range.h", "tr_cross.h", "tr_scene.h", "tr_scene_cross.h")])
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", so, SOURCE])
        L = C.CDLL(so)
        vp, i64 = C.c_void_p, C.c_int64
        L.sim_scene_cross_walk.restype = None
        L.sim_scene_cross_walk.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, i64, C.c_int, C.c_int] + [vp] * 3 + [i64] + \
            [vp] * 8 + [i64, vp]
        L.sim_scene_cross_sort.restype = None
        L.sim_scene_cross_sort.argtypes = [vp] * 4 + [C.c_int32]
        _LIB = L
    return _LIB


def stack_capacity():
    return int(lib().sim_scene_cross_stack_capacity())


_ptr = cross_sim._ptr
offsets_of = cross_sim.offsets_of


def brute(members, mesh_of_instance, M, origins, directions, tmin=None, tmax=None, ray_base=0):
    """Result by testing every triangle of every instance: see the module docstring"""
    o, d, lo, hi = scene_sim._rays(origins, directions, tmin, tmax)
    n = len(o)
    mesh_of, M12 = scene_sim._instances(mesh_of_instance, M, len(members))
    valid, flip = scene_sim.record(M12)[1:] if len(mesh_of) else ([], [])
    with np.errstate(invalid="ignore"):
        world_ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    parts = dict(ray=[np.zeros(0, np.int64)], instance=[np.zeros(0, np.int32)], faces=[np.zeros(0, np.int32)], t=[np.zeros(0, np.float32)],
                 front=[np.zeros(0, bool)], loc=[np.zeros((0, 3), np.float32)], uv=[np.zeros((0, 2), np.float32)])
    for k in range(len(mesh_of)):
        v, f = members[mesh_of[k]]
        if not valid[k] or len(f) == 0:
            continue
        o2, d2, ok = scene_sim.transform(M12[k], o, d)
        r = cross_sim.brute(v, f, o2, d2, lo, hi)      # (a transformed ray that fails tr_ray_setup has no rows there either)
        keep = (ok & world_ok)[r.ray]
        parts["ray"].append(r.ray[keep])
        parts["instance"].append(np.full(int(keep.sum()), k, np.int32))
        parts["faces"].append(r.faces[keep])
        parts["t"].append(r.t[keep])
        parts["front"].append(r.front[keep] != flip[k])
        parts["loc"].append(scene_sim.points(M12[k], r.loc[keep]).reshape(-1, 3))
        parts["uv"].append(r.uv[keep])
    rows = {k: np.concatenate(x) for k, x in parts.items()}
    order = np.lexsort((rows["faces"], rows["instance"], rows["t"], rows["ray"]))
    rows = {k: x[order] for k, x in rows.items()}
    count = np.bincount(rows["ray"], minlength=n).astype(np.int32)
    return Result(count, offsets_of(count), rows["instance"], rows["faces"], rows["t"], rows["front"], rows["loc"], rows["uv"], rows["ray"] + ray_base)


def _rows(h):
    return dict(instance=np.full(h, -7, np.int32), faces=np.full(h, -7, np.int32), t=np.zeros(h, np.float32), front=np.zeros(h, np.uint8),
                loc=np.zeros((h, 3), np.float32), uv=np.zeros((h, 2), np.float32))


def walk(hierarchies, mesh_of_instance, M, origins, directions, tmin=None, tmax=None, stack_entries=0, order=None, want_lost=False,
         ray_base=0, count=None, total=None):
    """Result of the walk on the sim.SimBVH trees at `stack_entries`, instances visited in `order` (None: ascending): the count
    walk, then the fill and the rows function.  count / total (default: the count walk's own): what the fill is handed instead.
    want_lost: (Result, lost [n] bool of the count walk)"""
    arrays = [[np.ascontiguousarray(a) for a in (B.nodes, B.links, B.tris)] for B in hierarchies]
    nf = np.array([B.nf for B in hierarchies] + [0], np.int64)
    mesh_of, M12 = scene_sim._instances(mesh_of_instance, M, len(hierarchies))
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    assert order is None or sorted(order.tolist()) == list(range(len(mesh_of)))
    o, d, lo, hi = scene_sim._rays(origins, directions, tmin, tmax)
    n = len(o)
    L = lib()
    pn, pl, pt = (scene_sim._ptrs([a[j] for a in arrays]) for j in range(3))

    def run(mode, out, cnt=None, off=None, tot=0, rows=(None,) * 8, lost=None):
        L.sim_scene_cross_walk(pn, pl, pt, nf.ctypes.data, len(hierarchies), mesh_of.ctypes.data, M12.ctypes.data, len(mesh_of), _ptr(order),
                               o.ctypes.data, d.ctypes.data, _ptr(lo), _ptr(hi), n, int(stack_entries), mode, _ptr(out), _ptr(cnt), _ptr(off), tot,
                               *(_ptr(x) for x in rows), int(ray_base), _ptr(lost))
    own, lost = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    run(0, own, lost=lost)
    cnt = own if count is None else np.ascontiguousarray(count, np.int32)
    off = offsets_of(cnt)
    h = int(off[-1]) if total is None else int(total)
    r = _rows(h)
    slot, ray = np.full(h, -7, np.int32), np.full(h, -7, np.int64)
    run(1, None, cnt, off, h, (r["instance"], r["faces"], r["t"], slot, r["front"], r["loc"], r["uv"], ray))
    res = Result(own, off, r["instance"], r["faces"], r["t"], r["front"].astype(bool), r["loc"], r["uv"], ray)
    return (res, lost.astype(bool)) if want_lost else res


def sort(t, inst, face, slot=None):
    """tr_scene_cross_sort on copies of the rows -> (t, inst, face, slot)"""
    t, inst, face = np.array(t, np.float32), np.array(inst, np.int32), np.array(face, np.int32)
    slot = None if slot is None else np.array(slot, np.int32)
    lib().sim_scene_cross_sort(t.ctypes.data, inst.ctypes.data, face.ctypes.data, _ptr(slot), len(t))
    return t, inst, face, slot
