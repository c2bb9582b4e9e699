#!/usr/bin/env python3
"""ms per call of the configurations that take the stealing grid-node kernel family, and of a few that must not move
(count, location, streaming, the exact-node launch): three runs of 100 calls each (50 on the 5.2 M-triangle mesh), one
JSON line per config.  For an A/B run it once per side and alternate, the library chosen by TRIRO_HIP_LIBRARY:
    TRIRO_HIP_LIBRARY=<parent's libtriro_hip.so> python scripts/bench_steal_configs.py P >> out.jsonl
    python scripts/bench_steal_configs.py H >> out.jsonl        (profiles/r09_configs_ab.jsonl: P H P H)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import workloads as W  # noqa: E402
from triro.ray.ray_optix import RayMeshIntersector  # noqa: E402

dev = torch.device("cuda:0")
SIDE = sys.argv[1]


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def run(name, r, fn, reps=100, warm=40, runs=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / reps * 1e3, 4))
    try:
        li = r.as_wrapper.last_launch()
        li = {k: li[k] for k in ("query", "shape", "grid_nodes", "addressing")}
    except Exception:
        li = None
    print(json.dumps(dict(side=SIDE, config=name, ms=ms, launch=li)), flush=True)


v, f, _ = W.bunny_mesh()
r = RayMeshIntersector(vertices=T(v), faces=T(f))
o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
ot, dt = T(o), T(d)
run("C2 closest", r, lambda: r.intersects_closest(ot, dt))
n = 10_000_000
o3, d3 = W.hash_rays_torch(n, 1234, v.min(0) * 1.5, v.max(0) * 1.5, device=dev)
run("C3 any (streaming)", r, lambda: r.intersects_any(o3, d3), reps=10, warm=4)
del o3, d3
v, f = W.nested_shells(7)
r = RayMeshIntersector(vertices=T(v), faces=T(f))
o, d = W.pinhole_grid(1024, 1024)
ot, dt = T(o), T(d)
run("C4 closest", r, lambda: r.intersects_closest(ot, dt))
run("C4 any", r, lambda: r.intersects_any(ot, dt))
run("C4 first", r, lambda: r.intersects_first(ot, dt))
run("C4 count", r, lambda: r.intersects_count(ot, dt), reps=30, warm=12)
run("C4 location", r, lambda: r.intersects_location(ot, dt), reps=10, warm=4)
v, f = W.interior_room()
r = RayMeshIntersector(vertices=T(v), faces=T(f))
_, d = W.ref_shape_rays(W.INTERIOR_EYE, W.INTERIOR_TARGET)
ot = torch.from_numpy(np.array(W.INTERIOR_EYE, np.float32)).to(dev).expand(360, 640, 3)
dt = T(d)
run("ROOM closest", r, lambda: r.intersects_closest(ot, dt))
v, f = W.terrain()
r = RayMeshIntersector(vertices=T(v), faces=T(f))
_, d = W.ref_shape_rays(W.TERRAIN_EYE, W.TERRAIN_TARGET, 1024, 576, 444.0 * 1024 / 640)
ot = torch.from_numpy(np.array(W.TERRAIN_EYE, np.float32)).to(dev).expand(576, 1024, 3)
dt = T(d)
run("TERRAIN closest", r, lambda: r.intersects_closest(ot, dt))
v, f = W.headline_mesh(8)
r = RayMeshIntersector(vertices=T(v), faces=T(f))
o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
ot, dt = T(o), T(d)
run("headline closest", r, lambda: r.intersects_closest(ot, dt))
run("headline any", r, lambda: r.intersects_any(ot, dt))
run("headline first", r, lambda: r.intersects_first(ot, dt))
from launch_options import options  # noqa: E402
with options(grid_nodes=0):
    run("headline closest, exact nodes (grid_nodes=0)", r, lambda: r.intersects_closest(ot, dt))
run("headline count", r, lambda: r.intersects_count(ot, dt), reps=30, warm=12)
del r
v, f = W.headline_mesh(9)
r = RayMeshIntersector(vertices=T(v), faces=T(f))
o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
ot, dt = T(o), T(d)
run(f"5.2 M triangles (depth {r.bvh_info()['depth']}) closest", r, lambda: r.intersects_closest(ot, dt), reps=50, warm=20)
