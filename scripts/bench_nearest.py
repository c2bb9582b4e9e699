#!/usr/bin/env python
"""closest_point (libtriro_nearest.so, one launch of k_closest_point) on the headline mesh (W.headline_mesh(): 1 310 720
triangles), and for scale the one launch of contains_points (tr_contains_points) on the same points.

Two point sets:
  hash    1 M hash points in 1.2x the mesh's box (incoherent: neighbouring lanes walk to different triangles)
  slice   the 1024 x 1024 points of a plane slice through the centre of the box, 1.2x its extent (coherent)

Per case: 5 warm-up launches, 20 timed ones, each between two device events; the figure is the median, min and max are
kept.  Nothing in the tests depends on these numbers: nobody had measured this walk before, there is no bar.

Appends one JSON line per case to <out>/nearest_bench.jsonl (default: profiles/)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import workloads as W  # noqa: E402
from triro.ray.ray_optix import RayMeshIntersector  # noqa: E402
import triro.backend.ops as hops  # noqa: E402


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivisions", type=int, default=8, help="of the headline icosphere (rehearsals: smaller)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nearest.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_nearest_module()
    hops.get_points_module()
    dev = torch.device("cuda", 0)
    v, f = W.headline_mesh(args.subdivisions)
    r = RayMeshIntersector(vertices=torch.from_numpy(v).to(dev), faces=torch.from_numpy(f).to(dev))
    lo, hi = v.min(0), v.max(0)
    centre, half = 0.5 * (lo + hi), 0.6 * (hi - lo)
    side = 1024
    xs = torch.linspace(float(centre[0] - half[0]), float(centre[0] + half[0]), side, device=dev)
    ys = torch.linspace(float(centre[1] - half[1]), float(centre[1] + half[1]), side, device=dev)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    sets = {
        "hash": W.hash_rays_torch(1 << 20, 77, centre - half, centre + half, device=dev)[0].contiguous(),
        "slice": torch.stack([gx, gy, torch.full_like(gx, float(centre[2]))], -1).reshape(-1, 3).contiguous(),
    }
    direction = torch.tensor(r._DEFAULT_DIRECTION, dtype=torch.float32, device=dev)
    box_lo, box_hi = r.mesh_aabb
    info = r.bvh_info()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "nearest_bench.jsonl"), "a") as fh:
        for name, pts in sets.items():
            closest, distance, tri = hops.closest_point_native(r.as_wrapper, pts)
            inside, _, _, _ = hops.contains_points_native(r.as_wrapper, pts, direction, box_lo, box_hi)
            torch.cuda.synchronize()
            facts = dict(points=int(pts.shape[0]), tris=int(info["num_tris"]), depth=int(info["depth"]),
                         mean_distance=float(distance.double().mean()), inside=int(inside.sum()),
                         distinct_triangles=int(torch.unique(tri).numel()))
            for what, fn in (("closest_point", lambda: hops.closest_point_native(r.as_wrapper, pts)),
                             ("contains_points", lambda: hops.contains_points_native(r.as_wrapper, pts, direction, box_lo, box_hi))):
                ms = timed(fn, args.warmup, args.calls)
                line = dict(case=name, query=what, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                            warmup=args.warmup, calls=args.calls, mpoints_per_s=pts.shape[0] / statistics.median(ms) / 1e3,
                            device=torch.cuda.get_device_name(0), **facts)
                print(json.dumps(line), flush=True)
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
