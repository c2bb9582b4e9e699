#!/usr/bin/env python
"""contains_points on an instanced scene (libtriro_scene_points.so: tr_scene_points_count, and the whole containing_instances)
against the route the scene offered before it: two intersects_all calls on (p, d) and (p, -d) -- each a count, a scan, a host
read, a fill and a per-ray ordering of rows (libtriro_scene_cross.so) -- and a torch reduction over (point, instance) that keeps
the pairs with an odd number of rows both ways.

Workload: that of scripts/bench_scene_cross.py -- N placed copies of the C2 stand-in (W.bunny_standin(): 81 920 triangles), N =
1, 8 and 64, on a jittered grid with a random rotation and a scale between 0.8 and 1.2 each -- under hash points in the scene's
world box, along the reference's default direction.

Per N, in ONE process: the two routes' answers are compared first (count and list must be equal: both are exact in the same
predicate), then 3 warm-up and `--calls` timed calls of each route, each between two device events (median, min, max); the
composed route is run twice, before and after the native one: the spread between its two medians is the run-to-run spread.
`count` is one launch; `list` is the whole query -- count, scan, one host read of the total, fill -- with the allocation of its
outputs.  For N = 1 the member's own contains_points launch (libtriro_points.so, through its binding) is also timed: on the
same points taken into the member's frame, beside tr_scene_points_any on a scene that holds the member at the identity.
The instance loop is linear in N and there is no top-level structure: nothing here promises a speed-up over a baked mesh.
Nothing in the tests depends on these numbers.

Appends one JSON line per (N, query, route) to <out>/r14_scene_points.jsonl and rewrites <out>/r14_scene_points_summary.md
(default: profiles/)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)
import workloads as W  # noqa: E402
from bench_scene import bake, placements, timed  # noqa: E402
from triro.ray import RaySceneIntersector  # noqa: E402
from triro.ray.ray_optix import RayMeshIntersector  # noqa: E402
import triro.backend.ops as hops  # noqa: E402


def composed(scene, dev, p, d, ninst):
    """(count int32[n], offsets int64[n + 1], instance int32[h]) by the route of the parent commit"""
    n = p.shape[0]
    odd = []
    for sign in (1.0, -1.0):
        dirs = (sign * d).expand(n, 3).contiguous()
        offsets, inst = hops.scene_cross_all_native(scene._handle, dev.index, p, dirs)[:2]
        ray = torch.repeat_interleave(torch.arange(n, device=p.device), offsets[1:] - offsets[:-1])
        keys, rows = torch.unique(ray * ninst + inst.long(), return_counts=True)      # (sorted: by point, then instance)
        odd.append(keys[rows % 2 == 1])
    both = odd[0][torch.isin(odd[0], odd[1], assume_unique=True)]
    count = torch.bincount(both // ninst, minlength=n).int()
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=p.device)
    offsets[1:] = torch.cumsum(count, 0)
    return count, offsets, (both % ninst).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--copies", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_points.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_scene_points_module()
    dev = torch.device("cuda", 0)
    v, f = W.bunny_standin()
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    extent = float((v.max(0) - v.min(0)).max())
    member = RayMeshIntersector(vertices=vt, faces=ft)
    d = torch.tensor(RayMeshIntersector._DEFAULT_DIRECTION, dtype=torch.float32, device=dev)
    os.makedirs(args.out, exist_ok=True)
    table = []
    with open(os.path.join(args.out, "r14_scene_points.jsonl"), "a") as fh:
        for N in args.copies:
            M = placements(N, extent, 90 + N)
            bv, _ = bake(vt, ft, M)
            lo, hi = bv.min(0).values.cpu().numpy(), bv.max(0).values.cpu().numpy()
            del bv
            p = W.hash_rays_torch(args.points, 83, lo, hi, device=dev)[0].contiguous()
            n = p.shape[0]
            scene = RaySceneIntersector([member], np.zeros(N, np.int32), M)
            h = scene._handle
            routes = dict(
                count=dict(composed=lambda: composed(scene, dev, p, d, N)[0], native=lambda: hops.scene_points_count_native(h, dev.index, p, d)),
                list=dict(composed=lambda: composed(scene, dev, p, d, N)[1:], native=lambda: hops.scene_points_list_native(h, dev.index, p, d)))
            # the two answers first
            c_count, c_offsets, c_inst = composed(scene, dev, p, d, N)
            n_count = routes["count"]["native"]()
            n_offsets, n_inst = routes["list"]["native"]()
            same = bool(torch.equal(c_count, n_count) and torch.equal(c_offsets, n_offsets) and torch.equal(c_inst, n_inst))
            inside, rows = int((n_count > 0).sum()), int(n_offsets[-1])
            if not same:
                raise SystemExit(f"N = {N}: the composed route and the native one disagree on {int((c_count != n_count).sum())} points")
            del c_count, c_offsets, c_inst, n_count, n_offsets, n_inst
            order = [("count", "composed", "composed"), ("count", "native", "native"), ("count", "composed_again", "composed"),
                     ("list", "composed", "composed"), ("list", "native", "native"), ("list", "composed_again", "composed")]
            if N == 1:      # the member's own launch: the points in the member's frame (the identity scene is timed beside it)
                Mi = np.linalg.inv(np.concatenate([M[0].astype(np.float64), [[0, 0, 0, 1]]]))
                q = (p.double() @ torch.from_numpy(Mi[:3, :3].T).to(dev) + torch.from_numpy(Mi[:3, 3]).to(dev)).float().contiguous()
                di = (torch.from_numpy(Mi[:3, :3]).to(dev) @ d.double()).float().contiguous()
                ident = RaySceneIntersector([member], np.zeros(1, np.int32), np.eye(3, 4, dtype=np.float32)[None])
                blo, bhi = (t.reshape(3) for t in member.mesh_aabb)
                routes["any"] = dict(mesh=lambda: hops.contains_points_native(member.as_wrapper, q, di, blo, bhi)[0],
                                     native=lambda: hops.scene_points_any_native(ident._handle, dev.index, q, di))
                agree = int((routes["any"]["mesh"]() == routes["any"]["native"]()).sum())
                order += [("any", "mesh", "mesh"), ("any", "native", "native")]
            res = {}
            for query, what, route in order:
                ms = timed(routes[query][route], args.warmup, args.calls)
                res[query, what] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
                line = dict(copies=N, query=query, route=what, points=n, tris_per_copy=int(ft.shape[0]), inside=inside, rows=rows,
                            same_answer=same, warmup=args.warmup, calls=args.calls, device=torch.cuda.get_device_name(0), **res[query, what])
                if query == "any":
                    line["same_as_mesh"] = agree
                print(json.dumps(line), flush=True)
                fh.write(json.dumps(line) + "\n")
                torch.cuda.empty_cache()
            table.append((N, n, inside, rows, res))
            del scene, p, routes
            torch.cuda.empty_cache()
    cell = lambda x: f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"      # noqa: E731
    with open(os.path.join(args.out, "r14_scene_points_summary.md"), "w") as fh:
        fh.write(f"# contains_points on an instanced scene against two intersects_all calls and a torch reduction ({args.points} hash points, "
                 f"N copies of the C2 stand-in, {int(ft.shape[0])} triangles each, the default direction, {torch.cuda.get_device_name(0)})\n\n")
        fh.write("Median ms of %d calls (min - max).  count = one launch (tr_scene_points_count).  list = the whole query: count, scan, one host "
                 "read of the total, fill, with the allocation of its outputs.  Composed = intersects_all on (p, d) and on (p, -d), then the "
                 "(point, instance) pairs with an odd number of rows both ways, in torch; run before and after the native route.  The two "
                 "routes gave the same count, offsets and list on every point before anything was timed.\n\n" % args.calls)
        fh.write("| N | points inside | rows | count: composed | composed again | native | composed / native | list: composed | composed again | native | composed / native |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for N, n, inside, rows, res in table:
            fh.write(f"| {N} | {inside} | {rows} | " + " | ".join(
                f"{cell(res[q, 'composed'])} | {cell(res[q, 'composed_again'])} | {cell(res[q, 'native'])} | "
                f"{res[q, 'composed']['median_ms'] / res[q, 'native']['median_ms']:.1f}x" for q in ("count", "list")) + " |\n")
        for N, n, inside, rows, res in table:
            if ("any", "mesh") in res:
                fh.write(f"\nN = 1, the same points in the member's frame: the member's own contains_points launch (libtriro_points.so, grid nodes, "
                         f"the unordered schedule) {cell(res['any', 'mesh'])} ms, tr_scene_points_any on the identity scene "
                         f"{cell(res['any', 'native'])} ms.\n")
        fh.write("\nEvery wave visits every instance (the cull of an instance is its root's two child boxes), so the launches grow with N.  "
                 "NOT MEASURED: a baked mesh of all copies under the mesh's contains_points (it answers another question: which copy holds "
                 "the point is lost), other directions, other point distributions, counters.\n")


if __name__ == "__main__":
    main()
