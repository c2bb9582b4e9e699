#!/usr/bin/env python
"""Every crossing over an instanced scene (libtriro_scene_cross.so: tr_scene_cross_count, and the whole intersects_all)
against the only route there was before it: transform every copy's vertices, concatenate everything into one mesh, build it,
and ask cross_count_native / cross_all_native (libtriro_cross.so).

Workload: that of scripts/bench_scene.py -- N placed copies of the C2 stand-in (W.bunny_standin(): 81 920 triangles), N = 1,
8 and 64, on a jittered grid with a random rotation and a scale between 0.8 and 1.2 each, under 10 M incoherent hash rays with
origins in the world box, default bounds.

Per N, in ONE process: 3 warm-up launches and `--calls` timed ones of each route, each between two device events (median,
min, max); the baked route is run twice, before and after the scene: the spread between its two medians is the run-to-run
spread.  `count` is one launch; `all` is the whole query -- count, scan, one host read of the total, fill (two launches) --
with the allocation of its outputs.  Also kept: the rows of the lists and on how many rays the two routes count the same
(they differ by rounding: the baked vertices are float32 roundings of the placed ones).
The instance loop is linear in N and there is no top-level structure: nothing here promises a speed-up.
Nothing in the tests depends on these numbers.

Appends one JSON line per (N, route) to <out>/r11_scene_cross.jsonl and rewrites <out>/r11_scene_cross_summary.md (default:
profiles/)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--copies", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_cross.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_scene_cross_module()
    dev = torch.device("cuda", 0)
    v, f = W.bunny_standin()
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    extent = float((v.max(0) - v.min(0)).max())
    member = RayMeshIntersector(vertices=vt, faces=ft)
    os.makedirs(args.out, exist_ok=True)
    rows = []
    with open(os.path.join(args.out, "r11_scene_cross.jsonl"), "a") as fh:
        for N in args.copies:
            M = placements(N, extent, 90 + N)
            bv, bf = bake(vt, ft, M)
            lo, hi = bv.min(0).values.cpu().numpy(), bv.max(0).values.cpu().numpy()
            o, d = W.hash_rays_torch(args.rays, 83, lo, hi, device=dev)
            d = (d / d.norm(dim=1, keepdim=True).clamp_min(1e-20)).contiguous()
            n = o.shape[0]
            scene = RaySceneIntersector([member], np.zeros(N, np.int32), M)
            baked = RayMeshIntersector(vertices=bv, faces=bf)
            routes = dict(
                count=dict(baked=lambda: hops.cross_count_native(baked.as_wrapper, o, d),
                           scene=lambda: hops.scene_cross_count_native(scene._handle, dev.index, o, d)),
                all=dict(baked=lambda: hops.cross_all_native(baked.as_wrapper, o, d),
                         scene=lambda: hops.scene_cross_all_native(scene._handle, dev.index, o, d)))
            s_count, b_count = routes["count"]["scene"](), routes["count"]["baked"]()
            total, agree = int(s_count.sum()), int((s_count == b_count).sum())
            del s_count, b_count
            res = {}
            for query in ("count", "all"):
                for what, route in (("baked", "baked"), ("scene", "scene"), ("baked_again", "baked")):
                    ms = timed(routes[query][route], args.warmup, args.calls)
                    res[query, what] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
                    line = dict(copies=N, query=query, route=what, rays=n, tris_per_copy=int(ft.shape[0]), rows=total, same_count=agree,
                                warmup=args.warmup, calls=args.calls, device=torch.cuda.get_device_name(0), **res[query, what])
                    print(json.dumps(line), flush=True)
                    fh.write(json.dumps(line) + "\n")
                    torch.cuda.empty_cache()
            rows.append((N, n, total, agree, res))
            del scene, baked, bv, bf, o, d, routes
            torch.cuda.empty_cache()
    with open(os.path.join(args.out, "r11_scene_cross_summary.md"), "w") as fh:
        fh.write(f"# Every crossing over an instanced scene against the baked mesh ({args.rays} hash rays, N copies of the C2 stand-in, "
                 f"{int(ft.shape[0])} triangles each, default bounds, {torch.cuda.get_device_name(0)})\n\n")
        fh.write("Median ms of %d calls (min - max).  count = one launch (tr_scene_cross_count; baked: tr_cross_count).  all = the whole "
                 "query: count, scan, one host read of the total, fill (two launches), with the allocation of its outputs.  Baked = the N "
                 "copies transformed, concatenated and built as one mesh, run before and after the scene.\n\n" % args.calls)
        fh.write("| N | rows | count: baked | baked again | scene | scene / baked | all: baked | baked again | scene | scene / baked | same count |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        cell = lambda x: f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"      # noqa: E731
        for N, n, total, agree, res in rows:
            fh.write(f"| {N} | {total} | " + " | ".join(
                f"{cell(res[q, 'baked'])} | {cell(res[q, 'baked_again'])} | {cell(res[q, 'scene'])} | "
                f"{res[q, 'scene']['median_ms'] / res[q, 'baked']['median_ms']:.2f}x" for q in ("count", "all")) + f" | {agree / n:.4%} |\n")
        fh.write("\nEvery wave visits every instance (the cull of an instance is its root's two child boxes), so the scene launches grow "
                 "with N where the baked mesh's one hierarchy hardly does.  What the scene buys is one BVH for N copies and a move by a commit "
                 "of twelve floats (profiles/r09_scene_summary.md has those columns).\n")


if __name__ == "__main__":
    main()
