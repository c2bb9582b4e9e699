#!/usr/bin/env python
"""closest_point on an instanced scene (libtriro_scene_nearest.so: tr_scene_closest_point) against the only route there was
before it: bake every placed copy into one mesh, build it, and run tr_closest_point on that.

Workload: that of scripts/bench_scene.py -- N placed copies of the C2 stand-in (W.bunny_standin(): 81 920 triangles), N = 1, 8
and 64, on a jittered grid with a random rotation and a scale between 0.8 and 1.2 each -- under hash points in the scene's
world box.

Per N, in ONE process: the two routes' answers are compared first (the baked route here transforms with torch, not with the
scene's fmaf chain, so the comparison is a rate of equal (instance, triangle), not bit for bit: tests/test_gpu_scene_nearest.py
has the bit-for-bit identity), then `--warmup` warm-up and `--calls` timed launches of each route, each between two device
events (median, min, max); the baked route is run twice, before and after the scene launch: the spread between its two medians
is the run-to-run spread.  Also: the wall time to move one copy by each route (scene: a commit of the table; baked: transform,
concatenate, rebuild) and the device memory of the acceleration structures (scene: one member arena and the scene's table).
The instance loop is linear in N and there is no top-level structure: nothing here promises a faster query than a baked mesh.
Nothing in the tests depends on these numbers.

Appends one JSON line per (N, route) to <out>/scene_nearest.jsonl and rewrites <out>/scene_nearest_summary.md (default: profiles/)."""
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
from bench_scene import bake, peak_mib, placements, timed, wall_ms  # noqa: E402
from triro.ray import RaySceneIntersector  # noqa: E402
from triro.ray.ray_optix import RayMeshIntersector  # noqa: E402
import triro.backend.ops as hops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--copies", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_nearest.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_scene_nearest_module()
    dev = torch.device("cuda", 0)
    v, f = W.bunny_standin()
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    extent = float((v.max(0) - v.min(0)).max())
    member = RayMeshIntersector(vertices=vt, faces=ft)
    os.makedirs(args.out, exist_ok=True)
    rows = []
    with open(os.path.join(args.out, "scene_nearest.jsonl"), "a") as fh:
        for N in args.copies:
            M = placements(N, extent, 90 + N)
            bv, bf = bake(vt, ft, M)
            lo, hi = bv.min(0).values.cpu().numpy(), bv.max(0).values.cpu().numpy()
            p = W.hash_rays_torch(args.points, 83, lo, hi, device=dev)[0].contiguous()
            n = p.shape[0]
            scene = RaySceneIntersector([member], np.zeros(N, np.int32), M)
            baked = RayMeshIntersector(vertices=bv, faces=bf)
            scene_mib = (member.bvh_info()["arena_bytes"] + scene.info()["table_bytes"]) / 2 ** 20
            baked_mib = baked.bvh_info()["arena_bytes"] / 2 ** 20

            def run_scene():
                return hops.scene_closest_point_native(scene._handle, dev.index, p)

            def run_baked():
                return hops.closest_point_native(baked.as_wrapper, p)

            _, s_d, s_inst, s_tri = run_scene()
            _, b_d, b_tri = run_baked()
            agree = int((s_inst.to(torch.int64) * ft.shape[0] + s_tri == b_tri).sum())
            mean_d, worst = float(s_d.double().mean()), float((s_d - b_d).abs().max())
            del s_d, s_inst, s_tri, b_d, b_tri
            M2 = M.copy()
            M2[N - 1, :, 3] += np.float32(0.05 * extent)

            def move_scene():
                scene.set_transforms(M2)

            def move_baked():
                baked.update_raw(*bake(vt, ft, M2))

            move = dict(scene_ms=wall_ms(move_scene), baked_ms=wall_ms(move_baked))
            scene.set_transforms(M)
            baked.update_raw(bv, bf)
            res = {}
            for what, fn in (("baked", run_baked), ("scene", run_scene), ("baked_again", run_baked)):
                ms = timed(fn, args.warmup, args.calls)
                res[what] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), peak_mib=peak_mib(fn))
                line = dict(copies=N, route=what, points=n, tris_per_copy=int(ft.shape[0]), same_triangle=agree, mean_distance=mean_d,
                            largest_distance_difference=worst, owned_mib=baked_mib if what.startswith("baked") else scene_mib,
                            move_one_copy_ms=move["baked_ms"] if what.startswith("baked") else move["scene_ms"], warmup=args.warmup,
                            calls=args.calls, device=torch.cuda.get_device_name(0), **res[what])
                print(json.dumps(line), flush=True)
                fh.write(json.dumps(line) + "\n")
            rows.append((N, n, agree, scene_mib, baked_mib, move, res))
            del scene, baked, bv, bf, p
            torch.cuda.empty_cache()
    with open(os.path.join(args.out, "scene_nearest_summary.md"), "w") as fh:
        fh.write(f"# closest_point on an instanced scene against the baked mesh ({args.points} hash points in the world box, N copies of the C2 "
                 f"stand-in, {int(ft.shape[0])} triangles each, {torch.cuda.get_device_name(0)})\n\n")
        fh.write("Median ms of %d launches (min - max) after %d warm-up launches.  Baked = tr_closest_point on the N copies transformed, "
                 "concatenated and built as one mesh, run before and after the scene launch.  Scene = tr_scene_closest_point, unbounded.  "
                 "Owned MiB = device memory of the acceleration structures (scene: one member arena + the scene table).  Move = wall ms to "
                 "move one copy (scene: a commit; baked: transform, concatenate, rebuild).  Same triangle = points on which both routes name "
                 "the same (instance, triangle); the baked route of this script transforms with torch, not with the scene's chain, so near-ties "
                 "may fall the other way.\n\n" % (args.calls, args.warmup))
        fh.write("| N | baked | baked again | scene (tr_scene_closest_point) | scene / baked | owned MiB scene / baked | peak MiB of a call scene / baked | move ms scene / baked | same triangle |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|\n")
        cell = lambda x: f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"      # noqa: E731
        for N, n, agree, scene_mib, baked_mib, move, res in rows:
            fh.write(f"| {N} | {cell(res['baked'])} | {cell(res['baked_again'])} | {cell(res['scene'])} | "
                     f"{res['scene']['median_ms'] / res['baked']['median_ms']:.2f}x | {scene_mib:.1f} / {baked_mib:.1f} | "
                     f"{res['scene']['peak_mib']:.0f} / {res['baked']['peak_mib']:.0f} | {move['scene_ms']:.3f} / {move['baked_ms']:.3f} | {agree / n:.4%} |\n")
        fh.write("\nEvery wave visits every instance (the cull of an instance is the placed boxes of its root's children against the best so "
                 "far), and every box and triangle it meets is placed into world space first, so the scene launch grows with N where the baked "
                 "mesh's one hierarchy hardly does.  What the scene buys is the memory column and the move column.  NOT MEASURED: bounded "
                 "max_distance, other point distributions, counters.\n")


if __name__ == "__main__":
    main()
