#!/usr/bin/env python
"""Triangle queries on an instanced scene (libtriro_scene_tris.so: tr_scene_tris_count / tr_scene_tris_fill) beside the only
route there was before them: bake every placed copy into one mesh, build it, and run tr_tris_count / tr_tris_fill on that.

Workload: N = 64 placed copies of the C2 stand-in (W.bunny_standin(): 81 920 triangles) on the jittered grid of
scripts/bench_scene.py, and a MOVING MESH -- a displaced icosphere(5), 20 480 faces, about one member's size -- at `--poses`
positions across the scene: its faces at every pose are the query triangles of one launch (poses x 20 480 queries).

In ONE process: the two routes' counts are compared first (the baked route here transforms with torch, not with the scene's
fmaf chain, so the comparison is a rate of equal counts, not bit for bit: tests/test_gpu_scene_tris.py has the identity on the
chain's own baking), then `--warmup` warm-up and `--calls` timed calls of each route and query, each between two device events
(median, min, max).  The baked route is the YARDSTICK, not the code under test; it is run before and after the scene's calls:
the spread between its two medians is the run-to-run spread.  count = one launch; fill = the walk and the ordering on counts
and offsets computed beforehand.  Also: the wall time to move one copy by each route and the device memory of the acceleration
structures.  The instance loop is linear in N and there is no top-level structure: nothing here promises a faster query than a
baked mesh, and the ratio is reported as measured.  Nothing in the tests depends on these numbers.

Appends one JSON line per (query, route) to <out>/scene_tris.jsonl (default: profiles/) and prints a table."""
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
from bench_scene import bake, placements, timed, wall_ms  # noqa: E402
from triro.ray import RaySceneIntersector  # noqa: E402
from triro.ray.ray_optix import RayMeshIntersector  # noqa: E402
import triro.backend.ops as hops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_tris.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_scene_tris_module()
    dev = torch.device("cuda", 0)
    v, f = W.bunny_standin()
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    extent = float((v.max(0) - v.min(0)).max())
    N = args.copies
    M = placements(N, extent, 90 + N)
    member = RayMeshIntersector(vertices=vt, faces=ft)
    scene = RaySceneIntersector([member], np.zeros(N, np.int32), M)
    bv, bf = bake(vt, ft, M)
    baked = RayMeshIntersector(vertices=bv, faces=bf)
    # the moving mesh at `poses` positions on a line through the scene's world box
    ov, of = W.icosphere(5)
    ov = W.displaced(ov, seed=3, amplitude=0.05)
    ov = (ov * np.float32(0.5 * extent / float((ov.max(0) - ov.min(0)).max()))).astype(np.float32)
    lo, hi = bv.min(0).values.cpu().numpy(), bv.max(0).values.cpu().numpy()
    steps = np.linspace(0.1, 0.9, args.poses)[:, None]
    centres = (lo + steps * (hi - lo)).astype(np.float32)
    tri = torch.from_numpy(np.concatenate([(ov + c)[of] for c in centres]).astype(np.float32)).to(dev).contiguous()
    n = tri.shape[0]
    h, di = scene._handle, dev.index
    # the two routes answer alike (up to the baking by torch), and what the fills will be given
    s_count = hops.scene_tris_native(h, di, tri, "count")
    b_count = hops.tris_native(baked.as_wrapper, tri, "count")
    same = int((s_count == b_count).sum())
    s_off, s_total = hops._scan_counts(s_count)
    b_off, b_total = hops._scan_counts(b_count)
    s_off, b_off = s_off[:-1].contiguous(), b_off[:-1].contiguous()
    meeting = int((s_count > 0).sum())
    M2 = M.copy()
    M2[N - 1, :, 3] += np.float32(0.05 * extent)
    move_scene = wall_ms(lambda: scene.set_transforms(M2))
    move_baked = wall_ms(lambda: baked.update_raw(*bake(vt, ft, M2)))
    scene.set_transforms(M)
    baked.update_raw(bv, bf)
    scene_mib = (member.bvh_info()["arena_bytes"] + scene.info()["table_bytes"]) / 2 ** 20
    baked_mib = baked.bvh_info()["arena_bytes"] / 2 ** 20
    runs = {
        ("count", "baked"): lambda: hops.tris_native(baked.as_wrapper, tri, "count"),
        ("count", "scene"): lambda: hops.scene_tris_native(h, di, tri, "count"),
        ("fill", "baked"): lambda: hops.tris_fill_native(baked.as_wrapper, tri, b_count, b_off, b_total),
        ("fill", "scene"): lambda: hops.scene_tris_fill_native(h, di, tri, s_count, s_off, s_total),
    }
    os.makedirs(args.out, exist_ok=True)
    res = {}
    with open(os.path.join(args.out, "scene_tris.jsonl"), "a") as fh:
        for query in ("count", "fill"):
            for route, key in (("baked", "baked"), ("scene", "scene"), ("baked_again", "baked")):
                ms = timed(runs[(query, key)], args.warmup, args.calls)
                res[(query, route)] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
                line = dict(query=query, route=route, copies=N, tris_per_copy=int(ft.shape[0]), queries=n, poses=args.poses,
                            queries_that_meet=meeting, rows=s_total if key == "scene" else b_total, same_count=same,
                            owned_mib=baked_mib if key == "baked" else scene_mib, move_one_copy_ms=move_baked if key == "baked" else move_scene,
                            warmup=args.warmup, calls=args.calls, device=torch.cuda.get_device_name(0), **res[(query, route)])
                print(json.dumps(line), flush=True)
                fh.write(json.dumps(line) + "\n")
    cell = lambda x: f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"      # noqa: E731
    print(f"\n{n} query triangles ({args.poses} poses x {len(of)} faces) against {N} copies of {int(ft.shape[0])} triangles; "
          f"{meeting} queries meet something, {s_total} rows; equal counts on {same / n:.4%} of the queries")
    print("| query | baked | baked again | scene | scene / baked |\n|---|---|---|---|---|")
    for query in ("count", "fill"):
        b, s, a = res[(query, "baked")], res[(query, "scene")], res[(query, "baked_again")]
        print(f"| {query} | {cell(b)} | {cell(a)} | {cell(s)} | {s['median_ms'] / b['median_ms']:.2f}x |")
    print(f"owned MiB scene / baked: {scene_mib:.1f} / {baked_mib:.1f}; move one copy, ms, scene / baked: {move_scene:.3f} / {move_baked:.3f}")


if __name__ == "__main__":
    main()
