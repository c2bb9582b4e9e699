#!/usr/bin/env python
"""Instanced scenes (libtriro_scene.so: tr_scene_closest) against the only route there was before them: transform every
copy's vertices, concatenate everything into one mesh, build it, and ask intersects_closest_range.

Workload: N placed copies of the C2 stand-in (W.bunny_standin(): 81 920 triangles), N = 1, 8 and 64, on a jittered grid with
a random rotation and a scale between 0.8 and 1.2 each, under 10 M incoherent hash rays with origins in the world box.

Per N, in ONE process: 3 warm-up launches and `--calls` timed ones of the scene launch and of the range launch on the baked
mesh, each between two device events (median, min, max); the baked route is run twice, before and after the scene: the
spread between its two medians is the run-to-run spread.  Also kept: the device memory both own (the members' arenas plus
the scene's table against the baked mesh's arena), peak memory of one query call of each, the wall time of moving ONE copy
(set_transforms: a commit, against transforming + concatenating + update_raw of the baked mesh), and on how many rays the two
routes name the same triangle (they differ by rounding: the baked vertices are float32 roundings of the placed ones).
The instance loop is linear in N and there is no top-level structure: nothing here promises a speed-up.
Nothing in the tests depends on these numbers.

Appends one JSON line per (N, route) to <out>/r09_scene.jsonl and rewrites <out>/r09_scene_summary.md (default: profiles/)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import workloads as W  # noqa: E402
from triro.ray import RaySceneIntersector  # noqa: E402
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


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def wall_ms(fn, repeats=3):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def placements(n, extent, seed):
    """[n, 3, 4] float32: a jittered grid of side ceil(cbrt(n)), 1.4 extents apart, a random rotation and scale each"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3) - 1e-9))
    out = np.zeros((n, 3, 4), np.float32)
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cell = np.array([k % side, (k // side) % side, k // (side * side)], np.float64)
        out[k, :, :3] = q * rng.uniform(0.8, 1.2)
        out[k, :, 3] = (cell + rng.uniform(-0.15, 0.15, 3)) * 1.4 * extent
    return out


def bake(v, f, M):
    """the parent commit's way: every copy's vertices transformed (float32, on the GPU) and everything concatenated"""
    Mt = torch.from_numpy(M).to(v.device)
    vs = torch.einsum("nij,vj->nvi", Mt[:, :, :3], v) + Mt[:, None, :, 3]
    fs = f[None, :, :] + (torch.arange(len(M), device=v.device, dtype=torch.int32) * v.shape[0])[:, None, None]
    return vs.reshape(-1, 3).contiguous(), fs.reshape(-1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--copies", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_scene_module()
    dev = torch.device("cuda", 0)
    v, f = W.bunny_standin()
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    extent = float((v.max(0) - v.min(0)).max())
    member = RayMeshIntersector(vertices=vt, faces=ft)
    os.makedirs(args.out, exist_ok=True)
    rows = []
    with open(os.path.join(args.out, "r09_scene.jsonl"), "a") as fh:
        for N in args.copies:
            M = placements(N, extent, 90 + N)
            bv, bf = bake(vt, ft, M)
            lo, hi = bv.min(0).values.cpu().numpy(), bv.max(0).values.cpu().numpy()
            o, d = W.hash_rays_torch(args.rays, 83, lo, hi, device=dev)
            d = (d / d.norm(dim=1, keepdim=True).clamp_min(1e-20)).contiguous()
            n = o.shape[0]
            scene = RaySceneIntersector([member], np.zeros(N, np.int32), M)
            baked = RayMeshIntersector(vertices=bv, faces=bf)
            scene_mib = (member.bvh_info()["arena_bytes"] + scene.info()["table_bytes"]) / 2 ** 20
            baked_mib = baked.bvh_info()["arena_bytes"] / 2 ** 20

            def run_scene():
                return hops.scene_closest_native(scene._handle, dev.index, o, d)

            def run_baked():
                return hops.range_closest_native(baked.as_wrapper, o, d)

            s_hit, _, s_inst, s_tri, _, _, _ = run_scene()
            b_hit, _, b_tri, _, _, _ = run_baked()
            same = (s_hit == b_hit) & (~s_hit | (s_inst.to(torch.int64) * ft.shape[0] + s_tri == b_tri))
            hits, agree = int(s_hit.sum()), int(same.sum())
            del s_hit, s_inst, s_tri, b_hit, b_tri, same
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
                line = dict(copies=N, route=what, rays=n, tris_per_copy=int(ft.shape[0]), hits=hits, same_triangle=agree,
                            owned_mib=baked_mib if what.startswith("baked") else scene_mib,
                            move_one_copy_ms=move["baked_ms"] if what.startswith("baked") else move["scene_ms"], warmup=args.warmup,
                            calls=args.calls, device=torch.cuda.get_device_name(0), **res[what])
                print(json.dumps(line), flush=True)
                fh.write(json.dumps(line) + "\n")
            rows.append((N, n, hits, agree, scene_mib, baked_mib, move, res))
            del scene, baked, bv, bf, o, d
            torch.cuda.empty_cache()
    with open(os.path.join(args.out, "r09_scene_summary.md"), "w") as fh:
        fh.write(f"# Instanced scene against the baked mesh ({args.rays} hash rays, N copies of the C2 stand-in, {int(ft.shape[0])} triangles each, "
                 f"{torch.cuda.get_device_name(0)})\n\n")
        fh.write("Median ms of %d launches (min - max).  Baked = tr_range_closest on the N copies transformed, concatenated and built "
                 "as one mesh, run before and after the scene launch.  Owned MiB = device memory of the acceleration structures "
                 "(scene: one member arena + the scene table).  Move = wall ms to move one copy (scene: a commit; baked: transform, "
                 "concatenate, rebuild).\n\n" % args.calls)
        fh.write("| N | hit | baked | baked again | scene (tr_scene_closest) | scene / baked | owned MiB scene / baked | peak MiB of a call scene / baked | move ms scene / baked | same triangle |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|\n")
        cell = lambda x: f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"      # noqa: E731
        for N, n, hits, agree, scene_mib, baked_mib, move, res in rows:
            fh.write(f"| {N} | {hits / n:.1%} | {cell(res['baked'])} | {cell(res['baked_again'])} | {cell(res['scene'])} | "
                     f"{res['scene']['median_ms'] / res['baked']['median_ms']:.2f}x | {scene_mib:.1f} / {baked_mib:.1f} | "
                     f"{res['scene']['peak_mib']:.0f} / {res['baked']['peak_mib']:.0f} | {move['scene_ms']:.3f} / {move['baked_ms']:.3f} | {agree / n:.4%} |\n")
        fh.write("\nEvery wave visits every instance (the cull of an instance is its root's two child boxes), so the scene launch grows with N "
                 "where the baked mesh's one hierarchy hardly does.  What the scene buys is the memory column and the move column.\n")


if __name__ == "__main__":
    main()
