#!/usr/bin/env python
"""contains_points: the fused launch (libtriro_points.so) against the torch statements around intersects_count
(RayMeshIntersector._contains_points_torch, what every call ran before), in ONE process, alternating.

Configs (points are hash points in a region of the mesh's box whose points are all inside the mesh: the reference treats a
point with a ray that hits nothing as unresolved and retries it, so points outside a closed mesh would time the retry; the
summary {points in the box, unresolved points} of every config is reported):
  c2        the C2 stand-in mesh (81 920 triangles), 10 M points
  headline  the headline mesh (1 310 720 triangles), 10 M points
  room      interior_room (0.9 M triangles), 1 M points in the air above the furniture

Per config: 5 warm-up calls of each path, then REPS repetitions of the pair (native, torch); a repetition = CALLS calls,
each between two device events recorded around the whole Python call; the figure of a repetition is the median of its
calls.  Requirement: median over the repetitions of the native path <= that of the torch path + (max - min) of the torch
path's repetitions.  Peak memory: torch.cuda.max_memory_allocated over one call, above what was allocated before it.
Algorithmic bytes: 12 B in + 2 B out per point + one read of the grid nodes and the triangles.

Measured on an MI355X (profiles/r07_contains_summary.md): c2 2.877 ms native against 4.210 torch, room 0.754 against 0.871,
headline 5.189 against 5.132 with a torch spread of 0.005 -- the headline config MISSES the requirement by 1.1 % (the
baseline there is the streaming launch on the 8-wide nodes), so the script ends with an error on it.

Writes <out>/r07_contains.jsonl (one line per repetition and path) and <out>/r07_contains_summary.md (the table; whatever
follows the marker line in an existing file is kept)."""
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

MARKER = "<!-- what follows is kept when scripts/bench_contains.py rewrites the table -->"


def configs(scale):
    def c2():
        v, f = W.bunny_standin()
        return v, f, [-0.45] * 3, [0.45] * 3, int(10_000_000 * scale)

    def headline():
        v, f = W.headline_mesh(8)
        return v, f, [-0.45] * 3, [0.45] * 3, int(10_000_000 * scale)

    def room():
        v, f = W.interior_room()
        # (above the furniture, and where neither ray of a point passes the seam between the floor's height field and a wall)
        return v, f, [-1.5, 2.5, 0.5], [3.3, 2.9, 2.4], int(1_000_000 * scale)
    return {"c2": c2, "headline": headline, "room": room}


def timed_calls(fn, calls):
    """milliseconds of each call: device events around the whole Python call"""
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def peak_bytes(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,headline,room")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the point counts (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contains.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_points_module()
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    rows, lines = [], []
    for name in args.configs.split(","):
        v, f, lo, hi, n = configs(args.scale)[name]()
        r = RayMeshIntersector(vertices=torch.from_numpy(v).to(dev), faces=torch.from_numpy(f).to(dev))
        pts = W.hash_rays_torch(n, 77, lo, hi, device=dev)[0].contiguous()
        info = r.bvh_info()
        tree = info["num_nodes"] * 32 + info["tri_bytes"]
        lo_t, hi_t = r.mesh_aabb
        _, _, _, summary = hops.contains_points_native(r.as_wrapper, pts, torch.tensor(r._DEFAULT_DIRECTION, device=dev), lo_t, hi_t)
        in_box, unresolved = summary.tolist()
        if unresolved != 0 or in_box != n:      # a retry (or an early return) would be timed: the region is wrong for this mesh
            raise SystemExit(f"{name}: {unresolved} unresolved points, {in_box} of {n} in the box -- no retry may be triggered")

        def native():
            assert r.native_contains
            return r.contains_points(pts)

        def baseline():
            return r._contains_points_torch(pts)
        got_n, got_t = native(), baseline()
        same = bool(torch.equal(got_n, got_t))
        inside = int(got_n.sum())
        del got_n, got_t
        for _ in range(args.warmup):
            native()
            baseline()
        torch.cuda.synchronize()
        med = {"native": [], "torch": []}
        for rep in range(args.reps):
            for path, fn in (("native", native), ("torch", baseline)):
                ms = timed_calls(fn, args.calls)
                med[path].append(statistics.median(ms))
                lines.append(dict(config=name, path=path, rep=rep, points=n, tris=info["num_tris"], calls=args.calls,
                                  median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms)))
        peak = {"native": peak_bytes(native), "torch": peak_bytes(baseline)}
        mn, mt = statistics.median(med["native"]), statistics.median(med["torch"])
        spread = max(med["torch"]) - min(med["torch"])
        algo = 14 * n + tree
        rows.append(dict(config=name, points=n, tris=info["num_tris"], native_ms=mn, torch_ms=mt, torch_spread_ms=spread,
                         native_spread_ms=max(med["native"]) - min(med["native"]), met=mn <= mt + spread, speedup=mt / mn,
                         peak_native=peak["native"], peak_torch=peak["torch"], algo_bytes=algo, algo_gbs=algo / (mn * 1e-3) / 1e9,
                         in_box=in_box, unresolved=unresolved, inside=inside, same=same,
                         addressing=hops.contains_addressing(r.as_wrapper)))
        print(json.dumps(rows[-1]), flush=True)
        del r, pts
        torch.cuda.empty_cache()
    with open(os.path.join(args.out, "r07_contains.jsonl"), "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")
    path = os.path.join(args.out, "r07_contains_summary.md")
    kept = ""
    if os.path.exists(path):
        old = open(path).read()
        if MARKER in old:
            kept = old[old.index(MARKER) + len(MARKER):]
    with open(path, "w") as fh:
        fh.write("# contains_points: the fused launch against the torch statements around intersects_count\n\n")
        fh.write(f"`scripts/bench_contains.py`: {args.warmup} warm-up calls, {args.reps} repetitions of the pair, {args.calls} calls per "
                 "repetition, device events around the whole Python call; a repetition's figure is the median of its calls, a path's "
                 "figure the median of its repetitions, spread = max - min over the repetitions.  Every repetition: "
                 "`r07_contains.jsonl`.\n\n")
        fh.write("| config | points | triangles | native ms | torch ms | torch spread ms | native <= torch + spread | torch / native | "
                 "peak MiB native | peak MiB torch | algorithmic MB | algorithmic GB/s (native) | in box | unresolved | inside | same result |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for x in rows:
            fh.write(f"| {x['config']} | {x['points']} | {x['tris']} | {x['native_ms']:.3f} | {x['torch_ms']:.3f} | {x['torch_spread_ms']:.3f} | "
                     f"{'yes' if x['met'] else 'NO'} | {x['speedup']:.2f} | {x['peak_native'] / 2**20:.1f} | {x['peak_torch'] / 2**20:.1f} | "
                     f"{x['algo_bytes'] / 1e6:.1f} | {x['algo_gbs']:.1f} | {x['in_box']} | {x['unresolved']} | {x['inside']} | "
                     f"{'yes' if x['same'] else 'NO'} |\n")
        fh.write("\n" + MARKER + kept)
    if not all(x["met"] and x["same"] for x in rows):
        raise SystemExit("a config misses the requirement (see the table)")


if __name__ == "__main__":
    main()
