#!/usr/bin/env python
"""Range queries (libtriro_range.so: tr_range_any, tr_range_closest) against the only route there was for tmin = 0 before
them: intersects_closest on the whole ray plus the torch comparison of |loc - o| with tmax * |d|.

Mesh: the C2 stand-in (W.bunny_standin(): 81 920 triangles).  Rays: 10 M incoherent hash rays with origins in the mesh's
box and normalised directions, so that tmax is a length.  Segment lengths: 1/64, 1/8 and 1 x the mesh extent, and unbounded
(tmax = None for the range entries; the baseline then is intersects_closest alone).

Per length, in ONE process: 3 warm-up launches and `--calls` timed ones of each of the three routes, each between two
device events; median, min and max are kept, and peak memory (torch.cuda.max_memory_allocated) of one call of each.  The
baseline is run twice per length, before and after the range entries: the spread between its two medians is the
run-to-run spread the claim is held against.  Nothing in the tests depends on these numbers.

Appends one JSON line per (length, route) to <out>/r08_range.jsonl and rewrites <out>/r08_range_summary.md (default: profiles/)."""
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


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_range.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_range_module()
    dev = torch.device("cuda", 0)
    v, f = W.bunny_standin()
    r = RayMeshIntersector(vertices=torch.from_numpy(v).to(dev), faces=torch.from_numpy(f).to(dev))
    lo, hi = v.min(0), v.max(0)
    extent = float((hi - lo).max())
    o, d = W.hash_rays_torch(args.rays, 83, lo, hi, device=dev)
    d = (d / d.norm(dim=1, keepdim=True).clamp_min(1e-20)).contiguous()
    n = o.shape[0]
    info = r.bvh_info()
    os.makedirs(args.out, exist_ok=True)
    rows = []
    with open(os.path.join(args.out, "r08_range.jsonl"), "a") as fh:
        for label, frac in (("1/64", 1 / 64), ("1/8", 1 / 8), ("1", 1.0), ("unbounded", None)):
            tmax = None if frac is None else torch.full((n,), frac * extent, dtype=torch.float32, device=dev)

            def baseline():
                hit, front, tri, loc, uv = hops.intersects_closest(r.as_wrapper, o, d)
                if tmax is None:
                    return hit
                return hit & ((loc - o).norm(dim=1) <= tmax * d.norm(dim=1))

            def range_any():
                return hops.range_any_native(r.as_wrapper, o, d, None, tmax)

            def range_closest():
                return hops.range_closest_native(r.as_wrapper, o, d, None, tmax)

            blocked = int(range_any().sum())
            agree = int((baseline() == range_any()).sum())
            routes = (("baseline", baseline), ("tr_range_any", range_any), ("tr_range_closest", range_closest), ("baseline_again", baseline))
            res = {}
            for what, fn in routes:
                ms = timed(fn, args.warmup, args.calls)
                res[what] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), peak_mib=peak_mib(fn))
                line = dict(length=label, tmax=None if frac is None else frac * extent, route=what, rays=n, tris=int(info["num_tris"]),
                            blocked=blocked, agree_with_baseline=agree, warmup=args.warmup, calls=args.calls,
                            device=torch.cuda.get_device_name(0), **res[what])
                print(json.dumps(line), flush=True)
                fh.write(json.dumps(line) + "\n")
            rows.append((label, blocked, agree, res))
    with open(os.path.join(args.out, "r08_range_summary.md"), "w") as fh:
        fh.write(f"# Range queries against intersects_closest + torch ({n} hash rays, C2 stand-in, {int(info['num_tris'])} triangles, "
                 f"{torch.cuda.get_device_name(0)})\n\n")
        fh.write("Median ms of %d launches (min - max); peak MiB of one call.  Baseline twice: before and after the range entries.\n\n" % args.calls)
        fh.write("| segment / extent | blocked | baseline | baseline again | tr_range_any | tr_range_closest | peak MiB base / any / closest |\n")
        fh.write("|---|---|---|---|---|---|---|\n")
        cell = lambda x: f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"      # noqa: E731
        for label, blocked, agree, res in rows:
            fh.write(f"| {label} | {blocked / n:.1%} | {cell(res['baseline'])} | {cell(res['baseline_again'])} | {cell(res['tr_range_any'])} | "
                     f"{cell(res['tr_range_closest'])} | {res['baseline']['peak_mib']:.0f} / {res['tr_range_any']['peak_mib']:.0f} / "
                     f"{res['tr_range_closest']['peak_mib']:.0f} |\n")
        fh.write("\nRays on which the baseline's float32 comparison and tr_range_any disagree (hits within rounding of tmax): " +
                 ", ".join(f"{label}: {n - agree}" for label, _, agree, _ in rows) + ".\n")


if __name__ == "__main__":
    main()
