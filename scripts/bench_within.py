#!/usr/bin/env python
"""Radius queries (libtriro_within.so) against the only route there was before them: closest_point followed by a comparison
of the float32 distance with r.  That route answers within_any and closest_point(max_distance) only -- it has no count and no
list -- and it is NOT exact at the boundary (a float64 d2 slightly above r^2 can round to a distance equal to r), which is
why the native entries exist besides being bounded from the first node.

Workload: the C2 stand-in (W.bunny_standin(): 81 920 triangles), 10 M hash points in 1.2x its box, radii of 1 %, 5 % and 25 %
of the extent.  within_count and faces_within test every face inside the radius: where the points x mean count of the whole
batch exceeds --pairs (default 2e9 for count, 1.5e8 rows for the lists) they run on a leading part of the points, and the
table says on how many.

Per radius, in ONE child process under its own time limit: 3 warm-up launches and `--calls` timed ones of each route, each
between two device events (median, min, max); the baseline is timed before and after the rest: the spread between its two
medians is the run-to-run spread.  A step that fails or runs out of time ends the run.  Nothing in the tests depends on these
numbers.

Appends one JSON line per (radius, route) to <out>/r10_within.jsonl and rewrites <out>/r10_within_summary.md (default:
profiles/)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = (0.01, 0.05, 0.25)


def timed(torch, fn, warmup, calls):
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
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def step(args):
    """one radius, every route, in this process; prints one JSON line per route"""
    for p in (ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import workloads as W
    import triro.backend.ops as hops
    from triro.ray.ray_optix import RayMeshIntersector
    if not torch.cuda.is_available():
        raise SystemExit("bench_within.py needs a GPU: a timing taken anywhere else says nothing")
    hops.get_within_module()
    dev = torch.device("cuda", 0)
    v, f = W.bunny_standin()
    extent = float((v.max(0) - v.min(0)).max())
    r = float(np.float32(args.step * extent))
    mid, half = (v.max(0) + v.min(0)) / 2, (v.max(0) - v.min(0)) / 2
    pts = W.hash_rays_torch(args.points, 97, mid - 1.2 * half, mid + 1.2 * half, device=dev)[0].contiguous()
    n = pts.shape[0]
    mesh = RayMeshIntersector(vertices=torch.from_numpy(v).to(dev), faces=torch.from_numpy(f).to(dev))
    acc = mesh.as_wrapper

    # what the batch holds: how many points have a face within r, the mean count (on the first 2^17 points)
    probe = hops.within_native(acc, pts[:1 << 17], r, "count")
    mean_count = float(probe.to(torch.float64).mean())
    any_frac = float((probe > 0).to(torch.float64).mean())
    n_count = n if mean_count * n <= args.pairs else max(1 << 17, int(args.pairs / max(mean_count, 1e-9)) // 128 * 128)
    n_rows = n if mean_count * n <= args.rows else max(1 << 12, int(args.rows / max(mean_count, 1e-9)) // 128 * 128)
    n_count, n_rows = min(n, n_count), min(n, n_rows)
    del probe

    def baseline():      # the parent commit's route: the unbounded nearest, then a comparison of float32 distances
        c, d, t = hops.closest_point_native(acc, pts)
        near = d <= r
        return near, torch.where(near, t, -1)

    def run_any():
        return hops.within_native(acc, pts, r, "any")

    def run_count():
        return hops.within_native(acc, pts[:n_count], r, "count")

    def run_lists():
        return hops.faces_within_native(acc, pts[:n_rows], r)

    def run_lists_rows():
        return hops.faces_within_native(acc, pts[:n_rows], r, True, True)

    def run_bounded():
        return hops.within_closest_native(acc, pts, r)

    # agreement of the two routes (the baseline is not exact at the boundary: counted, not asserted)
    near, tri = baseline()
    differ_any = int((near != run_any()).sum())
    differ_tri = int((tri != run_bounded()[2]).sum())
    rows_total = int(run_lists()[0][-1])
    del near, tri
    torch.cuda.empty_cache()
    common = dict(fraction=args.step, radius=r, points=n, triangles=int(len(f)), any_fraction=any_frac, mean_count=mean_count,
                  differ_any=differ_any, differ_tri=differ_tri, warmup=args.warmup, calls=args.calls, device=torch.cuda.get_device_name(0))
    for route, fn, used, rows in (("baseline", baseline, n, 0), ("within_any", run_any, n, 0), ("within_count", run_count, n_count, 0),
                                  ("faces_within", run_lists, n_rows, rows_total), ("faces_within_rows", run_lists_rows, n_rows, rows_total),
                                  ("closest_point_bounded", run_bounded, n, 0), ("baseline_again", baseline, n, 0)):
        t = timed(torch, fn, args.warmup, args.calls)
        line = dict(route=route, points_used=used, rows=rows, rows_per_s=rows / (t["median_ms"] * 1e-3) if rows else 0.0, **t, **common)
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()


def cell(x):
    return f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"


def summary(lines, path, calls):
    by = {}
    for ln in lines:
        by.setdefault(ln["fraction"], {})[ln["route"]] = ln
    with open(path, "w") as fh:
        first = lines[0]
        fh.write(f"# Radius queries against closest_point + comparison ({first['points']} hash points in 1.2x the box of the C2 stand-in, "
                 f"{first['triangles']} triangles, {first['device']})\n\n")
        fh.write(f"Median ms of {calls} launches (min - max) after 3 warm-ups, each radius in a process of its own.  Baseline = "
                 "tr_closest_point, then `distance <= r` and a select in torch: the only route before this library; it answers within_any "
                 "and the bounded nearest only, and not exactly at the boundary (`differ` = points on which it disagrees with the native "
                 "entry).  within_count and faces_within run on the leading `points used` of the batch where the whole batch would list too "
                 "many pairs.  faces_within = count + scan + host read + fill + ordering; `+ rows` adds distance and closest per row.\n\n")
        fh.write("| r / extent | points with a face within | mean count | baseline | baseline again | within_any | any / baseline | closest_point(max_distance) | "
                 "bounded / baseline | differ any / nearest | within_count (points used) | faces_within (points used, rows, rows/s) | faces_within + rows (rows/s) |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        notes = []
        for fr in sorted(by):
            b = by[fr]
            base = b["baseline"]["median_ms"]
            fh.write(f"| {fr:g} | {b['baseline']['any_fraction']:.1%} | {b['baseline']['mean_count']:.1f} | {cell(b['baseline'])} | {cell(b['baseline_again'])} | "
                     f"{cell(b['within_any'])} | {b['within_any']['median_ms'] / base:.3f}x | {cell(b['closest_point_bounded'])} | "
                     f"{b['closest_point_bounded']['median_ms'] / base:.3f}x | {b['baseline']['differ_any']} / {b['baseline']['differ_tri']} | "
                     f"{cell(b['within_count'])} ({b['within_count']['points_used']}) | {cell(b['faces_within'])} ({b['faces_within']['points_used']}, "
                     f"{b['faces_within']['rows']}, {b['faces_within']['rows_per_s']:.3g}) | {cell(b['faces_within_rows'])} ({b['faces_within_rows']['rows_per_s']:.3g}) |\n")
            for route, name in (("within_any", "within_any"), ("closest_point_bounded", "closest_point(max_distance)")):
                if b[route]["median_ms"] >= min(base, b["baseline_again"]["median_ms"]):
                    notes.append(f"At r = {fr:g} of the extent {name} is NOT faster than the unbounded closest_point + comparison "
                                 f"({b[route]['median_ms']:.3f} ms against {base:.3f} / {b['baseline_again']['median_ms']:.3f} ms).")
        fh.write("\n" + ("\n".join(notes) if notes else "Every bounded query above is faster than the unbounded closest_point + comparison at every radius measured.") + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--pairs", type=float, default=2e9, help="most (point, face) pairs a within_count launch may find")
    ap.add_argument("--rows", type=float, default=1.5e8, help="most rows a faces_within call may list")
    ap.add_argument("--limit", type=int, default=170, help="seconds one radius may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", type=float, default=None, help="(internal) run this fraction of the extent in this process")
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    os.makedirs(args.out, exist_ok=True)
    lines = []
    with open(os.path.join(args.out, "r10_within.jsonl"), "a") as fh:
        for fr in FRACTIONS:      # the parent never touches the GPU: every radius is a fresh child under its own time limit
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", repr(fr), "--points", str(args.points),
                   "--warmup", str(args.warmup), "--calls", str(args.calls), "--pairs", repr(args.pairs), "--rows", repr(args.rows)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            for ln in res.stdout.splitlines():
                print(ln, flush=True)
                if ln.startswith("{"):
                    lines.append(json.loads(ln))
                    fh.write(ln + "\n")
            if res.returncode != 0:
                raise SystemExit(f"the step r = {fr:g} of the extent ended with status {res.returncode}: nothing more is started")
    summary(lines, os.path.join(args.out, "r10_within_summary.md"), args.calls)


if __name__ == "__main__":
    main()
