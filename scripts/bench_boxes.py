#!/usr/bin/env python
"""Box queries (libtriro_boxes.so) against the only route there was before them: within_count / faces_within with each box's
circumscribed sphere -- centre of the box, radius = half its diagonal rounded up -- a SUPERSET that a caller would still have to
filter with an exact triangle / box test nobody shipped.

Workload: the headline mesh (W.headline_mesh(): 1 310 720 triangles) and `--cells`^3 boxes of one size, the cells of a dense
grid over the mesh's box (coherent: neighbouring lanes hold neighbouring cells) and the same number of boxes of the same size
at hashed places in that box (incoherent).  surface_voxels runs end to end at the pitch of that grid.

--routes picks what runs: `boxes` (boxes_any, boxes_count, faces_in_boxes), `baseline` (within_count, faces_within: needs
nothing of this library, so the same file times the route on a checkout that does not have the library yet) and `voxels`.

Per kind of boxes, in ONE child process under its own time limit: first the check -- with poisoned outputs (tests/poison.py)
boxes_count and faces_in_boxes of a subset of the boxes against the brute force over the predicate (tests/host_sim/boxes_sim),
every output element written, and the baseline's counts at least the boxes' counts on the whole batch -- then, without the
poison, 3 warm-up calls and `--calls` timed ones of each route, each between two device events (median, min, max); lists
run on a leading part of the boxes where the whole batch would list more than --rows rows.  surface_voxels is timed with a
host clock around a call that ends in a device synchronise.  A step that fails or runs out of time ends the run.  Nothing in
the tests depends on these numbers.

Appends one JSON line per (kind, route) to <out>/r12_boxes.jsonl and, when every route has a line there, rewrites
<out>/r12_boxes_summary.md (default: profiles/)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("grid", "hashed")


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


def timed_host(torch, fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def step(args):
    """one kind of boxes (or the voxels), every route asked for, in this process; prints one JSON line per route"""
    for p in (ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "host_sim")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import workloads as W
    import poison
    import triro.backend.ops as hops
    from triro.ray.ray_optix import RayMeshIntersector
    if not torch.cuda.is_available():
        raise SystemExit("bench_boxes.py needs a GPU: a timing taken anywhere else says nothing")
    routes = set(args.routes.split(","))
    dev = torch.device("cuda", 0)
    v, f = W.headline_mesh()
    lo_m, hi_m = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    G = args.cells
    pitch = float((hi_m - lo_m).max() / G)
    mesh = RayMeshIntersector(vertices=torch.from_numpy(v).to(dev), faces=torch.from_numpy(f).to(dev))
    acc = mesh.as_wrapper
    common = dict(kind=args.step, cells=G, boxes=G ** 3, pitch=pitch, triangles=int(len(f)), warmup=args.warmup, calls=args.calls,
                  device=torch.cuda.get_device_name(0), label=args.label)

    def emit(route, t, **more):
        print(json.dumps(dict(route=route, **t, **more, **common)), flush=True)

    if args.step == "voxels":
        cells = mesh.surface_voxels(pitch)
        # the cells inside the grid are the boxes of the grid that boxes_any says are met, in the same order
        ax = [torch.from_numpy(np.float32(lo_m[a] + np.arange(G + 1, dtype=np.float64) * pitch)).to(dev) for a in range(3)]
        flat = torch.arange(G ** 3, dtype=torch.int64, device=dev)
        ijk = torch.stack((flat // (G * G), (flat // G) % G, flat % G), dim=1)
        met = hops.boxes_native(acc, torch.stack([ax[a][ijk[:, a]] for a in range(3)], dim=1).contiguous(),
                                torch.stack([ax[a][ijk[:, a] + 1] for a in range(3)], dim=1).contiguous(), "any")
        inner = cells[((cells >= 0) & (cells < G)).all(1)]
        assert torch.equal(inner, ijk[met]), "surface_voxels disagrees with boxes_any on the cells of the grid"
        del flat, ijk, met
        emit("surface_voxels", timed_host(torch, lambda: mesh.surface_voxels(pitch), 1, args.calls), cells_met=int(cells.shape[0]),
             cells_met_inside_the_grid=int(inner.shape[0]))
        return

    # the boxes: planes as surface_voxels lays them, float32(origin + i * pitch) evaluated in float64
    planes = [torch.from_numpy(np.float32(lo_m[a] + np.arange(G + 1, dtype=np.float64) * pitch)).to(dev) for a in range(3)]
    n = G ** 3
    if args.step == "grid":
        flat = torch.arange(n, dtype=torch.int64, device=dev)
        ijk = torch.stack((flat // (G * G), (flat // G) % G, flat % G), dim=1)
        lo = torch.stack([planes[a][ijk[:, a]] for a in range(3)], dim=1).contiguous()
        hi = torch.stack([planes[a][ijk[:, a] + 1] for a in range(3)], dim=1).contiguous()
        del flat, ijk
    else:
        size = torch.tensor(pitch, dtype=torch.float32, device=dev)
        lo = W.hash_rays_torch(n, 131, lo_m.astype(np.float32), (hi_m - pitch).astype(np.float32), device=dev)[0].contiguous()
        hi = (lo + size).contiguous()
    centre = ((lo.double() + hi.double()) / 2).float().contiguous()
    # half the diagonal, rounded up twice: the sphere holds the box whatever the float32 centre lost
    radius = torch.nextafter(torch.nextafter(((hi.double() - lo.double()).pow(2).sum(1).sqrt() / 2).float(), centre.new_tensor(float("inf"))),
                             centre.new_tensor(float("inf"))) + torch.finfo(torch.float32).eps * centre.abs().amax(1)
    radius = radius.contiguous()

    have_boxes = "boxes" in routes
    count = None
    if have_boxes:
        import boxes_sim
        hops.get_boxes_module()
        poison.install()
        count = hops.boxes_native(acc, lo, hi, "count")
        any_ = hops.boxes_native(acc, lo, hi, "any")
        torch.cuda.synchronize()
        poison.assert_written(count, any_, what="boxes_native")
        assert bool(((count > 0) == any_).all())
        met = torch.nonzero(count > 0).reshape(-1)
        pick = torch.cat([met[:: max(1, len(met) // (args.check // 2))][: args.check // 2],
                          torch.arange(0, n, max(1, n // (args.check // 2)), device=dev)[: args.check // 2]])
        off, face, inside = hops.faces_in_boxes_native(acc, lo[pick].contiguous(), hi[pick].contiguous(), True)
        torch.cuda.synchronize()
        poison.assert_written(off, face, inside, what="faces_in_boxes_native")
        want = boxes_sim.brute(v, f, lo[pick].cpu().numpy(), hi[pick].cpu().numpy())
        assert np.array_equal(count[pick].cpu().numpy(), want.count) and np.array_equal(off.cpu().numpy(), want.offsets)
        assert np.array_equal(face.cpu().numpy(), want.faces) and np.array_equal(inside.cpu().numpy(), want.inside)
        common.update(checked_boxes=int(len(pick)), checked_rows=int(want.offsets[-1]), met_fraction=float((count > 0).double().mean()),
                      mean_count=float(count.double().mean()))
        poison.uninstall()
        del any_, off, face, inside
    if "baseline" in routes:
        poison.install()
        wcount = hops.within_native(acc, centre, radius, "count")
        torch.cuda.synchronize()
        poison.assert_written(wcount, what="within_native")
        poison.uninstall()
        if count is not None:
            assert bool((wcount >= count).all()), "the circumscribed sphere lists fewer faces than its box"
        common.update(sphere_mean_count=float(wcount.double().mean()), sphere_met_fraction=float((wcount > 0).double().mean()))
        mean_rows = float(wcount.double().mean())
        del wcount
    else:
        mean_rows = float(count.double().mean())
    # the lists of both routes run on the same leading part of the boxes: the larger mean count (the spheres') sizes it
    n_rows = n if mean_rows * n <= args.rows else max(1 << 12, int(args.rows / max(mean_rows, 1e-9)) // 128 * 128)
    n_rows = min(n, n_rows)
    lo_r, hi_r, centre_r, radius_r = lo[:n_rows].contiguous(), hi[:n_rows].contiguous(), centre[:n_rows].contiguous(), radius[:n_rows].contiguous()
    torch.cuda.empty_cache()

    plan = []
    if have_boxes:
        plan += [("boxes_any", lambda: hops.boxes_native(acc, lo, hi, "any"), n, False),
                 ("boxes_count", lambda: hops.boxes_native(acc, lo, hi, "count"), n, False),
                 ("faces_in_boxes", lambda: hops.faces_in_boxes_native(acc, lo_r, hi_r), n_rows, True),
                 ("faces_in_boxes_inside", lambda: hops.faces_in_boxes_native(acc, lo_r, hi_r, True), n_rows, True)]
    if "baseline" in routes:
        plan += [("within_count", lambda: hops.within_native(acc, centre, radius, "count"), n, False),
                 ("faces_within", lambda: hops.faces_within_native(acc, centre_r, radius_r), n_rows, True)]
    if have_boxes:
        plan += [("boxes_count_again", lambda: hops.boxes_native(acc, lo, hi, "count"), n, False)]
    elif "baseline" in routes:
        plan += [("within_count_again", lambda: hops.within_native(acc, centre, radius, "count"), n, False)]
    for route, fn, used, lists in plan:
        rows = int(fn()[0][-1]) if lists else 0
        t = timed(torch, fn, args.warmup, args.calls)
        emit(route, t, boxes_used=used, rows=rows, rows_per_s=rows / (t["median_ms"] * 1e-3) if rows else 0.0,
             boxes_per_s=used / (t["median_ms"] * 1e-3))
        torch.cuda.empty_cache()


def cell(x):
    return f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"


def summary(lines, path):
    by = {}
    for ln in lines:                                  # (the last line of a route wins: the file is appended to)
        by.setdefault(ln["kind"], {})[ln["route"]] = ln
    need = ("boxes_count", "faces_in_boxes", "within_count", "faces_within")
    if not all(k in by and all(r in by[k] for r in need) for k in KINDS):
        return False
    first = by["grid"]["boxes_count"]
    with open(path, "w") as fh:
        fh.write(f"# Box queries against within_count / faces_within on the circumscribed spheres ({first['boxes']} boxes of side "
                 f"{first['pitch']:.4g}, the headline mesh of {first['triangles']} triangles, {first['device']})\n\n")
        fh.write(f"Median ms of {first['calls']} calls (min - max) after {first['warmup']} warm-ups, each kind of boxes in a process of its own.  "
                 "grid = the cells of a dense grid over the mesh's box in lexicographic order; hashed = as many boxes of the same size at "
                 "hashed places.  The sphere route is a superset that still needs a filter: `mean count` is what each route lists per box.  "
                 "Lists (count + scan + host read + fill + ordering) run on the leading `boxes used` of the batch.  Before the timing, with "
                 "poisoned outputs: counts, offsets, faces and inside flags of a subset of the boxes equal the brute force, and every sphere "
                 "counts at least what its box counts.  The sphere route's figures are those of the run labelled "
                 f"'{by['grid']['within_count']['label'] or 'this tree'}' (--label; the route needs nothing of libtriro_boxes.so, so it is timed on "
                 "the commit before the library as well).\n\n")
        fh.write("| boxes | met | mean count box / sphere | boxes_any | boxes_count | again | within_count (spheres) | count: boxes / spheres | "
                 "faces_in_boxes (boxes used, rows, rows/s) | + inside | faces_within (rows, rows/s) | lists: boxes / spheres | checked boxes (rows) |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        notes = []
        for kind in KINDS:
            b = by[kind]
            bc, wc, fb, fw = b["boxes_count"], b["within_count"], b["faces_in_boxes"], b["faces_within"]
            fh.write(f"| {kind} | {bc['met_fraction']:.1%} | {bc['mean_count']:.2f} / {wc['sphere_mean_count']:.2f} | {cell(b['boxes_any'])} | {cell(bc)} | "
                     f"{cell(b['boxes_count_again'])} | {cell(wc)} | {bc['median_ms'] / wc['median_ms']:.3f}x | {cell(fb)} ({fb['boxes_used']}, {fb['rows']}, "
                     f"{fb['rows_per_s']:.3g}) | {cell(b['faces_in_boxes_inside'])} | {cell(fw)} ({fw['rows']}, {fw['rows_per_s']:.3g}) | "
                     f"{fb['median_ms'] / fw['median_ms']:.3f}x | {bc['checked_boxes']} ({bc['checked_rows']}) |\n")
            for mine, theirs, name in ((bc, wc, "boxes_count"), (fb, fw, "faces_in_boxes")):
                if mine["median_ms"] >= theirs["median_ms"]:
                    notes.append(f"On the {kind} boxes {name} is NOT faster than the sphere route ({mine['median_ms']:.3f} ms against {theirs['median_ms']:.3f} ms).")
        if "voxels" in by:
            sv = by["voxels"]["surface_voxels"]
            fh.write(f"\nsurface_voxels(pitch = {sv['pitch']:.4g}) end to end (host clock, synchronised): {cell(sv)} ms for {sv['boxes']}+ cells, "
                     f"{sv['cells_met']} of them met.\n")
        fh.write("\n" + ("\n".join(notes) if notes else "Both box queries are faster than the sphere route on both kinds of boxes.") + "\n")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=320, help="cells per axis of the grid: cells^3 boxes")
    ap.add_argument("--routes", default="boxes,baseline,voxels")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rows", type=float, default=1.5e8, help="most rows a list call may list")
    ap.add_argument("--check", type=int, default=256, help="boxes checked against the brute force")
    ap.add_argument("--limit", type=int, default=170, help="seconds one kind of boxes may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--label", default="", help="a word kept in every line, such as the commit the run was made on")
    ap.add_argument("--step", default=None, help="(internal) run this kind of boxes in this process")
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    os.makedirs(args.out, exist_ok=True)
    routes = set(args.routes.split(","))
    steps = [k for k in KINDS if routes & {"boxes", "baseline"}] + (["voxels"] if "voxels" in routes else [])
    log = os.path.join(args.out, "r12_boxes.jsonl")
    with open(log, "a") as fh:
        for kind in steps:      # the parent never touches the GPU: every kind is a fresh child under its own time limit
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", kind, "--cells", str(args.cells),
                   "--routes", args.routes, "--warmup", str(args.warmup), "--calls", str(args.calls), "--rows", repr(args.rows), "--check", str(args.check), "--label", args.label]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            for ln in res.stdout.splitlines():
                print(ln, flush=True)
                if ln.startswith("{"):
                    fh.write(ln + "\n")
            if res.returncode != 0:
                raise SystemExit(f"the step {kind} ended with status {res.returncode}: nothing more is started")
    lines = [json.loads(ln) for ln in open(log) if ln.startswith("{")]
    if not summary(lines, os.path.join(args.out, "r12_boxes_summary.md")):
        print("(no summary yet: the log does not hold every route)")


if __name__ == "__main__":
    main()
