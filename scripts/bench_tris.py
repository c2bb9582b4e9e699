#!/usr/bin/env python
"""Triangle queries (libtriro_tris.so) against the only route there was before them: boxes_count / faces_in_boxes on the boxes
of the query triangles -- the broad phase, a SUPERSET that a caller would still have to filter with an exact triangle /
triangle test nobody shipped.  The two routes do not compute the same set: the table says what the exact answer costs over the
superset and how many rows it saves a caller.

Workload: the headline mesh (W.headline_mesh(): 1 310 720 triangles) against as many query triangles: `displaced`, its own
faces moved by --shift of the extent (coherent: neighbouring lanes hold neighbouring faces, many contacts), and `hashed`,
triangles of the mean face size at hashed places in the mesh's box (incoherent).  mesh_contacts runs end to end on the
displaced copy.

--routes picks what runs: `tris` (triangles_any, triangles_count, faces_meeting_triangles), `baseline` (boxes_count,
faces_in_boxes: needs nothing of this library, so the same file times the route on a checkout that does not have the library
yet) and `contacts`.

Per kind of queries, in ONE child process under its own time limit: first the check -- with poisoned outputs (tests/poison.py)
counts and lists of a subset of the queries against the brute force over the predicate (tests/host_sim/tris_sim), every output
element written, and the baseline's counts at least the exact counts on the whole batch -- then, without the poison, 3 warm-up
calls and `--calls` timed ones of each route, each between two device events (median, min, max).  mesh_contacts is timed with
a host clock around a call that ends in a device synchronise.  A step that fails or runs out of time ends the run.  Nothing in
the tests depends on these numbers.

Appends one JSON line per (kind, route) to <out>/r13_tris.jsonl and, when every route has a line there, rewrites
<out>/r13_tris_summary.md (default: profiles/)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_boxes import cell, timed, timed_host  # noqa: E402  (the same clocks as the box queries' table)

KINDS = ("displaced", "hashed")


def step(args):
    """one kind of queries (or the contacts), every route asked for, in this process; prints one JSON line per route"""
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
        raise SystemExit("bench_tris.py needs a GPU: a timing taken anywhere else says nothing")
    routes = set(args.routes.split(","))
    dev = torch.device("cuda", 0)
    v, f = W.headline_mesh()
    lo_m, hi_m = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = float((hi_m - lo_m).max())
    shift = (np.float64(args.shift * ext) * np.array([2, -1, 2]) / 3).astype(np.float32)
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    mesh = RayMeshIntersector(vertices=vt, faces=ft)
    acc = mesh.as_wrapper
    n = int(len(f))
    common = dict(kind=args.step, queries=n, shift=args.shift, triangles=n, warmup=args.warmup, calls=args.calls,
                  device=torch.cuda.get_device_name(0), label=args.label)

    def emit(route, t, **more):
        print(json.dumps(dict(route=route, **t, **more, **common)), flush=True)

    moved = (vt + torch.from_numpy(shift).to(dev)).contiguous()
    if args.step == "contacts":
        pairs = mesh.mesh_contacts(moved, ft)
        off, face = mesh.faces_meeting_triangles(moved[ft.long()])
        assert int(off[-1]) == pairs.shape[0] and torch.equal(pairs[:, 1], face.long())
        assert torch.equal(pairs[:, 0], torch.repeat_interleave(torch.arange(n, device=dev), torch.diff(off)))
        assert mesh.mesh_collides(moved, ft) is (pairs.shape[0] > 0)
        emit("mesh_contacts", timed_host(torch, lambda: mesh.mesh_contacts(moved, ft), 1, args.calls), rows=int(pairs.shape[0]))
        return

    if args.step == "displaced":
        tri = moved[ft.long()].contiguous()
    else:
        own = vt[ft.long()]
        size = float((own.amax(1) - own.amin(1)).amax(1).double().mean())          # the mean face size: the longest side of its box
        c = W.hash_rays_torch(n, 131, lo_m.astype(np.float32), hi_m.astype(np.float32), device=dev)[0]
        d = torch.stack([W.hash_rays_torch(n, 137 + k, np.float32([-0.5] * 3), np.float32([0.5] * 3), device=dev)[0] for k in range(3)], dim=1)
        tri = (c[:, None, :] + d * size).contiguous()
        common.update(size=size)
    lo, hi = tri.amin(1).contiguous(), tri.amax(1).contiguous()                      # the boxes of the queries: the broad phase

    have_tris = "tris" in routes
    count = None
    if have_tris:
        import tris_sim
        hops.get_tris_module()
        poison.install()
        count = hops.tris_native(acc, tri, "count")
        any_ = hops.tris_native(acc, tri, "any")
        torch.cuda.synchronize()
        poison.assert_written(count, any_, what="tris_native")
        assert bool(((count > 0) == any_).all())
        met = torch.nonzero(count > 0).reshape(-1)
        pick = torch.cat([met[:: max(1, len(met) // (args.check // 2))][: args.check // 2],
                          torch.arange(0, n, max(1, n // (args.check // 2)), device=dev)[: args.check // 2]])
        off, face = hops.faces_meeting_triangles_native(acc, tri[pick].contiguous())
        torch.cuda.synchronize()
        poison.assert_written(off, face, what="faces_meeting_triangles_native")
        want = tris_sim.brute(v, f, tri[pick].cpu().numpy())
        assert np.array_equal(count[pick].cpu().numpy(), want.count) and np.array_equal(off.cpu().numpy(), want.offsets)
        assert np.array_equal(face.cpu().numpy(), want.faces)
        common.update(checked_queries=int(len(pick)), checked_rows=int(want.offsets[-1]), met_fraction=float((count > 0).double().mean()),
                      mean_count=float(count.double().mean()))
        poison.uninstall()
        del any_, off, face
    if "baseline" in routes:
        poison.install()
        bcount = hops.boxes_native(acc, lo, hi, "count")
        torch.cuda.synchronize()
        poison.assert_written(bcount, what="boxes_native")
        poison.uninstall()
        if count is not None:
            assert bool((bcount >= count).all()), "the box of a query lists fewer faces than the query"
        common.update(box_mean_count=float(bcount.double().mean()), box_met_fraction=float((bcount > 0).double().mean()))
        del bcount
    torch.cuda.empty_cache()

    plan = []
    if have_tris:
        plan += [("triangles_any", lambda: hops.tris_native(acc, tri, "any"), False),
                 ("triangles_count", lambda: hops.tris_native(acc, tri, "count"), False),
                 ("faces_meeting_triangles", lambda: hops.faces_meeting_triangles_native(acc, tri), True)]
    if "baseline" in routes:
        plan += [("boxes_count", lambda: hops.boxes_native(acc, lo, hi, "count"), False),
                 ("faces_in_boxes", lambda: hops.faces_in_boxes_native(acc, lo, hi), True)]
    if have_tris:
        plan += [("triangles_count_again", lambda: hops.tris_native(acc, tri, "count"), False)]
    elif "baseline" in routes:
        plan += [("boxes_count_again", lambda: hops.boxes_native(acc, lo, hi, "count"), False)]
    for route, fn, lists in plan:
        rows = int(fn()[0][-1]) if lists else 0
        t = timed(torch, fn, args.warmup, args.calls)
        emit(route, t, rows=rows, rows_per_s=rows / (t["median_ms"] * 1e-3) if rows else 0.0, queries_per_s=n / (t["median_ms"] * 1e-3))
        torch.cuda.empty_cache()


def summary(lines, path):
    by = {}
    for ln in lines:                                  # (the last line of a route wins: the file is appended to)
        by.setdefault(ln["kind"], {})[ln["route"]] = ln
    need = ("triangles_count", "faces_meeting_triangles", "boxes_count", "faces_in_boxes")
    if not all(k in by and all(r in by[k] for r in need) for k in KINDS):
        return False
    first = by["displaced"]["triangles_count"]
    with open(path, "w") as fh:
        fh.write(f"# Triangle queries against boxes_count / faces_in_boxes on the queries' boxes ({first['queries']} query triangles, the "
                 f"headline mesh of {first['triangles']} triangles, {first['device']})\n\n")
        fh.write(f"Median ms of {first['calls']} calls (min - max) after {first['warmup']} warm-ups, each kind of queries in a process of its own.  "
                 f"displaced = the mesh's own faces moved by {first['shift']:g} of the extent; hashed = as many triangles of the mean face size at "
                 "hashed places.  The box route is the broad phase, a superset that still needs an exact filter, so the two columns do not "
                 "compute the same set: `mean count` is what each route lists per query.  Lists are count + scan + host read + fill + ordering "
                 "on the whole batch.  Before the timing, with poisoned outputs: counts, offsets and faces of a subset of the queries equal "
                 "the brute force, and every box counts at least what its triangle counts.  The box route's figures are those of the run "
                 f"labelled '{by['displaced']['boxes_count']['label'] or 'this tree'}' (--label; the route needs nothing of libtriro_tris.so, so "
                 "it is timed on the commit before the library).\n\n")
        fh.write("| queries | met | mean count triangle / box | triangles_any | triangles_count | again | boxes_count (boxes) | count: triangles / boxes | "
                 "faces_meeting_triangles (rows, rows/s) | faces_in_boxes (rows, rows/s) | lists: triangles / boxes | rows saved | checked queries (rows) |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for kind in KINDS:
            b = by[kind]
            tc, bc, ft, fb = b["triangles_count"], b["boxes_count"], b["faces_meeting_triangles"], b["faces_in_boxes"]
            fh.write(f"| {kind} | {tc['met_fraction']:.1%} | {tc['mean_count']:.2f} / {bc['box_mean_count']:.2f} | {cell(b['triangles_any'])} | {cell(tc)} | "
                     f"{cell(b['triangles_count_again'])} | {cell(bc)} | {tc['median_ms'] / bc['median_ms']:.3f}x | {cell(ft)} ({ft['rows']}, "
                     f"{ft['rows_per_s']:.3g}) | {cell(fb)} ({fb['rows']}, {fb['rows_per_s']:.3g}) | {ft['median_ms'] / fb['median_ms']:.3f}x | "
                     f"{fb['rows'] - ft['rows']} ({1 - ft['rows'] / max(fb['rows'], 1):.1%}) | {tc['checked_queries']} ({tc['checked_rows']}) |\n")
        if "contacts" in by:
            mc = by["contacts"]["mesh_contacts"]
            fh.write(f"\nmesh_contacts of the displaced copy end to end (host clock, synchronised): {cell(mc)} ms for {mc['queries']} faces against "
                     f"{mc['triangles']}, {mc['rows']} contact pairs.\n")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shift", type=float, default=1 / 512, help="the displacement of the copy, as a fraction of the extent")
    ap.add_argument("--routes", default="tris,baseline,contacts")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--check", type=int, default=256, help="queries checked against the brute force")
    ap.add_argument("--limit", type=int, default=170, help="seconds one kind of queries may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--label", default="", help="a word kept in every line, such as the commit the run was made on")
    ap.add_argument("--step", default=None, help="(internal) run this kind of queries in this process")
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    os.makedirs(args.out, exist_ok=True)
    routes = set(args.routes.split(","))
    steps = [k for k in KINDS if routes & {"tris", "baseline"}] + (["contacts"] if "contacts" in routes else [])
    log = os.path.join(args.out, "r13_tris.jsonl")
    with open(log, "a") as fh:
        for kind in steps:      # the parent never touches the GPU: every kind is a fresh child under its own time limit
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", kind, "--shift", repr(args.shift),
                   "--routes", args.routes, "--warmup", str(args.warmup), "--calls", str(args.calls), "--check", str(args.check), "--label", args.label]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            for ln in res.stdout.splitlines():
                print(ln, flush=True)
                if ln.startswith("{"):
                    fh.write(ln + "\n")
            if res.returncode != 0:
                raise SystemExit(f"the step {kind} ended with status {res.returncode}: nothing more is started")
    lines = [json.loads(ln) for ln in open(log) if ln.startswith("{")]
    if not summary(lines, os.path.join(args.out, "r13_tris_summary.md")):
        print("(no summary yet: the log does not hold every route)")


if __name__ == "__main__":
    main()
