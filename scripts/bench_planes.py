#!/usr/bin/env python
"""Plane queries (libtriro_planes.so) against what a user of this library wrote before them: the signed values (V - o) . n of
every vertex for every plane in float64 with torch on the same GPU (this is how trimesh.intersections.mesh_multiplane works),
the signs gathered per face, and nonzero -- in chunks of `--chunk` planes, as memory demands.  Nothing on the commit before the
library answers this query.

Workload: the headline mesh (W.headline_mesh(): 1 310 720 triangles) and `--planes` planes (1 024): `parallel` = normal (0, 0, 1),
evenly spaced over the mesh's extent along z; `hashed` = the same origins with hashed normals.

Per kind of planes, in ONE child process under its own time limit: first the check -- with poisoned outputs (tests/poison.py)
planes_count, faces_on_planes and section_segments of a subset of the planes against the brute force over the predicate
(tests/host_sim/planes_sim), every output element written, the segments of every plane closing into loops bit for bit, and the
torch route's counts against the native ones on the whole batch (equal on the parallel planes, where both sums are exact
differences; on hashed normals the two float64 sums round differently and the number of planes that differ is recorded) -- then,
without the poison, `--warmup` warm-up calls and `--calls` timed ones of each route, each between two device events (median, min,
max).  The torch route stops at the list of (plane, face): it computes no segments, so it is a LOWER bound of a baseline for
section_segments.  A step that fails or runs out of time ends the run.  Nothing in the tests depends on these numbers.

Appends one JSON line per (kind, route) to <out>/r15_planes.jsonl and, when every route has a line there, rewrites
<out>/r15_planes_summary.md (default: profiles/)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("parallel", "hashed")


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
    """one kind of planes, every route, in this process; prints one JSON line per route"""
    for p in (ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "host_sim")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import workloads as W
    import planes_cases as PC
    import planes_sim
    import poison
    import triro.backend.ops as hops
    from triro.ray.ray_optix import RayMeshIntersector
    if not torch.cuda.is_available():
        raise SystemExit("bench_planes.py needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    v, f = W.headline_mesh()
    lo_m, hi_m = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    n = args.planes
    z = lo_m[2] + (np.arange(n, dtype=np.float64) + 0.5) / n * (hi_m[2] - lo_m[2])
    centre = 0.5 * (lo_m + hi_m)
    o_np = np.float32(np.stack([np.full(n, centre[0]), np.full(n, centre[1]), z], 1))
    if args.step == "parallel":
        n_np = np.tile(np.float32([0, 0, 1]), (n, 1))
    else:
        n_np = np.ascontiguousarray(W.hash_rays(n, 151, np.float32([-1, -1, -1]), np.float32([1, 1, 1]))[0], np.float32)
    mesh = RayMeshIntersector(vertices=torch.from_numpy(v).to(dev), faces=torch.from_numpy(f).to(dev))
    acc = mesh.as_wrapper
    o, nr = torch.from_numpy(o_np).to(dev), torch.from_numpy(n_np).to(dev)
    V64 = mesh.mesh_vertices.double()
    F = mesh.mesh_faces.long()
    common = dict(kind=args.step, planes=n, triangles=int(len(f)), warmup=args.warmup, calls=args.calls, chunk=args.chunk,
                  device=torch.cuda.get_device_name(0), label=args.label)

    def emit(route, t, **more):
        print(json.dumps(dict(route=route, **t, **more, **common)), flush=True)

    # the torch route: signed values per vertex in float64, signs gathered per face
    def torch_tables(a, b, cut):
        o64, n64 = o[a:b].double(), nr[a:b].double()
        s = ((V64[None, :, :] - o64[:, None, :]) * n64[:, None, :]).sum(-1)           # [p, NV]
        pos, neg = (s > 0)[:, F], (s < 0)[:, F]                                       # [p, NF, 3]
        if cut:
            zero = (s == 0)[:, F]
            return pos.any(-1) & (neg.any(-1) | (zero.sum(-1) == 2))
        return ~(pos.all(-1) | neg.all(-1))

    def torch_count(cut):
        return torch.cat([torch_tables(a, min(a + args.chunk, n), cut).sum(1, dtype=torch.int32) for a in range(0, n, args.chunk)])

    def torch_faces(cut):
        counts, faces = [], []
        for a in range(0, n, args.chunk):
            t = torch_tables(a, min(a + args.chunk, n), cut)
            counts.append(t.sum(1, dtype=torch.int32))
            faces.append(torch.nonzero(t)[:, 1].to(torch.int32))
        return torch.cat(counts), torch.cat(faces)

    # ---- the check ----
    hops.get_planes_module()
    poison.install()
    count_meet = hops.planes_native(acc, o, nr, "count", False)
    count_cut = hops.planes_native(acc, o, nr, "count", True)
    any_ = hops.planes_native(acc, o, nr, "any", False)
    torch.cuda.synchronize()
    poison.assert_written(count_meet, count_cut, any_, what="planes_native")
    assert bool(((count_meet > 0) == any_).all()) and bool((count_cut <= count_meet).all())
    pick = torch.arange(0, n, max(1, n // args.check), device=dev)[: args.check]
    op, npk = o[pick].contiguous(), nr[pick].contiguous()
    for cut in (False, True):
        off, face, seg = hops.faces_on_planes_native(acc, op, npk, cut, cut)
        torch.cuda.synchronize()
        poison.assert_written(off, face, seg, what="faces_on_planes_native")
        want = planes_sim.brute(v, f, op.cpu().numpy(), npk.cpu().numpy(), cut=cut)
        got = planes_sim.Result(None, (count_cut if cut else count_meet)[pick].cpu().numpy(), off.cpu().numpy(), face.cpu().numpy(),
                                None if seg is None else seg.cpu().numpy())
        PC.assert_same(got, want, f"bench check, cut={cut}")
    off, face, seg = hops.faces_on_planes_native(acc, o, nr, True, True)
    torch.cuda.synchronize()
    poison.assert_written(off, face, seg, what="section_segments")
    whole = planes_sim.Result(None, count_cut.cpu().numpy(), off.cpu().numpy(), face.cpu().numpy(), seg.cpu().numpy())
    rows_closed = PC.loops_close(whole, "bench check: the sections of the whole batch")
    poison.uninstall()
    t_meet, t_cut = torch_count(False), torch_count(True)
    differ = int((t_meet != count_meet).sum()) + int((t_cut != count_cut).sum())
    if args.step == "parallel":
        assert differ == 0, "the torch route counts other faces than the native one on planes where both sums are exact"
    rows_meet, rows_cut = int(count_meet.sum()), int(count_cut.sum())
    common.update(rows_meet=rows_meet, rows_cut=rows_cut, checked_planes=int(len(pick)), rows_closed=int(rows_closed),
                  planes_whose_torch_count_differs=differ, max_rows_of_a_plane=int(count_meet.max()))
    del off, face, seg, whole, t_meet, t_cut
    torch.cuda.empty_cache()

    plan = [("planes_any", lambda: hops.planes_native(acc, o, nr, "any", False), 0),
            ("planes_count", lambda: hops.planes_native(acc, o, nr, "count", False), rows_meet),
            ("planes_count_cut", lambda: hops.planes_native(acc, o, nr, "count", True), rows_cut),
            ("faces_on_planes", lambda: hops.faces_on_planes_native(acc, o, nr, False), rows_meet),
            ("faces_on_planes_cut", lambda: hops.faces_on_planes_native(acc, o, nr, True), rows_cut),
            ("section_segments", lambda: hops.faces_on_planes_native(acc, o, nr, True, True), rows_cut),
            ("torch_count", lambda: torch_count(False), rows_meet),
            ("torch_count_cut", lambda: torch_count(True), rows_cut),
            ("torch_faces", lambda: torch_faces(False), rows_meet),
            ("torch_faces_cut", lambda: torch_faces(True), rows_cut),
            ("planes_count_again", lambda: hops.planes_native(acc, o, nr, "count", False), rows_meet)]
    for route, fn, rows in plan:
        t = timed(torch, fn, args.warmup, args.calls)
        emit(route, t, rows=rows, rows_per_s=rows / (t["median_ms"] * 1e-3) if rows else 0.0)
        torch.cuda.empty_cache()


def cell(x):
    return f"{x['median_ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"


PAIRS = (("planes_count", "torch_count"), ("planes_count_cut", "torch_count_cut"), ("faces_on_planes", "torch_faces"),
         ("faces_on_planes_cut", "torch_faces_cut"), ("section_segments", "torch_faces_cut"))


def summary(lines, path):
    by = {}
    for ln in lines:                                  # (the last line of a route wins: the file is appended to)
        by.setdefault(ln["kind"], {})[ln["route"]] = ln
    need = {r for pair in PAIRS for r in pair} | {"planes_any", "planes_count_again"}
    if not all(k in by and all(r in by[k] for r in need) for k in KINDS):
        return False
    first = by["parallel"]["planes_count"]
    with open(path, "w") as fh:
        fh.write(f"# Plane queries against signed values, gathered signs and nonzero in torch ({first['planes']} planes, the headline mesh of "
                 f"{first['triangles']} triangles, {first['device']})\n\n")
        fh.write(f"Median ms of {first['calls']} calls (min - max) after {first['warmup']} warm-ups, each kind of planes in a process of its own.  "
                 "parallel = normal (0, 0, 1), evenly spaced over the mesh's extent along z; hashed = the same origins with hashed normals.  "
                 f"The torch route evaluates (V - o) . n in float64 for {first['chunk']} planes at a time, gathers the signs per face and lists "
                 "with nonzero; it computes no segments, so for section_segments it is a lower bound of a baseline.  Lists are count + scan + "
                 "host read + fill + ordering (+ segments).  Before the timing, with poisoned outputs: counts, offsets, faces and segments of a "
                 "subset of the planes equal the brute force bit for bit, the segments of every plane of the batch pair up end for end, and "
                 "the torch route's counts are compared with the native ones.\n\n")
        fh.write("| planes | rows met / cut | most rows of a plane | planes_any | native | torch | native / torch | checked planes | "
                 "planes whose torch count differs |\n|---|---|---|---|---|---|---|---|---|\n")
        notes = []
        for kind in KINDS:
            b = by[kind]
            for mine, theirs in PAIRS:
                m, t = b[mine], b[theirs]
                fh.write(f"| {kind} | {m['rows_meet']} / {m['rows_cut']} | {m['max_rows_of_a_plane']} | {cell(b['planes_any'])} | {mine}: {cell(m)} | "
                         f"{theirs}: {cell(t)} | {m['median_ms'] / t['median_ms']:.3f}x | {m['checked_planes']} | {m['planes_whose_torch_count_differs']} |\n")
                if m["median_ms"] >= t["median_ms"]:
                    notes.append(f"On the {kind} planes {mine} is NOT faster than {theirs} ({m['median_ms']:.3f} ms against {t['median_ms']:.3f} ms).")
            fh.write(f"| {kind} | | | | planes_count again: {cell(b['planes_count_again'])} | | | | |\n")
        fh.write("\n" + ("\n".join(notes) if notes else "Every native route is faster than the torch route on both kinds of planes.") + "\n")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=32, help="planes per chunk of the torch route")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", type=int, default=16, help="planes checked against the brute force")
    ap.add_argument("--limit", type=int, default=280, help="seconds one kind of planes may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--label", default="", help="a word kept in every line, such as the commit the run was made on")
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--step", default=None, help="(internal) run this kind of planes in this process")
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    os.makedirs(args.out, exist_ok=True)
    log = os.path.join(args.out, "r15_planes.jsonl")
    with open(log, "a") as fh:
        for kind in args.kinds.split(","):      # the parent never touches the GPU: every kind is a fresh child under its own time limit
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", kind, "--planes", str(args.planes),
                   "--chunk", str(args.chunk), "--warmup", str(args.warmup), "--calls", str(args.calls), "--check", str(args.check),
                   "--label", args.label]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            for ln in res.stdout.splitlines():
                print(ln, flush=True)
                if ln.startswith("{"):
                    fh.write(ln + "\n")
            if res.returncode != 0:
                raise SystemExit(f"the step {kind} ended with status {res.returncode}: nothing more is started")
    lines = [json.loads(ln) for ln in open(log) if ln.startswith("{")]
    if not summary(lines, os.path.join(args.out, "r15_planes_summary.md")):
        print("(no summary yet: the log does not hold every route)")


if __name__ == "__main__":
    main()
