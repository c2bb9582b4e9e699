#!/usr/bin/env python
"""triangles_nearest / mesh_distance (libtriro_tri_nearest.so) beside the two queries a caller had before them: triangles_count
on the same query triangles (the collision query: what the overlap predicate alone costs on the same walk shape) and
closest_point on the queries' vertices (three points per query: the route that is wrong whenever the nearest features are two
edges or a face interior, timed for what the right answer costs over it).  The three do not compute the same thing.

Workload: the faces of one displaced icosphere (--level: 20 * 4^level faces, seed 1) as queries against another (seed 0), at
two separations given as fractions of the extent (--shifts): a small one, where the surfaces interleave and many distances are 0,
and one beyond the extent, where every walk has to find a distant face.  Per separation: triangles_nearest without a bound and
with one (the median of the unbounded distances, so that half of the queries have no result), mesh_distance without and with
that bound, triangles_count and closest_point.

Per separation, in ONE child process under its own time limit: first the check -- with poisoned outputs (tests/poison.py) the
four outputs of a subset of the queries against the brute force over the distance function (tests/host_sim/tri_nearest_sim),
bit for bit, every output element written, and mesh_distance against the reduction of the whole batch -- then, without the
poison, --warmup warm-up calls and --calls timed ones of each route, each between two device events (median, min, max).
mesh_distance is timed with a host clock around a call that ends in a device synchronise.  A step that fails or runs out of time
ends the run.  Nothing in the tests depends on these numbers.

Appends one JSON line per (separation, route) to <out>/tri_nearest.jsonl (default: profiles/) and prints a table."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_boxes import cell, timed, timed_host  # noqa: E402  (the same clocks as the other satellite tables)


def step(args):
    """one separation, every route, in this process; prints one JSON line per route"""
    for p in (ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "host_sim")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import workloads as W
    import poison
    import tri_nearest_sim
    import triro.backend.ops as hops
    from triro.ray.ray_optix import RayMeshIntersector
    if not torch.cuda.is_available():
        raise SystemExit("bench_tri_nearest.py needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    v0, f = W.icosphere(args.level)
    v, other = W.displaced(v0, seed=0, amplitude=0.08), W.displaced(v0, seed=1, amplitude=0.08)
    ext = float((v.max(0).astype(np.float64) - v.min(0)).max())
    shift = float(args.step)
    other = (other + (np.float64(shift * ext) * np.array([2, -1, 2]) / 3).astype(np.float32)).astype(np.float32)
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    ot = torch.from_numpy(other).to(dev)
    mesh = RayMeshIntersector(vertices=vt, faces=ft)
    acc = mesh.as_wrapper
    tri = ot[ft.long()].contiguous()
    points = tri.reshape(-1, 3).contiguous()
    n = int(len(f))
    common = dict(shift=shift, queries=n, triangles=n, warmup=args.warmup, calls=args.calls, device=torch.cuda.get_device_name(0),
                  label=args.label)

    def emit(route, t, **more):
        print(json.dumps(dict(route=route, **t, **more, **common)), flush=True)

    # the check
    hops.get_tri_nearest_module()
    poison.install()
    face, distance, on_mesh, on_query = hops.triangles_nearest_native(acc, tri)
    torch.cuda.synchronize()
    poison.assert_written(face, distance, on_mesh, on_query, what="triangles_nearest_native")
    bound = float(distance.median())
    pick = torch.arange(0, n, max(1, n // args.check), device=dev)[: args.check]
    got = hops.triangles_nearest_native(acc, tri[pick].contiguous())
    within = hops.triangles_nearest_native(acc, tri[pick].contiguous(), bound)
    torch.cuda.synchronize()
    poison.assert_written(*got, *within, what="triangles_nearest_native (subset)")
    for res, md in ((got, None), (within, bound)):
        want = tri_nearest_sim.brute(v, f, tri[pick].cpu().numpy(), md)
        assert np.array_equal(res[0].cpu().numpy(), want[0])
        for g, w in zip(res[1:], want[1:]):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))
    d = distance.cpu().numpy()
    k = int(np.flatnonzero(d == d.min())[0])
    whole = mesh.mesh_distance(ot, ft)
    assert float(whole[0]) == d[k] and int(whole[1]) == k and int(whole[2]) == int(face[k])
    chunked = mesh.mesh_distance(ot, ft, chunk=max(1, n // 7))
    assert all(torch.equal(a, b) for a, b in zip(whole[:3], chunked[:3]))
    poison.uninstall()
    common.update(checked_queries=int(len(pick)), zero_fraction=float((distance == 0).double().mean()), median_distance=bound,
                  least_distance=float(whole[0]))
    del got, within, face, distance, on_mesh, on_query
    torch.cuda.empty_cache()

    plan = [("triangles_nearest", lambda: hops.triangles_nearest_native(acc, tri)),
            ("triangles_nearest_bounded", lambda: hops.triangles_nearest_native(acc, tri, bound)),
            ("triangles_nearest_distance_only", lambda: hops.triangles_nearest_native(acc, tri, None, 0, (True, False, False))),
            ("triangles_count", lambda: hops.tris_native(acc, tri, "count")),
            ("closest_point_on_vertices", lambda: hops.closest_point_native(acc, points)),
            ("triangles_nearest_again", lambda: hops.triangles_nearest_native(acc, tri))]
    for route, fn in plan:
        t = timed(torch, fn, args.warmup, args.calls)
        emit(route, t, queries_per_s=n / (t["median_ms"] * 1e-3))
        torch.cuda.empty_cache()
    for route, fn in (("mesh_distance", lambda: mesh.mesh_distance(ot, ft)), ("mesh_distance_bounded", lambda: mesh.mesh_distance(ot, ft, bound)),
                      ("mesh_distance_8_chunks", lambda: mesh.mesh_distance(ot, ft, chunk=-(-n // 8)))):
        emit(route, timed_host(torch, fn, 1, args.calls))


def table(lines):
    by = {}
    for ln in lines:                                  # (the last line of a route wins: the file is appended to)
        by.setdefault(ln["shift"], {})[ln["route"]] = ln
    for shift, b in sorted(by.items()):
        first = next(iter(b.values()))
        print(f"\nshift {shift:g} of the extent: {first['queries']} query faces against {first['triangles']} ({first['device']}); distance 0 for "
              f"{first['zero_fraction']:.1%} of the queries, median {first['median_distance']:.4g}, least {first['least_distance']:.4g}; median ms "
              f"of {first['calls']} calls (min - max); {first['checked_queries']} queries checked against the brute force")
        for route, ln in b.items():
            print(f"  {route:34s} {cell(ln)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=7, help="subdivisions of the icospheres: 20 * 4^level faces each")
    ap.add_argument("--shifts", default="0.01,1.25", help="the separations, as fractions of the extent")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--check", type=int, default=32, help="queries checked against the brute force")
    ap.add_argument("--limit", type=int, default=170, help="seconds one separation may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--label", default="", help="a word kept in every line, such as the commit the run was made on")
    ap.add_argument("--step", default=None, help="(internal) run this separation in this process")
    args = ap.parse_args()
    if args.step is not None:
        return step(args)
    os.makedirs(args.out, exist_ok=True)
    log = os.path.join(args.out, "tri_nearest.jsonl")
    with open(log, "a") as fh:
        for shift in args.shifts.split(","):      # the parent never touches the GPU: every separation is a fresh child under its own time limit
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", shift, "--level", str(args.level),
                   "--warmup", str(args.warmup), "--calls", str(args.calls), "--check", str(args.check), "--label", args.label]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            for ln in res.stdout.splitlines():
                print(ln, flush=True)
                if ln.startswith("{"):
                    fh.write(ln + "\n")
            if res.returncode != 0:
                raise SystemExit(f"the separation {shift} ended with status {res.returncode}: nothing more is started")
    table([json.loads(ln) for ln in open(log) if ln.startswith("{")])


if __name__ == "__main__":
    main()
