#!/usr/bin/env python3
"""How many of a wave's trips come before its first leaf, from the host simulation (tests/host_sim/descent_model.cpp: the
product's own tr_descent_step and tr_fused_step compiled with g++, the stealing launch wave by wave below the give-away
threshold; no GPU).  A wave of the launch is an 8x8 pixel tile.  Every workload runs twice -- the general loop alone and
with the descent phase in front -- and the totals must be the same:
    python scripts/descent_model.py [headline c2 c4 terrain] > profiles/r11_descent_model.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "host_sim")]
import numpy as np  # noqa: E402

import descent_sim as D  # noqa: E402
import sim  # noqa: E402
import workloads as W  # noqa: E402


def tile_order(h, w):
    """ray indices of a row-major h x w image, 8x8 tile after 8x8 tile"""
    return np.arange(h * w).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)


def workload(name):
    if name == "headline":
        v, f = W.headline_mesh(8)
        o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    elif name == "c2":
        v, f, _ = W.bunny_mesh()
        o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    elif name == "c4":
        v, f = W.nested_shells(7)
        o, d = W.pinhole_grid(1024, 1024)
    elif name == "terrain":
        v, f = W.terrain()
        _, d = W.ref_shape_rays(W.TERRAIN_EYE, W.TERRAIN_TARGET, 1024, 576, 444.0 * 1024 / 640)
        o = np.array(W.TERRAIN_EYE, np.float32)
    else:
        raise SystemExit(f"unknown workload {name}")
    d = np.ascontiguousarray(d, np.float32)
    h, w = d.shape[:2]
    o = np.ascontiguousarray(np.broadcast_to(o, d.shape), np.float32).reshape(-1, 3)
    k = tile_order(h, w)
    return v, f, o[k], d.reshape(-1, 3)[k], (h, w)


def row(label, a):
    a = np.asarray(a, np.float64)
    print(f"{label:<72}{a.mean():7.2f}  median {np.median(a):5.1f}  p10 / p90 {np.percentile(a, 10):5.1f} / {np.percentile(a, 90):5.1f}")


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["headline", "c2", "c4", "terrain"]):
        v, f, o, d, (h, w) = workload(name)
        B = sim.SimBVH(v, f)
        t0 = time.perf_counter()
        g = D.query(B, 2, o, d, D.GENERAL)
        p = D.query(B, 2, o, d, D.DESCENT)
        same = all(g[k].tobytes() == p[k].tobytes() for k in ("hit", "front", "tri", "loc", "uv", "per_ray"))
        print(f"{name}: {len(f)} triangles, {w}x{h} rays in 8x8 tiles, closest hit ({time.perf_counter() - t0:.0f} s)")
        for label, r in (("general loop alone", g), ("with the descent phase", p)):
            n, nodes, tris = (int(x) for x in r["stats"][:3])
            print(f"  {label:<24} node visits {nodes}, leaf tests {tris}, lost rays {r['lost']}")
        print(f"  outputs, node visits, leaf tests and lost flag of every ray the same: {same}")
        G, P = g["per_group"].astype(np.int64), p["per_group"].astype(np.int64)
        print(f"  per wave ({len(G)} tiles)")
        first = np.where(G[:, 0] > 0, G[:, 0] - 1, G[:, 2])      # a wave that never has a leaf: all its trips
        row("  leading trips before any lane's box test accepts a leaf child", first)
        row("  ... of which every visiting lane is at the same node (from the root on)", G[:, 1])
        row("  all trips of the wave (its longest lane)", G[:, 2])
        row("  trips the descent phase runs (the trip that accepts the leaf included)", P[:, 3])
        print(f"  share of the wave trips that the phase runs: {100.0 * P[:, 3].sum() / G[:, 2].sum():.1f} %")
        print(flush=True)
