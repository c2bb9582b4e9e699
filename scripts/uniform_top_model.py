#!/usr/bin/env python3
"""How many trips the uniform top of wave_traverse_steal runs per wave, and how many waves its octant test turns away, from
the host simulation (tests/host_sim/uniform_top_model.cpp: the product's own tr_uniform_test, tr_uniform_wave, tr_descent_step and
tr_fused_step compiled with g++, the stealing launch wave by wave below the give-away threshold; no GPU).  A wave of the
launch is an 8x8 pixel tile.  Every workload runs twice -- descent phase + general loop, and with the uniform top in front
-- and the totals must be the same:
    python scripts/uniform_top_model.py [headline c2 c4 terrain] > profiles/r17_uniform_top_model.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "host_sim"), os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402

import sim  # noqa: E402
import uniform_top_sim as U  # noqa: E402
from descent_model import row, workload  # noqa: E402

if __name__ == "__main__":
    for name in (sys.argv[1:] or ["headline", "c2", "c4", "terrain"]):
        v, f, o, d, (h, w) = workload(name)
        B = sim.SimBVH(v, f)
        t0 = time.perf_counter()
        p = U.query(B, 2, o, d, U.PHASE)
        u = U.query(B, 2, o, d, U.UNIFORM_TOP)
        same = all(p[k].tobytes() == u[k].tobytes() for k in ("hit", "front", "tri", "loc", "uv", "per_ray"))
        print(f"{name}: {len(f)} triangles, {w}x{h} rays in 8x8 tiles, closest hit ({time.perf_counter() - t0:.0f} s)")
        for label, r in (("descent phase alone", p), ("with the uniform top", u)):
            n, nodes, tris = (int(x) for x in r["stats"][:3])
            print(f"  {label:<24} node visits {nodes}, leaf tests {tris}, lost rays {r['lost']}")
        print(f"  outputs, node visits, leaf tests and lost flag of every ray the same: {same}")
        P, G = p["per_group"].astype(np.int64), u["per_group"].astype(np.int64)
        print(f"  per wave ({len(G)} tiles)")
        row("  leading trips on which every visiting lane is at the same node", P[:, 1])
        row("  trips the uniform top runs (its last trip included)", G[:, 4])
        row("  trips the descent phase runs behind it", G[:, 3])
        row("  trips the descent phase ran alone", P[:, 3])
        row("  all trips of the wave (its longest lane)", G[:, 2])
        fail = G[:, 5] != 0
        print(f"  waves that fail the octant test: {int(fail.sum())} of {len(G)} = {100.0 * fail.mean():.1f} %"
              f" (their uniform leading trips: {P[fail, 1].mean() if fail.any() else 0.0:.2f})")
        print(f"  uniform leading trips the loop does not run: {P[:, 1].mean() - G[:, 4].mean():.2f} per wave"
              f" = {100.0 * (1.0 - G[:, 4].sum() / max(1, P[:, 1].sum())):.1f} %")
        print(f"  waves as long as they were: {bool(np.array_equal(P[:, 2], G[:, 2]))}")
        print(flush=True)
