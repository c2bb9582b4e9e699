#!/usr/bin/env python3
"""How many trips of a wave the table loop of the float top runs for tables of D = 8, 10 and 12 levels, from the host
simulation (tests/host_sim/float_top_model.cpp: the product's own tr_top_fill, tr_top_test, tr_top_build_slot beside
tr_uniform_test, tr_uniform_wave, tr_descent_step and tr_fused_step compiled with g++; no GPU).  A wave of the launch is an
8x8 pixel tile.  Every workload runs with the uniform top alone and then with the table loop in front of it, per D, and
every ray's outputs, node visits, leaf tests and lost flag and every wave's trips must be the same:
    python scripts/float_top_model.py [headline c2 c4 terrain] > profiles/r18_float_top_model.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "host_sim"), os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402

import float_top_sim as F  # noqa: E402
import sim  # noqa: E402
from descent_model import row, workload  # noqa: E402

LEVELS = (8, 10, 12)

if __name__ == "__main__":
    for name in (sys.argv[1:] or ["headline", "c2", "c4", "terrain"]):
        v, f, o, d, (h, w) = workload(name)
        B = sim.SimBVH(v, f)
        t0 = time.perf_counter()
        u = F.query(B, 2, o, d, F.UNIFORM_TOP)
        U = u["per_group"].astype(np.int64)
        n, nodes, tris = (int(x) for x in u["stats"][:3])
        print(f"{name}: {len(f)} triangles, {w}x{h} rays in 8x8 tiles, closest hit")
        print(f"  {'uniform top alone':<24} node visits {nodes}, leaf tests {tris}, lost rays {u['lost']}")
        row("  trips the uniform top runs (its last trip included)", U[:, 4])
        row("  all trips of the wave (its longest lane)", U[:, 2])
        means = {}
        for D in LEVELS:
            top = F.table(B.qnodes, D)
            present = int((top[0].view(np.int32)[:, 12:14] != 0).any(1).sum())      # a node's children are never both 0
            t = F.query(B, 2, o, d, F.FLOAT_TOP, levels=D, top=top)
            T = t["per_group"].astype(np.int64)
            n, nodes, tris = (int(x) for x in t["stats"][:3])
            same = all(u[k].tobytes() == t[k].tobytes() for k in ("hit", "front", "tri", "loc", "uv", "per_ray"))
            print(f"  D = {D}: {8 * top.shape[1] * F.REC // 1024} KiB, {present} of {top.shape[1]} slots present")
            print(f"    {'with the table loop':<22} node visits {nodes}, leaf tests {tris}, lost rays {t['lost']}")
            print(f"    outputs, node visits, leaf tests and lost flag of every ray the same: {same}")
            print(f"    trips of every wave the same (first leaf, uniform, longest lane, phase, uniform top): "
                  f"{bool(np.array_equal(U[:, :5], T[:, :5]))}")
            row("    trips the table loop runs", T[:, 6])
            means[D] = T[:, 6].mean()
            print(f"    share of the uniform top's trips: {100.0 * T[:, 6].sum() / max(1, T[:, 4].sum()):.1f} %")
        print(f"  table trips relative to D = {LEVELS[-1]}: " +
              ", ".join(f"D = {D}: {100.0 * means[D] / max(1e-9, means[LEVELS[-1]]):.1f} %" for D in LEVELS) +
              f" ({time.perf_counter() - t0:.0f} s)")
        print(flush=True)
