#!/usr/bin/env python3
"""Traversal counters of the HEADLINE workload from the host simulation (tests/host_sim: the product's own
tr_bvh.h compiled with g++; no GPU): node visits, leaf tests and links[] loads spent climbing, per ray and in total,
for the closest-hit query as the stealing launch walks it (fused trip, 32-bit state, 32-byte grid nodes: use_fused(2 | 4))
and for count through the unordered schedule.  These are the totals tests/test_dense_stack_cpu.py pins for the
commit BEFORE the dense far-child stack; run on any tree to compare:
    python scripts/host_sim_stack_stats.py [subdivisions=8] [resolution=1024] > profiles/r07_dense_stack_host_sim.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "host_sim")]
import numpy as np  # noqa: E402

import sim  # noqa: E402
import workloads as W  # noqa: E402

Q_ANY, Q_FIRST, Q_CLOSEST, Q_COUNT = 0, 1, 2, 3


def headline(subdiv=8, res=1024):
    v, f = W.headline_mesh(subdiv)
    o, d = W.pinhole_grid(res, res, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    o = np.ascontiguousarray(np.broadcast_to(o, d.shape)).reshape(-1, 3)
    return v, f, o, d.reshape(-1, 3)


def counters(B, q, o, d, fused, unordered=False, ring=True):
    sim.use_fused(fused)
    sim.use_unordered(unordered)
    sim.use_ring(ring)
    try:
        st = B.query(q, o, d)["stats"]
    finally:
        sim.use_fused(0)
        sim.use_unordered(False)
        sim.use_ring(True)
    return [int(x) for x in st]      # rays, node visits, leaf tests, climbs


if __name__ == "__main__":
    subdiv = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    res = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    v, f, o, d = headline(subdiv, res)
    t0 = time.perf_counter()
    B = sim.SimBVH(v, f)
    print(f"headline_mesh({subdiv}): {len(f)} triangles, hierarchy {B.depth} levels, {res}x{res} pinhole rays "
          f"(build {time.perf_counter() - t0:.1f} s)")
    print(f"{'query / schedule':58s} {'node visits':>14s} {'leaf tests':>12s} {'climbs':>10s}   per ray")
    for name, q, fused, unordered, ring in (
            ("closest, fused trip, grid nodes, 32-bit state (2|4)", Q_CLOSEST, 6, False, True),
            ("closest, the same without the LDS stack", Q_CLOSEST, 6, False, False),
            ("first, fused trip, grid nodes, 32-bit state (2|4)", Q_FIRST, 6, False, True),
            ("closest, fused trip, exact nodes, 32-bit state (2)", Q_CLOSEST, 2, False, True),
            ("count, unordered schedule", Q_COUNT, 0, True, True),
            ("any, unordered schedule", Q_ANY, 0, True, True)):
        n, nodes, tris, climbs = counters(B, q, o, d, fused, unordered, ring)
        print(f"{name:58s} {nodes:14d} {tris:12d} {climbs:10d}   {nodes / n:.4f} / {tris / n:.4f} / {climbs / n:.4f}")
