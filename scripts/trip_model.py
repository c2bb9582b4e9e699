#!/usr/bin/env python3
"""Where the trips of the headline launch go, from the host simulation (tests/host_sim/trip_model.cpp: the product's own
tr_bvh.h compiled with g++, the stealing trip's schedule ray by ray; no GPU).  A wave of the launch is an 8x8 pixel tile
and lasts as long as its longest lane (below the give-away threshold nothing moves between lanes), so per-ray trip
counters folded into tiles give the wave's trips:
    python scripts/trip_model.py [subdivisions=8] [resolution=1024] > profiles/r10_trip_model.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "host_sim")]
import numpy as np  # noqa: E402

import sim  # noqa: E402
import trip_sim  # noqa: E402
import workloads as W  # noqa: E402


def tiles(a, res):
    """(res * res,) per-ray values of a row-major image -> (tiles, 64)"""
    return a.reshape(res // 8, 8, res // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


if __name__ == "__main__":
    subdiv = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    res = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    v, f = W.headline_mesh(subdiv)
    o, d = W.pinhole_grid(res, res, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    o = np.ascontiguousarray(np.broadcast_to(o, d.shape)).reshape(-1, 3)
    d = d.reshape(-1, 3)
    B = sim.SimBVH(v, f)
    t0 = time.perf_counter()
    r = trip_sim.query(B, 2, o, d, per_ray=True)
    n, nodes, tris, climbs = (int(x) for x in r["stats"])
    p = r["per_ray"].astype(np.int64)
    trips, visits, stalls, leaf_only, first, ent = (p[:, k] for k in range(6))
    print(f"headline_mesh({subdiv}): {len(f)} triangles, {res}x{res} pinhole rays, closest hit through the address form "
          f"({time.perf_counter() - t0:.0f} s)")
    print(f"node visits {nodes}, leaf tests {tris}, lost rays {r['lost']}, climbs {climbs}")
    T = tiles(trips, res)
    longest = T.max(1)
    arg = T.argmax(1)
    hitm = first > 0
    print(f"tiles (8x8)                                              {len(T)}")
    print(f"mean over the tiles of the longest lane's trips          {longest.mean():.2f}")
    print(f"mean trips per ray                                       {trips.mean():.2f}")
    print(f"mean node visits per ray                                 {visits.mean():.2f}")
    print(f"lane-trips that do something                             {100.0 * T.sum() / (64.0 * longest.sum()):.1f} %")
    print(f"trips a lane loses to a full leaf FIFO / the alternation {stalls.mean():.2f} per ray")
    print(f"trips with only queued leaves left                       {leaf_only.mean():.2f} per ray")
    print(f"rays with a hit                                          {int(hitm.sum())}")
    print(f"trip at which a ray finds its first hit (rays with one)  {first[hitm].mean():.2f} of {trips[hitm].mean():.2f}")
    print(f"trips after the first hit                                {(trips[hitm] - first[hitm]).mean():.2f}")
    print(f"stack entries at the first hit                           {ent[hitm].mean():.2f}")
    F = tiles(first, res)
    lf = F[np.arange(len(T)), arg]
    hl = lf > 0
    print(f"longest lane of a tile: first hit at trip / its trips    {lf[hl].mean():.2f} / {longest[hl].mean():.2f} ({int(hl.sum())} tiles whose longest lane hits)")
    # Optimistic bound for "idle lanes take subtrees only from rays that already have a hit": what a ray does up to its
    # first hit stays on its lane (a ray without a hit gives nothing away), everything after it is spread over the
    # wave's 64 lanes without loss and without the cost of the looks.
    own = np.where(F > 0, F, T)
    bound = np.maximum(own.max(1), np.ceil(T.sum(1) / 64.0))
    print(f"bound, work after a first hit shared perfectly           {bound.mean():.2f} against {longest.mean():.2f} "
          f"({100.0 * (bound.mean() / longest.mean() - 1.0):+.1f} % wave trips)")
