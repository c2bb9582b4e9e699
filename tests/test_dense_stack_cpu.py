"""The dense far-child stack of the fused trip (tr_bvh.h: tr_push_far / tr_pop_far / tr_bottom_slot), on the host simulation.

Far children are kept in rank order in the 16 LDS words of a lane instead of at depth % 16.  Checked here: results stay
the oracle's bit for bit on every schedule; on the headline workload the climbs vanish while node visits and leaf tests
are exactly those of the commit before (the walk is the same, only where owed children are kept changed); a ray that owes
more far children at once than the stack holds falls back to the climb and still gets the oracle's answer; and the
stealing launches' hand-over, which the ray-by-ray simulation never performs, agrees with a plain vector."""
import numpy as np
import pytest

import sim
import workloads as W
from oracle.oracle import OracleIntersector
from sim import SimBVH

Q_ANY, Q_FIRST, Q_CLOSEST, Q_COUNT = 0, 1, 2, 3


def _flat(o, d):
    o = np.ascontiguousarray(np.broadcast_to(o, np.shape(d)), np.float32).reshape(-1, 3)
    return o, np.ascontiguousarray(d, np.float32).reshape(-1, 3)


def _headline_rays(v, res):
    return _flat(*W.pinhole_grid(res, res, distance=2.5 * float(np.linalg.norm(v, axis=1).max())))


def _expected(v, f, o, d):
    R = OracleIntersector(v, f, 1)
    h, fr, tri, loc, uv, _ = R.closest_raw(o, d)
    return dict(hit=h.ravel(), front=fr.ravel(), tri=tri.ravel(), loc=loc.reshape(-1, 3), uv=uv.reshape(-1, 2),
                count=R.intersects_count(o, d).ravel())


def _check(B, o, d, want, queries=(Q_CLOSEST, Q_FIRST, Q_ANY, Q_COUNT)):
    """the four queries through whatever schedule sim is set to; returns the closest query's counters"""
    stats = None
    for q in queries:
        r = B.query(q, o, d)
        if q == Q_CLOSEST:
            stats = [int(x) for x in r["stats"]]
            assert np.array_equal(r["hit"], want["hit"]) and np.array_equal(r["front"], want["front"])
            assert np.array_equal(r["tri"], want["tri"])
            assert np.array_equal(r["loc"], want["loc"]) and np.array_equal(r["uv"], want["uv"])
        elif q == Q_FIRST:
            assert np.array_equal(r["tri"], want["tri"])
        elif q == Q_ANY:
            assert np.array_equal(r["hit"], want["count"] > 0)
        else:
            assert np.array_equal(r["count"], want["count"])
    return stats


def _scenes():
    for sub in (6, 7):
        v, f = W.headline_mesh(sub)
        yield f"headline({sub})", v, f, [_headline_rays(v, 256), _headline_rays(v, 512)]
    v, f = W.nested_shells()                              # C4
    yield "shells", v, f, [_flat(*W.pinhole_grid(256, 256))]
    v, f = W.terrain()
    yield "terrain", v, f, [_flat(*W.ref_shape_rays(W.TERRAIN_EYE, W.TERRAIN_TARGET, 256, 144, 444.0 * 256 / 640))]


@pytest.mark.parametrize("scene", ["headline(6)", "headline(7)", "shells", "terrain"])
def test_every_schedule_returns_the_oracles_results(scene):
    """closest / first / any / count, stack on and off, fused modes 1, 2 and 2|4 (a hierarchy of more than 32 levels cannot
    run the 32-bit state: it takes 1 and 1|4)"""
    name, v, f, batches = next(s for s in _scenes() if s[0] == scene)
    B = SimBVH(v, f)
    modes = (1, 2, 6) if B.depth <= 32 else (1, 5)
    try:
        for o, d in batches:
            want = _expected(v, f, o, d)
            for ring in (True, False):
                sim.use_ring(ring)
                for mode in modes:
                    sim.use_fused(mode)
                    _check(B, o, d, want)
            sim.use_ring(True)
            sim.use_fused(0)
            sim.use_unordered(True)                       # any / count through the unordered schedule (its ring is depth-indexed)
            _check(B, o, d, want, queries=(Q_ANY, Q_COUNT))
            sim.use_unordered(False)
    finally:
        sim.use_ring(True)
        sim.use_fused(0)
        sim.use_unordered(False)


# Totals of the commit BEFORE the dense stack (depth-indexed ring of 16 nodes, no entry distances), from
# `python scripts/host_sim_stack_stats.py` run on that commit: headline_mesh(8), 1024 x 1024 pinhole rays at 2.5 radii,
# closest through use_fused(2 | 4) -- 35.7625 node visits, 2.8242 leaf tests, 3.0155 climbs per ray.
PARENT_RAYS, PARENT_NODES, PARENT_TRIS, PARENT_CLIMBS = 1 << 20, 37499751, 2961392, 3162006


def test_headline_counters_against_the_commit_before():
    """The issue also asks for FEWER node visits (entries beyond the cull limit dropped at the pop, from a stored entry
    distance).  That part was built and measured slower on the GPU than the stack without it (DESIGN_experiments.md part
    R7: headline 0.168 against 0.150 ms) and is not shipped: the visits are pinned as EQUAL to the commit before."""
    v, f = W.headline_mesh(8)
    o, d = _headline_rays(v, 1024)
    B = SimBVH(v, f)
    sim.use_fused(2 | 4)
    try:
        n, nodes, tris, climbs = (int(x) for x in B.query(Q_CLOSEST, o, d)["stats"])
    finally:
        sim.use_fused(0)
    print(f"rays {n}: node visits {nodes} (before {PARENT_NODES}), leaf tests {tris} (before {PARENT_TRIS}), "
          f"climbs {climbs} ({climbs / n:.4f} per ray; before {PARENT_CLIMBS / n:.4f})")
    assert n == PARENT_RAYS
    assert tris == PARENT_TRIS and nodes == PARENT_NODES
    assert climbs * 20 <= PARENT_CLIMBS
    assert climbs == 0                                  # a ray of this batch owes 13 far children at most, the stack holds 16


def test_a_ray_that_owes_more_than_the_stack_holds_climbs_and_is_still_right():
    """A soup of 30 000 triangles as large as the scene: nearly every box is hit, the hierarchy is 22 levels deep, and rays
    owe more than sixteen far children at once.  With the 64-bit and the 32-bit state, on the grid nodes and on the exact
    ones, the walk must overflow (climbs > 0 with the stack ON) and still return the oracle's results for every query."""
    v, f = W.random_soup(30000, seed=8, size=1.5)
    o, d = W.hash_rays(3000, 4, v.min(0) * 1.5, v.max(0) * 1.5)
    B = SimBVH(v, f)
    assert 16 < B.depth <= 32
    want = _expected(v, f, o, d)
    try:
        for mode in (1 | 4, 1, 2 | 4, 2):
            sim.use_fused(mode)
            st = _check(B, o, d, want)
            assert st[3] > 0, f"no push found the 16-slot stack full (mode {mode}): the scene does not exercise the overflow"
    finally:
        sim.use_fused(0)


@pytest.mark.parametrize("bits", [32, 64])
def test_stack_with_hand_overs_against_a_plain_vector(bits, tmp_path):
    """What the ray-by-ray simulation never does: the stealing launches' hand-over (tr_bottom_slot: the shallowest entry
    leaves, its owned bit stays as a ghost, slots wrap mod 16).  tests/host_sim/stack_model.cpp drives tr_push_far /
    tr_pop_far / tr_bottom_slot with random pushes, descents, pops and hand-overs against a vector of owed entries:
    every pop and hand-over must return the vector's entry, and the sequence must have reached the corners -- full
    stacks, wrapped slots, a ghost above an entry that was never recorded."""
    import ctypes as C
    import os
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
    so = str(tmp_path / "libstack_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma",
                           "-Wno-unknown-pragmas", "-o", so, os.path.join(here, "stack_model.cpp")])
    L = C.CDLL(so)
    L.stack_model.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_void_p]
    tot = np.zeros(8, np.int64)
    for seed in range(1, 9):
        out = np.zeros(8, np.int64)
        L.stack_model(bits, seed, 400_000, out.ctypes.data)
        assert out[0] == 0, (seed, out)
        tot += out
    print(dict(zip(("mismatches", "recorded", "onto_full", "hand_overs", "wrapped", "ghost_above_unrecorded", "from_stack"),
                   tot.tolist())))
    assert all(tot[k] > 0 for k in (1, 2, 3, 4, 5, 6))
