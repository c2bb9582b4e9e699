"""The plain far-child stack of the stealing closest / first / any launch on the grid nodes (tr_bvh.h: tr_plain_push /
tr_plain_pop / tr_plain_give, the walk selected by tr_plain_w), on the host simulation (tests/host_sim/plain_sim.py).

The walk keeps owed far children on a stack with a stack pointer: no trail, no owned word, no depth.  Checked here: on
the headline workload it visits exactly the nodes and tests exactly the leaves of the dense stack and loses nothing; a ray
that owes more far children at once than the stack holds is flagged, traversed a second time by the stackless walk and
still gets the oracle's answer; and the hand-over of the stealing launch, which the ray-by-ray simulation never performs,
agrees with a plain vector."""
import numpy as np

import plain_sim
import workloads as W
from oracle.oracle import OracleIntersector
from sim import SimBVH

Q_ANY, Q_FIRST, Q_CLOSEST = 0, 1, 2

# the dense stack's totals on the headline (tests/test_dense_stack_cpu.py pins the same two against the commit before it)
HEADLINE_RAYS, HEADLINE_NODES, HEADLINE_TRIS = 1 << 20, 37499751, 2961392


def _flat(o, d):
    o = np.ascontiguousarray(np.broadcast_to(o, np.shape(d)), np.float32).reshape(-1, 3)
    return o, np.ascontiguousarray(d, np.float32).reshape(-1, 3)


def _check(B, o, d, closest, count):
    """closest / first / any through the plain walk against the oracle -> (closest's counters, lost rays per query)"""
    stats, lost = None, {}
    for q in (Q_CLOSEST, Q_FIRST, Q_ANY):
        r = plain_sim.query(B, q, o, d)
        lost[q] = r["lost"]
        if q == Q_CLOSEST:
            stats = [int(x) for x in r["stats"]]
            for key, want in zip(("hit", "front", "tri", "loc", "uv"), closest):
                assert np.array_equal(r[key], want.reshape(r[key].shape)), f"closest {key}"
        elif q == Q_FIRST:
            assert np.array_equal(r["tri"], closest[2].ravel())
        else:
            assert np.array_equal(r["hit"], count > 0)
    return stats, lost


def test_headline_visits_what_the_dense_stack_visits_and_loses_nothing():
    v, f = W.headline_mesh(8)
    o, d = _flat(*W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max())))
    R = OracleIntersector(v, f, 1)
    closest = R.closest_raw(o, d)[:5]
    B = SimBVH(v, f)
    r = plain_sim.query(B, Q_CLOSEST, o, d)
    lost = r["lost"]
    n, nodes, tris, climbs = (int(x) for x in r["stats"])
    print(f"rays {n}: node visits {nodes}, leaf tests {tris}, lost rays {lost}, climbs {climbs}")
    assert n == HEADLINE_RAYS
    assert nodes == HEADLINE_NODES and tris == HEADLINE_TRIS
    assert lost == 0 and climbs == 0
    for key, want in zip(("hit", "front", "tri", "loc", "uv"), closest):
        assert np.array_equal(r[key], want.reshape(r[key].shape)), f"closest {key}"


def test_a_ray_that_owes_more_than_the_stack_holds_is_traversed_again_and_is_still_right():
    """The overflow scene of tests/test_dense_stack_cpu.py: a soup of 30 000 triangles as large as the scene, rays that owe
    more than sixteen far children at once.  The plain walk must lose children here (or the scene does not exercise the
    second traversal) and closest / first / any must still be the oracle's."""
    v, f = W.random_soup(30000, seed=8, size=1.5)
    o, d = W.hash_rays(3000, 4, v.min(0) * 1.5, v.max(0) * 1.5)
    B = SimBVH(v, f)
    assert 16 < B.depth <= 32
    R = OracleIntersector(v, f, 1)
    closest, count = R.closest_raw(o, d)[:5], R.intersects_count(o, d).ravel()
    stats, lost = _check(B, o, d, closest, count)
    print(f"lost rays of {len(o)}: closest {lost[Q_CLOSEST]}, first {lost[Q_FIRST]}, any {lost[Q_ANY]}; climbs of the second traversals {stats[3]}")
    assert lost[Q_CLOSEST] > 0 and lost[Q_FIRST] > 0 and lost[Q_ANY] > 0, "no push found the stack full: the scene does not exercise the overflow"
    assert stats[3] > 0                                   # the second traversal is the stackless one: it climbs


def test_the_other_scene_families_through_the_plain_walk():
    """nested shells (rays that cross twelve surfaces) and the terrain (a camera inside the mesh's box), as
    tests/test_dense_stack_cpu.py runs them through the dense stack"""
    scenes = ((W.nested_shells(), _flat(*W.pinhole_grid(128, 128))),
              (W.terrain(), _flat(*W.ref_shape_rays(W.TERRAIN_EYE, W.TERRAIN_TARGET, 128, 72, 444.0 * 128 / 640))))
    for (v, f), (o, d) in scenes:
        R = OracleIntersector(v, f, 1)
        _check(SimBVH(v, f), o, d, R.closest_raw(o, d)[:5], R.intersects_count(o, d).ravel())


def test_stack_with_hand_overs_against_a_plain_vector(tmp_path):
    """tests/host_sim/plain_stack_model.cpp drives tr_plain_push / tr_plain_pop / tr_plain_give with random pushes, pops
    and hand-overs against a vector of owed entries: every pop and hand-over must return the vector's entry, a push must be
    lost exactly when the slots are used up, and the sequence must have reached the corners -- pushes onto sixteen live
    entries, pushes that did not fit because of slots given away, pops interleaved with hand-overs, walks that end on a
    given-away slot."""
    import ctypes as C
    import os
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
    so = str(tmp_path / "libplain_stack_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma",
                           "-Wno-unknown-pragmas", "-o", so, os.path.join(here, "plain_stack_model.cpp")])
    L = C.CDLL(so)
    L.plain_stack_model.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
    tot = np.zeros(10, np.int64)
    for seed in range(1, 9):
        out = np.zeros(10, np.int64)
        L.plain_stack_model(seed, 400_000, out.ctypes.data)
        assert out[0] == 0, (seed, out)
        tot += out
    print(dict(zip(("mismatches", "recorded", "onto_16_live", "short_by_gifts", "hand_overs", "from_stack", "pops_after_hand_over",
                    "ended_on_given_slot", "ended_empty", "ended_lost"), tot.tolist())))
    assert all(tot[k] > 0 for k in range(1, 10))
