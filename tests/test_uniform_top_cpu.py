"""The uniform top of the stealing grid-node launch (kernels_direct.inc: wave_traverse_steal; tr_bvh.h: tr_uniform_test,
tr_uniform_wave): while every visiting lane of a wave is at one node and all its rays point into one octant, the record is
read once for the wave and what depends on record and octant alone is done once.  The loop must change NOTHING: every lane
visits the nodes it visited before, in the same trips, and the descent phase and the general loop take over in the state they
would have reached by themselves.

Checked here, on the host (tests/host_sim/uniform_top_model.cpp: the product's own tr_uniform_test, tr_uniform_wave,
tr_descent_step and tr_fused_step, rays in groups of 64 with the wave's entry test and exit rules): loop + phase + general
loop against phase + general loop, wave by wave -- every output bit for bit, and node visits, leaf tests and the lost flag
per ray.  And that the comparison has bite: two deliberately wrong loops inside the model (no octant test; going on after the
lanes' next nodes differ) are reported.  The inputs are those of tests/test_gpu_uniform_top.py (tests/uniform_top_cases.py)."""
import numpy as np
import pytest

import uniform_top_cases as C
import uniform_top_sim as U
from oracle.oracle import OracleIntersector
from sim import SimBVH

Q_ANY, Q_FIRST, Q_CLOSEST = 0, 1, 2
QUERIES = (Q_ANY, Q_FIRST, Q_CLOSEST)
OUTPUTS = {Q_ANY: ("hit",), Q_FIRST: ("tri",), Q_CLOSEST: ("hit", "front", "tri", "loc", "uv")}
FIRST_LEAF, UNIFORM, LONGEST, PHASE, LOOP, OCTANT_FAIL = range(6)      # columns of per_group (U.PER_GROUP)

_SCENES = {}


def scene(case):
    """the case's mesh, its hierarchy and its rays, built once"""
    if case not in _SCENES:
        v, f, o, d = C.CASES[case]()
        _SCENES[case] = (v, f, SimBVH(v, f), o, d)
    return _SCENES[case]


def differences(q, a, b):
    """what differs between two runs of the model: names of outputs (compared as bytes: a NaN or a -0.0 counts), and the
    per-ray counters"""
    bad = [k for k in OUTPUTS[q] if a[k].tobytes() != b[k].tobytes()]
    for j, name in enumerate(U.PER_RAY):
        if not np.array_equal(a["per_ray"][:, j], b["per_ray"][:, j]):
            bad.append(name)
    return bad


def same_through_the_loop(B, o, d, steal_min=U.STEAL_MIN, queries=QUERIES):
    """phase + general loop against loop + phase + general loop, for every query; returns the closest-hit pair of runs"""
    pair = None
    for q in queries:
        p = U.query(B, q, o, d, U.PHASE, steal_min)
        u = U.query(B, q, o, d, U.UNIFORM_TOP, steal_min)
        assert differences(q, p, u) == [], (q, differences(q, p, u))
        assert p["lost"] == u["lost"]
        # the waves are as long as they were, their first leaf comes on the trip it came on, and the loop's trips are trips
        # the phase no longer runs
        assert np.array_equal(p["per_group"][:, :3], u["per_group"][:, :3]), q
        assert np.array_equal(u["per_group"][:, LOOP] + u["per_group"][:, PHASE], p["per_group"][:, PHASE]), q
        assert (u["per_group"][:, LOOP] <= p["per_group"][:, UNIFORM]).all(), q      # never past the uniform trips
        if q == Q_CLOSEST:
            pair = (p, u)
    return pair


@pytest.mark.parametrize("case", list(C.CASES))
def test_the_loop_changes_nothing(case):
    v, f, B, o, d = scene(case)
    p, u = same_through_the_loop(B, o, d)
    G = u["per_group"]
    if case == "one triangle":
        assert (G[:, LOOP] == 0).all() and not u["hit"].any()      # no hierarchy: nothing is walked
        return
    want = OracleIntersector(v, f, 1).closest_raw(o, d)[:5]
    for key, w in zip(OUTPUTS[Q_CLOSEST], want):
        assert np.array_equal(u[key], w.reshape(u[key].shape)), key
    if case == "two triangles":
        assert u["hit"][:128].any() and (G[:, LOOP] == 1).all() and (G[:, PHASE] == 0).all()      # a leaf child at the root: trip 1
    if case == "three triangles":
        assert u["hit"][128:].any()
        # the waves at the pair: on trip 1 the lanes beside the pair's box have no child, so the loop ends and the phase takes
        # trip 2; the waves at the single triangle: the root's leaf child ends both on trip 1
        assert G[:, LOOP].tolist() == [1, 1, 1, 1] and G[:, PHASE].tolist() == [1, 1, 0, 0]
    if case == "sphere from outside":
        assert u["hit"].any() and not u["hit"].all()
        assert G[:, LOOP].mean() > 3 and (G[:, PHASE] > 0).any()      # the loop runs, and hands over to the phase
    if case == "sphere from inside":
        assert u["hit"].all() and G[:32, OCTANT_FAIL].all() and (G[32:, OCTANT_FAIL] == 0).any()
    if case == "64 identical rays":
        # uniform down to the trip that accepts the leaf: the loop runs them all and the phase none
        assert u["hit"].all() and G[0, LOOP] == G[0, FIRST_LEAF] > 4 and G[0, PHASE] == 0
    if case == "one 8 x 8 tile":
        assert G[0, OCTANT_FAIL] == 0 and G[0, LOOP] > 1 and u["hit"].any()
    if case == "lane 0 invalid":
        assert not u["hit"][0::64].any() and not u["hit"][1::64].any() and not u["hit"][64:67].any() and u["hit"].any()
        assert (G[:, LOOP] > 0).all() and (G[:, OCTANT_FAIL] == 0).all()
    if case == "rays that miss the root box":
        assert not u["hit"].any() and (u["per_ray"][:, 0] == 1).all()
        assert (G[:, LOOP] == 1).all() and (G[:, PHASE] == 0).all()      # the root's visit: every lane would pop, and nobody has a node
    if case == "mixed octants":
        assert G[0, OCTANT_FAIL] == 1 and G[0, LOOP] == 0 and G[0, PHASE] == p["per_group"][0, PHASE] > 0 and u["hit"].any()
    if case.startswith("one lane leaves at trip"):
        k = int(case.split()[-1])
        assert G[0, OCTANT_FAIL] == 0 and G[0, LOOP] == k and G[0, PHASE] == G[0, FIRST_LEAF] - k > 0
    if case == "4096 hash rays":
        assert u["hit"].any() and G[:, OCTANT_FAIL].mean() > 0.9      # unrelated rays fall out at the entry test
    if case == "dense soup":
        assert u["lost"] > 0, "no ray lost a far child: the input does not reach the case"
        assert (G[:, FIRST_LEAF] > 17).all()                         # the stack overflows before the first leaf


@pytest.mark.parametrize("steal_min", C.STEAL_MINS)
@pytest.mark.parametrize("case", ["sphere from outside", "64 identical rays", "one lane leaves at trip 3", "lane 0 invalid", "4096 hash rays"])
def test_the_give_away_threshold_ends_the_loop(case, steal_min):
    """the loop and the phase are over before the first look that could give a subtree away, with the schedule where it
    would have been -- odd thresholds and 1 included"""
    v, f, B, o, d = scene(case)
    p, u = same_through_the_loop(B, o, d, steal_min)
    assert (u["per_group"][:, LOOP] + u["per_group"][:, PHASE] <= steal_min).all()
    if case == "64 identical rays":
        assert u["per_group"][0, LOOP] == min(steal_min, p["per_group"][0, FIRST_LEAF])


def test_the_comparison_has_bite():
    for case, wrong in (("mixed octants", U.WRONG_NO_OCTANT_TEST), ("sphere from inside", U.WRONG_NO_OCTANT_TEST),
                        ("sphere from outside", U.WRONG_GOES_ON_AFTER_A_SPLIT), ("one lane leaves at trip 2", U.WRONG_GOES_ON_AFTER_A_SPLIT)):
        v, f, B, o, d = scene(case)
        for q in QUERIES:
            p = U.query(B, q, o, d, U.PHASE)
            assert differences(q, p, U.query(B, q, o, d, wrong)) != [], (case, q)
