"""The descent phase of the stealing grid-node launch (kernels_direct.inc: wave_traverse_steal; tr_bvh.h: tr_descent_step):
until some lane of a wave accepts a leaf child, a trip is fetch, box test, push / descend / pop and nothing else.  The phase
must change NOTHING: every lane visits the nodes it visited before, in the same trips, and the general loop takes over in
the state and at the point of its schedule that it would have reached by itself.

Checked here, on the host (tests/host_sim/descent_model.cpp: the product's own tr_descent_step and tr_fused_step, rays in
groups of 64 with the wave's exit rule): phase + general loop against the general loop alone, per ray -- every output bit
for bit, node visits, leaf tests, the lost flag.  And that the comparison has bite: two deliberately wrong phases inside the
model (the second leaf of the last trip dropped; the general loop entered with the wrong flavour of trip) are reported."""
import numpy as np
import pytest

import descent_sim as D
import workloads as W
from oracle.oracle import OracleIntersector
from sim import SimBVH

Q_ANY, Q_FIRST, Q_CLOSEST = 0, 1, 2
QUERIES = (Q_ANY, Q_FIRST, Q_CLOSEST)
OUTPUTS = {Q_ANY: ("hit",), Q_FIRST: ("tri",), Q_CLOSEST: ("hit", "front", "tri", "loc", "uv")}


def differences(q, a, b):
    """what differs between two runs of the model: names of outputs (compared as bytes: a NaN or a -0.0 counts), and the
    per-ray counters"""
    bad = [k for k in OUTPUTS[q] if a[k].tobytes() != b[k].tobytes()]
    for j, name in enumerate(D.PER_RAY):
        if not np.array_equal(a["per_ray"][:, j], b["per_ray"][:, j]):
            bad.append(name)
    return bad


def same_through_the_phase(B, o, d, steal_min=D.STEAL_MIN, queries=QUERIES):
    """general loop alone against phase + general loop, for every query; returns the closest-hit pair of runs"""
    pair = None
    for q in queries:
        g = D.query(B, q, o, d, D.GENERAL, steal_min)
        h = D.query(B, q, o, d, D.DESCENT, steal_min)
        assert differences(q, g, h) == [], (q, differences(q, g, h))
        assert g["lost"] == h["lost"]
        if q == Q_CLOSEST:
            pair = (g, h)
    return pair


def image(w, h, distance=2.5, vfov=40.0):
    o, d = W.pinhole_grid(w, h, vfov_deg=vfov, distance=distance)
    return np.ascontiguousarray(np.broadcast_to(o, d.shape), np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)


@pytest.fixture(scope="module")
def sphere():
    v, f = W.icosphere(3)
    return v, f, SimBVH(v, f)


def small_mesh(n):
    """1 triangle: no internal node; 2: a root with two leaf children; 3: a root with a leaf and an internal child"""
    v, f = W.two_triangles()
    if n == 1:
        return v[:3].copy(), f[:1].copy()
    if n == 3:
        v = np.concatenate([v, v[:3] + np.float32([10.0, 0.0, 0.0])]).astype(np.float32)      # far off to the side: the root's leaf child
        f = np.concatenate([f, [[6, 7, 8]]]).astype(np.int32)
    return v, f


@pytest.mark.parametrize("ntri", [1, 2, 3])
def test_meshes_of_one_two_and_three_triangles(ntri):
    v, f = small_mesh(ntri)
    o, d = image(16, 8, distance=3.0, vfov=30.0)
    o, d = np.concatenate([o, o + np.float32([10.0, 0.0, 0.0])]), np.concatenate([d, d])      # two groups at the pair, two beside it
    g, h = same_through_the_phase(SimBVH(v, f), o, d)
    phase = h["per_group"][:, 3]
    if ntri == 1:
        assert (phase == 0).all() and not h["hit"].any()      # no hierarchy: nothing is walked (the kernels test the triangle directly)
        return
    want = OracleIntersector(v, f, 1).closest_raw(o, d)[:5]
    for key, w in zip(OUTPUTS[Q_CLOSEST], want):
        assert np.array_equal(h[key], w.reshape(h[key].shape)), key
    assert h["hit"][:128].any()
    if ntri == 2:
        assert (phase == 1).all()                  # the root's children are leaves: the phase ends on its first trip
    if ntri == 3:
        assert h["hit"][128:].any()
        assert phase.tolist() == [2, 2, 1, 1]      # through the internal child to its leaves; the root's leaf child at once


def test_sphere_from_outside(sphere):
    v, f, B = sphere
    o, d = image(64, 64)
    g, h = same_through_the_phase(B, o, d)
    want = OracleIntersector(v, f, 1).closest_raw(o, d)[:5]
    for key, w in zip(OUTPUTS[Q_CLOSEST], want):
        assert np.array_equal(h[key], w.reshape(h[key].shape)), key
    # the phase did run, and it ended on the trip that gave the wave its first leaf
    hitting = g["per_group"][:, 0] > 0
    assert hitting.any() and h["per_group"][:, 3].mean() > 4
    assert np.array_equal(h["per_group"][hitting, 3], g["per_group"][hitting, 0])
    assert np.array_equal(h["per_group"][:, 2], g["per_group"][:, 2])      # the waves are as long as they were


def test_the_comparison_has_bite(sphere):
    v, f, B = sphere
    o, d = image(64, 64)
    for q in QUERIES:
        g = D.query(B, q, o, d, D.GENERAL)
        assert differences(q, g, D.query(B, q, o, d, D.WRONG_DROPS_SECOND_LEAF)) != [], q
        assert differences(q, g, D.query(B, q, o, d, D.WRONG_FLAVOUR)) != [], q


def test_origins_inside_the_mesh(sphere):
    v, f, B = sphere
    lo, hi = np.float32([-0.5] * 3), np.float32([0.5] * 3)
    o, d = W.hash_rays(2048, 11, lo, hi)
    assert (np.linalg.norm(o, axis=1) < 0.9).all()
    g, h = same_through_the_phase(B, o, d)
    assert h["hit"].all()
    # coherent origins too: one point inside, an image's directions
    o2, d2 = image(32, 32)
    same_through_the_phase(B, np.zeros_like(o2) + np.float32([0.1, -0.2, 0.3]), d2)


def test_rays_that_miss_the_root_box(sphere):
    v, f, B = sphere
    o, d = image(16, 16)
    g, h = same_through_the_phase(B, o + np.float32([0, 0, 1]), -d)      # looking away
    assert not h["hit"].any()
    assert (h["per_ray"][:, 0] == 1).all() and (h["per_group"][:, 3] == 1).all()      # the root's visit, and the phase is over


def test_invalid_lanes(sphere):
    v, f, B = sphere
    o, d = image(32, 16)
    d = d.copy()
    d[::3] = 0.0
    d[5::7, 1] = np.nan
    d[64:128] = 0.0                       # a whole group without a valid ray
    g, h = same_through_the_phase(B, o, d)
    assert h["hit"].any() and not h["hit"][::3].any() and not h["hit"][64:128].any()
    assert h["per_group"][1, 0] == 0 and (h["per_ray"][64:128, 1] == 0).all()      # that group never has a leaf


@pytest.mark.parametrize("n", [1, 63, 65, 193])
def test_group_sizes(sphere, n):
    v, f, B = sphere
    o, d = image(64, 64)
    s = 64 * 30 + 20                      # a stretch of the image that crosses the silhouette
    g, h = same_through_the_phase(B, o[s:s + n], d[s:s + n])
    assert len(h["per_group"]) == (n + 63) // 64 and h["hit"].any()


def test_an_image_of_20_by_12(sphere):
    v, f, B = sphere
    o, d = image(20, 12)
    g, h = same_through_the_phase(B, o, d)
    assert h["hit"].any() and not h["hit"].all()


@pytest.mark.parametrize("steal_min", [D.STEAL_EARLY, D.STEAL_MIN, 5, 1])
def test_hash_rays_and_the_incoherent_vote(sphere, steal_min):
    """a wave of unrelated rays gives subtrees away from trip TR_STEAL_EARLY on: the phase must be over by then, with the
    schedule where it would have been (and with any other threshold, odd ones included)"""
    v, f, B = sphere
    o, d = W.hash_rays(4096, 4, v.min(0) * 1.5, v.max(0) * 1.5)
    g, h = same_through_the_phase(B, o, d, steal_min)
    assert h["hit"].any()
    assert h["per_group"][:, 3].max() <= steal_min


def test_a_stack_that_overflows_inside_the_phase():
    """a dense soup (2^18 triangles that all overlap: eighteen levels on which both children are hit before the first leaf)
    seen through a narrow image: every ray pushes a seventeenth far child before its wave has a leaf"""
    v, f = W.random_soup(1 << 18, seed=8, extent=0.2, size=3.0)
    o, d = image(16, 8, distance=4.0 * float(np.abs(v).max()), vfov=5.0)
    B = SimBVH(v, f)
    for q in QUERIES:
        g = D.query(B, q, o, d, D.GENERAL)
        h = D.query(B, q, o, d, D.DESCENT)
        assert g["lost_before_first_leaf"] > 0, "no ray lost a child before its group's first leaf: the input does not reach the case"
        assert h["lost_in_phase"] >= g["lost_before_first_leaf"]
        assert differences(q, g, h) == [], (q, differences(q, g, h))
        assert g["lost"] == h["lost"] > 0
    want = OracleIntersector(v, f, 1).closest_raw(o, d)[:5]
    for key, w in zip(OUTPUTS[Q_CLOSEST], want):
        assert np.array_equal(h[key], w.reshape(h[key].shape)), key
