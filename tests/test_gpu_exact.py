"""Every GPU query against the integer-arithmetic reference of tests/exact_ref.py, on scenes made of exact ties and of
near-ties (tests/test_exact_cpu.py holds the oracle and the host simulation to the same reference and describes the two
corpora).

Under the default options every output of any / first / closest / count / location / id goes through the assertions
of exact_checks (the ideal rule on the lattice scenes; one crossing, parity and the rounding band on the
near-degenerate ones) and must equal the oracle bit for bit.  Then every launch shape of
test_gpu_kernel_matrix.SHAPES, with compact and generic addressing, runs the same rays: its outputs must equal the
oracle's, bit for bit -- the oracle's outputs having passed exact_checks in this very session (verified()) -- and
tr_bvh_last_launch must report the shape the case claims, so that every family that reaches a leaf test sees the ties.
Ray lists are repeated up to the smallest batch a shape takes (64 blocks of 128 rays for the learned order that the
sort-carrying launches need); the scenes stay as small as they are.

contains_points (the fused launch and the torch statements) and the sign of signed_distance on the closed lattice
scenes and the flat tetrahedra: integer points and points at odd multiples of 1/2, the truth from the parity of ideal
crossings along an axis -- another ray than the library shoots, the same truth."""
import functools

import numpy as np
import pytest
import torch

import exact_checks as K
import exact_ref as X
from launch_options import options
from oracle.oracle import OracleIntersector
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import SHAPES, T, check_query, expect_launch, run_query

pytestmark = pytest.mark.gpu

LATTICE = [s["name"] for s in X.lattice_scenes()]
DEGENERATE = [r["name"] for r in X.degenerate_scenes()]
GROUPS = {"fans": [n for n in DEGENERATE if n.startswith("fan")], "tetrahedra": [n for n in DEGENERATE if n.startswith("tetra")],
          "tube and needles": [n for n in DEGENERATE if n.startswith(("tube", "needle"))]}
MIN_ORDERED_BATCH = 64 * 128      # sched_acquire (csrc/launch_policy.inc): no learned order below 64 blocks of TR_BS = 128 rays


def scene_of(name):
    return next(s for s in X.lattice_scenes() + X.degenerate_scenes() if s["name"] == name)


@functools.lru_cache(maxsize=None)
def verified(name):
    """the oracle's outputs on the scene, after they passed the assertions of exact_checks"""
    s = scene_of(name)
    R = OracleIntersector(s["v"], s["f"], 1)
    res = K.oracle_results(R, s["o"], s["d"])
    if name in LATTICE:
        K.check_lattice(s, res, K.anchored_mask(R, s["o"], s["d"]), f"{name} / oracle")
    else:
        for o in s["stars"]:
            assert X.star_shaped(s["v"], s["f"], o), f"{name}: not star-shaped from {o}"
        K.check_degenerate(s, res, f"{name} / oracle")
    return res


@functools.lru_cache(maxsize=None)
def expected(name, reps):
    """what check_query compares with, on the ray list repeated `reps` times"""
    s = scene_of(name)
    if reps == 1:
        res = verified(name)
    else:
        o, d = np.tile(s["o"], (reps, 1)), np.tile(s["d"], (reps, 1))
        res = K.oracle_results(OracleIntersector(s["v"], s["f"], 1), o, d)
        K.assert_same({k: v[:len(s["o"])] for k, v in res.items() if not k.startswith("list")}, verified(name), name)
    return {"closest": (res["hit"], res["front"], res["tri"], res["loc"], res["uv"]), "count": res["count"],
            "location": (res["list_loc"], res["list_ray"], res["list_tri"])}


def make(s, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(s["v"], device), faces=T(s["f"], device))


def gpu_results(r, ot, dt):
    hit, front, tri, loc, uv = r.intersects_closest(ot, dt)
    ll, lr, lt = r.intersects_location(ot, dt)
    it, ir, il = r.intersects_id(ot, dt, return_locations=True)
    assert torch.equal(it, lt) and torch.equal(ir, lr) and torch.equal(il, ll)
    it1, ir1 = r.intersects_id(ot, dt, multiple_hits=False)
    assert torch.equal(it1, tri[hit]) and torch.equal(ir1, torch.nonzero(hit).reshape(-1).to(torch.int32))
    n = lambda x: x.cpu().numpy()  # noqa: E731
    return dict(count=n(r.intersects_count(ot, dt)), any=n(r.intersects_any(ot, dt)), first=n(r.intersects_first(ot, dt)),
                hit=n(hit), front=n(front), tri=n(tri), loc=n(loc), uv=n(uv), list_loc=n(ll), list_ray=n(lr), list_tri=n(lt))


@pytest.mark.parametrize("name", LATTICE)
def test_lattice_scene_equals_the_ideal_rule(device, name):
    s = scene_of(name)
    res = gpu_results(make(s, device), T(s["o"], device), T(s["d"], device))
    anchored = K.anchored_mask(OracleIntersector(s["v"], s["f"], 1), s["o"], s["d"])
    K.check_lattice(s, res, anchored, f"{name} / GPU")
    K.assert_same(res, verified(name), f"{name} / GPU")


@pytest.mark.parametrize("group", list(GROUPS))
def test_near_degenerate_scenes_have_one_crossing_from_inside(device, group):
    for name in GROUPS[group]:
        s = scene_of(name)
        res = gpu_results(make(s, device), T(s["o"], device), T(s["d"], device))
        K.check_degenerate(s, res, f"{name} / GPU")
        K.assert_same(res, verified(name), f"{name} / GPU")


# (the corpora's hierarchies are at most 20 levels high: `deep` addressing has nothing to run on here)
@pytest.mark.parametrize("addressing,shape", [(a, s) for s in SHAPES for a in ("compact", "generic") if a in SHAPES[s][2]])
def test_every_launch_shape_sees_the_ties(device, addressing, shape):
    opts, queries, _, _ = SHAPES[shape]
    streaming = shape.startswith("stream")
    for name in LATTICE + DEGENERATE:
        s = scene_of(name)
        reps = -(-MIN_ORDERED_BATCH // len(s["o"])) if shape == "sort_carried" else 1
        exp = expected(name, reps)
        ot, dt = T(np.tile(s["o"], (reps, 1)), device), T(np.tile(s["d"], (reps, 1)), device)
        with options(compact=0 if addressing == "generic" else 1, **opts):
            r = make(s, device)
            assert r.bvh_info()["depth"] <= 32, name
            for query in queries:
                what = f"{query} / {addressing} / {shape} / {name}"
                if shape == "sort_carried":
                    carried = False
                    for k in range(16):
                        check_query(query, run_query(r, query, ot, dt), exp, f"{what} launch {k}")
                        if expect_launch(r, query, shape, addressing, f"{what} launch {k}")["sort_carried"]:
                            carried = True
                            break
                    assert carried, f"{what}: no launch of 16 carried the sort"
                    continue
                for k in range(2):                    # the second launch runs on the learned order, where there is one
                    check_query(query, run_query(r, query, ot, dt), exp, f"{what} launch {k}")
                    if streaming:
                        with pytest.raises(ValueError, match="no direct launch"):
                            r.as_wrapper.last_launch()
                    else:
                        assert expect_launch(r, query, shape, addressing, f"{what} launch {k}")["sort_carried"] == 0, what
            torch.cuda.synchronize()


def _closed_scenes():
    return [s["name"] for s in X.lattice_scenes() if s["closed"]] + GROUPS["tetrahedra"]


@functools.lru_cache(maxsize=None)
def points_of(name):
    s = scene_of(name)
    return X.lattice_points(s) if name in LATTICE else X.tetra_points(s)


@pytest.mark.parametrize("name", _closed_scenes())
def test_contains_points_and_the_sign_of_signed_distance(device, name):
    s = scene_of(name)
    p, inside = points_of(name)
    assert inside.any() and not inside.all()
    r = make(s, device)
    pt = T(p, device)
    retry = torch.tensor([0.3, -0.2, 0.45])
    assert r.native_contains is True
    try:
        for native in (True, False):
            r.native_contains = native
            got = r.contains_points(pt, _retry_direction=retry).cpu().numpy()
            assert np.array_equal(got, inside), f"{name} native {native}: {int((got != inside).sum())} of {len(p)} points"
    finally:
        r.native_contains = True
    # the SIGN (positive inside): a face of a flat tetrahedron passes its inner points closer than float64 resolves, and
    # the distance -- closest_point's own arithmetic, not looked at here -- may then be zero: +0 inside, -0 outside
    sd = r.signed_distance(pt).cpu().numpy()
    assert np.all(np.isfinite(sd))
    assert np.array_equal(~np.signbit(sd), inside), f"{name}: the sign of signed_distance is wrong at {int((~np.signbit(sd) != inside).sum())} points"
