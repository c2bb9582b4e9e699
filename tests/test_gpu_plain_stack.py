"""The stealing closest / first / any launch on the grid nodes with the plain far-child stack (csrc/tr_bvh.h: tr_plain_w;
csrc/kernels_direct.inc: wave_traverse_steal, retraverse_lost), against the oracle bit for bit.

The shapes are the smallest that can still go wrong:
  * the overflow scene of tests/test_plain_stack_cpu.py -- rays that owe more than sixteen far children at once, so that
    lanes lose children and their rays take the second, stackless traversal -- through the default policy, and with the
    hand-over forced to its earliest trip, so that the lanes that lose children include thieves, whose flag has to reach
    the ray's owner;
  * a 64 x 64 image launched six times through the default policy, and a 128 x 128 image with tiles and split blocks
    switched on: 8 x 8 tiles (the scalar tile arithmetic of the prologue), the cold launch, the learning launches, split
    blocks and the launch that carries the sort;
  * the hostile batch of tests/hostile_rays.py (waves with dead rays, rays that walk most of the tree).
tests/test_plain_stack_cpu.py shows on the host simulation that the overflow scene does overflow."""
import numpy as np
import pytest

import hostile_rays as H
import workloads as W
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import PRUNING, QID, T, check_query, run_query

pytestmark = pytest.mark.gpu

_CACHE = {}


def _expected(key, v, f, o, d):
    """the oracle's results, computed once per scene and left unchanged"""
    if key not in _CACHE:
        from oracle.oracle import OracleIntersector
        R = OracleIntersector(v, f, 1)
        of, df = (np.ascontiguousarray(np.broadcast_to(x, np.shape(d)), np.float32).reshape(-1, 3) for x in (o, d))
        exp = {"closest": R.closest_raw(of, df)[:5], "count": R.intersects_count(of, df)}
        for a in list(exp["closest"]) + [exp["count"]]:
            a.setflags(write=False)
        _CACHE[key] = exp
    return _CACHE[key]


def _soup():
    v, f = W.random_soup(30000, seed=8, size=1.5)
    o, d = W.hash_rays(3000, 4, v.min(0) * 1.5, v.max(0) * 1.5)
    return v, f, o, d, _expected("soup", v, f, o, d)


def _expect_stealing_grid_launch(r, query, what):
    li = r.as_wrapper.last_launch()
    assert (li["query"], li["shape"], li["grid_nodes"]) == (QID[query], 1, 1), f"{what}: not the stealing launch on the grid nodes: {li}"
    return li


@pytest.mark.parametrize("steal", [1, 2], ids=["default policy", "hand-over from the second trip"])
@pytest.mark.parametrize("query", PRUNING)
def test_rays_that_lose_far_children_get_the_oracles_answer(device, query, steal):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d, exp = _soup()
    with options(steal=steal):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        assert 16 < r.bvh_info()["depth"] <= 32
        ot, dt = T(o, device), T(d, device)
        for k in range(2):                                # the second launch runs on the learned order
            what = f"{query}, steal = {steal}, launch {k}"
            check_query(query, run_query(r, query, ot, dt), exp, what)
            _expect_stealing_grid_launch(r, query, what)


def _launch_repeatedly(r, query, ot, dt, exp, launches):
    """every launch equals the oracle and the first -> per launch (tile rows lg, learned order, split blocks, sort carried)"""
    import torch
    first, seen = None, []
    for k in range(launches):
        got = run_query(r, query, ot, dt)
        check_query(query, got, exp, f"{query}, launch {k}")
        li = _expect_stealing_grid_launch(r, query, f"{query}, launch {k}")
        seen.append((li["tile_rows_lg"], li["learned_order"], li["split_blocks"], li["sort_carried"]))
        got = got if isinstance(got, (tuple, list)) else (got,)
        if first is None:
            first = [g.clone() for g in got]
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, first)), f"{query}: launch {k} differs from the first"
    print(f"{query}: (tile rows lg, learned order, split blocks, sort carried) per launch: {seen}")
    return seen


@pytest.mark.parametrize("query", PRUNING)
def test_small_image_launched_six_times(device, query):
    """64 x 64 pixels of icosphere(5) through the default policy (32 blocks: rows of 64 pixels, no learned order)"""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(5)
    o, d = W.pinhole_grid(64, 64, distance=2.5)
    exp = _expected("icosphere5/64", v, f, o, d)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    _launch_repeatedly(r, query, T(o, device), T(d, device), exp, 6)


@pytest.mark.parametrize("query", PRUNING)
def test_image_tiles_split_blocks_and_the_learned_order(device, query):
    """The default policy gives an image of 32 blocks neither tiles nor a learned order (launch_policy.inc, sched_acquire: an order is
    learned from 64 blocks on, tiles and split blocks come with much larger launches).  128 x 128 pixels = 128 blocks with
    8 x 8 tiles and split blocks switched on by option reach all of it: the cold launch, the measuring launches, the
    learned order with split blocks (lanes that start idle and steal at once) and the launch that carries the sort."""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(5)
    o, d = W.pinhole_grid(128, 128, distance=2.5)
    exp = _expected("icosphere5/128", v, f, o, d)
    with options(tile=2, split=2):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        seen = _launch_repeatedly(r, query, T(o, device), T(d, device), exp, 10)
    assert all(s[0] == 3 for s in seen), f"8 x 8 tiles on every launch: {seen}"
    assert seen[0][1] == 0 and any(s[1] for s in seen), f"a cold launch, then launches on a learned order: {seen}"
    assert any(s[2] > 0 for s in seen), f"no launch had split blocks: {seen}"
    assert any(s[3] for s in seen), f"no launch carried the sort: {seen}"


@pytest.mark.parametrize("query", PRUNING)
def test_hostile_rays_through_the_stealing_launch(device, query):
    from triro.ray.ray_optix import RayMeshIntersector
    for name in ("soup", "shells"):
        v, f = H.scene(name)[:2]
        batch, exp = H.expected(name, "interleaved")
        with options(stream=0, steal=2, grid_nodes=1, wide_direct=0):
            r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
            ot, dt = T(np.array(batch.o, order="C"), device), T(np.array(batch.d, order="C"), device)
            for k in range(2):
                what = f"{query} / {name} / launch {k}"
                check_query(query, run_query(r, query, ot, dt), exp, what)
                _expect_stealing_grid_launch(r, query, what)
