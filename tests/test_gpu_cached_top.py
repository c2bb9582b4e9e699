"""The trip of the stealing closest / first / any launch on the grid nodes after its LDS waits were taken out of the
body (csrc/tr_bvh.h: the plain-stack branch of tr_fused_body issues the pop's load behind the descend path's write;
csrc/kernels_direct.inc: the look at the wave tests the wave-uniform threshold before any lane reads `bot`), against the
oracle bit for bit and against the launch record.

The smallest shapes at which these changes can go wrong:
  * early hand-over on the overflow soup: donors hold one or two entries when they give, so the slot given away is the top
    of the donor's stack, and thieves lose children;
  * one batch of exactly 64 rays, one of 65 and one of 127: a whole wave, a wave with one live lane, a last wave with one
    dead lane -- idle lanes in the first look, below the threshold;
  * the 128 x 128 image with tiles and split blocks: lanes that start idle and steal at once, the other half of the
    threshold argument, the launch that carries the sort;
  * the deep tree of tests/hostile_rays.py (more than 32 levels): the DEEP instantiation.

The file carries the name of the variant these cases were written for, the top of the stack cached in a register, which was
measured slower and does not ship (DESIGN_experiments.md part R9).  The soup and the split-block cases repeat cases of
tests/test_gpu_plain_stack.py on purpose; the 64 / 65 / 127-ray batches and the deep tree are new.  The shipped change is
bit-identical to the code before it, so none of these cases can tell the two apart: they guard the walk, not the speed."""
import numpy as np
import pytest

import hostile_rays as H
import workloads as W
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import ADDRESSING, PRUNING, T, check_query, run_query
from test_gpu_plain_stack import _expect_stealing_grid_launch, _expected, _launch_repeatedly, _soup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("query", PRUNING)
def test_early_hand_over_on_the_soup(device, query):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d, exp = _soup()
    with options(steal=2):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        assert 16 < r.bvh_info()["depth"] <= 32
        ot, dt = T(o, device), T(d, device)
        for k in range(2):
            what = f"{query}, hand-over from the second trip, launch {k}"
            check_query(query, run_query(r, query, ot, dt), exp, what)
            _expect_stealing_grid_launch(r, query, what)


@pytest.mark.parametrize("rays", [64, 65, 127])
@pytest.mark.parametrize("query", PRUNING)
def test_whole_wave_and_straddling_waves(device, query, rays):
    """the first `rays` pixels of a 64 x 64 image of icosphere(5): rows of 64 pixels, so a whole wave, a wave with one
    live lane behind it, and a last wave with one dead lane"""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(5)
    o, d = W.pinhole_grid(64, 64, distance=2.5)
    o = np.ascontiguousarray(np.broadcast_to(o, d.shape), np.float32).reshape(-1, 3)[:rays]
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)[:rays]
    exp = _expected(f"icosphere5/first{rays}", v, f, o, d)
    assert exp["closest"][0].any(), "no ray of the batch hits the sphere"
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    ot, dt = T(o, device), T(d, device)
    for k in range(2):
        what = f"{query}, {rays} rays, launch {k}"
        check_query(query, run_query(r, query, ot, dt), exp, what)
        _expect_stealing_grid_launch(r, query, what)


@pytest.mark.parametrize("query", PRUNING)
def test_split_blocks_and_the_carried_sort(device, query):
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
def test_deep_tree(device, query):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = H.scene("deep")[:2]
    batch, exp = H.expected("deep", "interleaved")
    with options(compact=1, stream=0, steal=2, grid_nodes=1, wide_direct=0):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        assert r.bvh_info()["depth"] > 32
        ot, dt = T(np.array(batch.o, order="C"), device), T(np.array(batch.d, order="C"), device)
        for k in range(2):
            what = f"{query} / deep tree / launch {k}"
            check_query(query, run_query(r, query, ot, dt), exp, what)
            li = _expect_stealing_grid_launch(r, query, what)
            assert li["addressing"] == ADDRESSING["deep"], f"{what}: not the DEEP instantiation: {li}"
