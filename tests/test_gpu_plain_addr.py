"""The stealing closest / first / any launch on the grid nodes with the far-child stack addressed by LDS byte address
(csrc/tr_bvh.h: tr_plaina_w, tr_addr_push / tr_addr_pop / tr_addr_give; csrc/kernels_direct.inc: wave_traverse_steal),
against the oracle bit for bit -- closest with `loc` and `uv`, first, any.

What can go wrong with an address that could not with a slot count, and the smallest shape that reaches it:
  * the top of the stack and the lost flag (bit 31 of the address; a lost walk ends at its next pop): the overflowing
    soup of tests/test_gpu_plain_stack.py, 3 000 rays that owe more than sixteen far children at once, under the default
    policy and with hand-overs from the second trip, where thieves lose children too and a donor's stack is shorter by
    its gifts.  That rays ARE lost on this scene through the address form is asserted on the host, where it can be
    counted (tests/test_plain_addr_cpu.py: lost > 0 for closest, first and any); the launch reports no such counter, so
    what the GPU run shows is that every ray of the scene, lost or not, gets the oracle's bits;
  * the hand-over from the address alone (the lane's slot 0 and its slots in use are derived from `sa`, a thief starts
    at its own slot 0): a 64 x 64 pinhole image of icosphere(4) with the give-away threshold at its minimum, so that
    every wave hands over from its first look;
  * the same image on a hierarchy deeper than 32 levels (the DEEP instantiations);
  * the launch that carries the sort (`k_query_direct_sort`, whose first workgroups sort in the LDS the stacks live in):
    launches of one shape (128 x 128 pixels, enough blocks for a learned order) until one has carried it.
tests/test_plain_addr_cpu.py checks the address form against the slot-count form operation by operation on the host."""
import numpy as np
import pytest

import workloads as W
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import ADDRESSING, PRUNING, T, check_query, run_query
from test_gpu_plain_stack import _expect_stealing_grid_launch, _expected, _soup

pytestmark = pytest.mark.gpu


def _image(deep, res=64):
    """icosphere(4), radius 0.3, in the middle of the unit cube, seen by a res x res pinhole camera; `deep`: plus the 63
    single-bit triangles and the pile of five of W.deep_tree_mesh (in the same cube), which make the hierarchy 38 levels"""
    v, f = W.icosphere(4)
    v = (0.3 * v + 0.5).astype(np.float32)
    if deep:
        dv, df = W.deep_tree_mesh(5)
        f = np.concatenate([f, df + len(v)]).astype(np.int32)
        v = np.concatenate([v, dv]).astype(np.float32)
    o, d = W.pinhole_grid(res, res, distance=1.2, center=(0.5, 0.5, 0.5))
    return v, f, o, d, _expected(f"addr image {deep} {res}", v, f, o, d)


@pytest.mark.parametrize("steal", [1, 2], ids=["default policy", "hand-over from the second trip"])
@pytest.mark.parametrize("query", PRUNING)
def test_overflowing_soup(device, query, steal):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d, exp = _soup()
    with options(steal=steal):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        assert 16 < r.bvh_info()["depth"] <= 32               # deep enough to owe more than sixteen, the 32-bit instantiation
        ot, dt = T(o, device), T(d, device)
        for k in range(2):                                # the second launch runs on the learned order
            what = f"{query}, steal = {steal}, launch {k}"
            check_query(query, run_query(r, query, ot, dt), exp, what)
            _expect_stealing_grid_launch(r, query, what)


@pytest.mark.parametrize("deep", [False, True], ids=["32-bit trail", "deeper than 32 levels"])
@pytest.mark.parametrize("query", PRUNING)
def test_image_with_every_wave_handing_over(device, query, deep):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d, exp = _image(deep)
    assert exp["closest"][0].any() and not exp["closest"][0].all()      # the silhouette is in the image
    with options(steal=2, grid_nodes=1, sort_inline=0):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        depth = r.bvh_info()["depth"]
        assert depth > 32 if deep else depth <= 32, depth
        ot, dt = T(o, device), T(d, device)
        for k in range(2):
            what = f"{query}, deep = {deep}, launch {k}"
            check_query(query, run_query(r, query, ot, dt), exp, what)
            li = _expect_stealing_grid_launch(r, query, what)
            assert li["addressing"] == ADDRESSING["deep" if deep else "compact"], li


@pytest.mark.parametrize("query", PRUNING)
def test_launch_that_carries_the_sort(device, query):
    """128 x 128 pixels: an order is learned from 64 blocks on (launch_policy.inc, sched_acquire), and its sort rides in a later launch"""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d, exp = _image(False, 128)
    with options(stream=0, steal=2, grid_nodes=1, sort_inline=1, wide_direct=0):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        ot, dt = T(o, device), T(d, device)
        carried = False
        for k in range(16):
            what = f"{query}, launch {k}"
            check_query(query, run_query(r, query, ot, dt), exp, what)
            li = _expect_stealing_grid_launch(r, query, what)
            if li["sort_carried"]:
                carried = True
                break
        assert carried, "no launch of 16 carried the sort"
