"""The descent phase of the stealing closest / first / any launch on the grid nodes (csrc/kernels_direct.inc:
wave_traverse_steal; csrc/tr_bvh.h: tr_descent_step) against the oracle bit for bit -- closest with `loc` and `uv`, first,
any -- on the inputs of tests/test_descent_cpu.py, which holds the phase to the general loop trip by trip on the host.

What the phase can get wrong, and the smallest shape that reaches it:
  * the hand-over to the general loop (the leaves of the phase's last trip, the flavour of the next trip, the place in the
    round of trips): an image of icosphere(3) from outside and from inside, an image of 20 x 12, batches of 1, 63, 65 and
    193 rays, lanes without a valid ray, rays that miss the root's box;
  * a phase that ends on its first trip (two triangles: the root's children are leaves), on its second (three), and a mesh
    without a hierarchy (one triangle: no phase at all);
  * a wave of unrelated rays, which gives subtrees away from its first look on: 4 096 hash rays;
  * a far-child stack that overflows INSIDE the phase: the dense soup of tests/test_descent_cpu.py, where that it does is
    counted on the host;
  * the launches on a learned order and the launch that carries the sort: one shape launched repeatedly, every launch equal
    to the first."""
import numpy as np
import pytest

import workloads as W
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import PRUNING, T, check_query, run_query
from test_gpu_plain_stack import _expect_stealing_grid_launch, _expected, _launch_repeatedly

pytestmark = pytest.mark.gpu


def _image(w, h, distance=2.5, vfov=40.0):
    o, d = W.pinhole_grid(w, h, vfov_deg=vfov, distance=distance)
    return (np.ascontiguousarray(np.broadcast_to(o, d.shape), np.float32).reshape(-1, 3),
            np.ascontiguousarray(d, np.float32).reshape(-1, 3))


def _small_mesh(n):
    v, f = W.two_triangles()
    if n == 1:
        return v[:3].copy(), f[:1].copy()
    if n == 3:
        v = np.concatenate([v, v[:3] + np.float32([10.0, 0.0, 0.0])]).astype(np.float32)
        f = np.concatenate([f, [[6, 7, 8]]]).astype(np.int32)
    return v, f


def _small(n):
    v, f = _small_mesh(n)
    o, d = _image(16, 8, distance=3.0, vfov=30.0)
    return v, f, np.concatenate([o, o + np.float32([10.0, 0.0, 0.0])]), np.concatenate([d, d])


def _sphere(rays):
    v, f = W.icosphere(3)
    o, d = rays(v)
    return v, f, o, d


def _inside(v):
    return W.hash_rays(2048, 11, np.float32([-0.5] * 3), np.float32([0.5] * 3))


def _away(v):
    o, d = _image(16, 16)
    return o + np.float32([0, 0, 1]), -d


def _invalid(v):
    o, d = _image(32, 16)
    d = d.copy()
    d[::3] = 0.0
    d[5::7, 1] = np.nan
    d[64:128] = 0.0
    return o, d


def _stretch(n):
    def rays(v):
        o, d = _image(64, 64)
        s = 64 * 30 + 20
        return o[s:s + n], d[s:s + n]
    return rays


def _dense_soup():
    v, f = W.random_soup(1 << 18, seed=8, extent=0.2, size=3.0)
    o, d = _image(16, 8, distance=4.0 * float(np.abs(v).max()), vfov=5.0)
    return v, f, o, d


CASES = {
    "one triangle": lambda: _small(1),
    "two triangles": lambda: _small(2),
    "three triangles": lambda: _small(3),
    "sphere from outside": lambda: _sphere(lambda v: _image(64, 64)),
    "origins inside": lambda: _sphere(_inside),
    "rays that miss the root box": lambda: _sphere(_away),
    "invalid lanes": lambda: _sphere(_invalid),
    "1 ray": lambda: _sphere(_stretch(1)),
    "63 rays": lambda: _sphere(_stretch(63)),
    "65 rays": lambda: _sphere(_stretch(65)),
    "193 rays": lambda: _sphere(_stretch(193)),
    "image of 20 x 12": lambda: _sphere(lambda v: _image(20, 12)),
    "4096 hash rays": lambda: _sphere(lambda v: W.hash_rays(4096, 4, v.min(0) * 1.5, v.max(0) * 1.5)),
    "stack overflow inside the phase": _dense_soup,
}


@pytest.mark.parametrize("query", PRUNING)
@pytest.mark.parametrize("case", list(CASES))
def test_against_the_oracle(device, case, query):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d = CASES[case]()
    exp = _expected("descent " + case, v, f, o, d)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    ot, dt = T(o, device), T(d, device)
    for k in range(2):
        what = f"{case}, {query}, launch {k}"
        check_query(query, run_query(r, query, ot, dt), exp, what)
        if len(f) >= 2:
            _expect_stealing_grid_launch(r, query, what)


@pytest.mark.parametrize("query", PRUNING)
def test_one_shape_launched_five_times(device, query):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(3)
    o, d = W.pinhole_grid(64, 64, distance=2.5)
    exp = _expected("descent sphere 64", v, f, o, d)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    _launch_repeatedly(r, query, T(o, device), T(d, device), exp, 5)


@pytest.mark.parametrize("query", PRUNING)
def test_learned_order_and_the_launch_that_carries_the_sort(device, query):
    """128 x 128 pixels: an order is learned from 64 blocks on, and its sort rides in a later launch (k_query_direct_sort)"""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(3)
    o, d = W.pinhole_grid(128, 128, distance=2.5)
    exp = _expected("descent sphere 128", v, f, o, d)
    with options(stream=0, steal=1, grid_nodes=1, sort_inline=1, wide_direct=0):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        seen = _launch_repeatedly(r, query, T(o, device), T(d, device), exp, 12)
    assert any(s[1] for s in seen), f"no launch ran on a learned order: {seen}"
    assert any(s[3] for s in seen), f"no launch carried the sort: {seen}"
