"""The uniform top of the stealing closest / first / any launch on the grid nodes (csrc/kernels_direct.inc:
wave_traverse_steal; csrc/tr_bvh.h: tr_uniform_test, tr_uniform_wave) against the oracle bit for bit -- closest with `loc` and
`uv`, first, any -- on the inputs of tests/test_uniform_top_cpu.py (tests/uniform_top_cases.py), which holds the loop to the
descent phase trip by trip on the host and shows what each input reaches: a leaf child at the root, waves that stay at one
node down to their first leaf, a lane that leaves the common path on trips 1 to 5, lanes without a ray (lane 0 among them),
rays that miss the root's box, waves of mixed octants (which must not enter the loop), batches of 1 / 63 / 65 / 193 rays, and
a far-child stack that overflows before the first leaf.

The give-away threshold: option steal = N >= 2 makes N the trip from which subtrees are given away, which is where the loop
and the phase must be over -- 4, 5 and 64 as on the host, and 2, the smallest the option can name; steal = 1 is the default
policy (64, or 4 for a wave of unrelated rays).  A threshold of 1 exists only in the host simulation.

And one shape launched five times, plus the launch that carries the sort (k_query_direct_sort runs the same loop)."""
import pytest

import uniform_top_cases as C
import workloads as W
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_descent import _expected, _expect_stealing_grid_launch, _launch_repeatedly
from test_gpu_kernel_matrix import PRUNING, T, check_query, run_query

pytestmark = pytest.mark.gpu

_SCENES = {}


def _scene(case):
    if case not in _SCENES:
        _SCENES[case] = C.CASES[case]()
    return _SCENES[case]


@pytest.mark.parametrize("query", PRUNING)
@pytest.mark.parametrize("case", list(C.CASES))
def test_against_the_oracle(device, case, query):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d = _scene(case)
    exp = _expected("uniform top " + case, v, f, o, d)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    ot, dt = T(o, device), T(d, device)
    for k in range(2):
        what = f"{case}, {query}, launch {k}"
        check_query(query, run_query(r, query, ot, dt), exp, what)
        if len(f) >= 2:
            _expect_stealing_grid_launch(r, query, what)


@pytest.mark.parametrize("query", PRUNING)
@pytest.mark.parametrize("steal", [4, 64, 5, 2])
@pytest.mark.parametrize("case", ["sphere from outside", "64 identical rays", "one lane leaves at trip 3", "lane 0 invalid", "4096 hash rays"])
def test_give_away_thresholds(device, case, steal, query):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d = _scene(case)
    exp = _expected("uniform top " + case, v, f, o, d)
    with options(steal=steal):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        what = f"{case}, {query}, steal = {steal}"
        check_query(query, run_query(r, query, T(o, device), T(d, device)), exp, what)
        _expect_stealing_grid_launch(r, query, what)


@pytest.mark.parametrize("query", PRUNING)
def test_one_shape_launched_five_times_and_the_launch_that_carries_the_sort(device, query):
    """64 x 64 pixels five times through the default policy; then 128 x 128: an order is learned from 64 blocks on, and its
    sort rides in a later launch (k_query_direct_sort)"""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(3)
    o, d = W.pinhole_grid(64, 64, distance=2.5)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    _launch_repeatedly(r, query, T(o, device), T(d, device), _expected("descent sphere 64", v, f, o, d), 5)
    o, d = W.pinhole_grid(128, 128, distance=2.5)
    exp = _expected("descent sphere 128", v, f, o, d)
    with options(stream=0, steal=1, grid_nodes=1, sort_inline=1, wide_direct=0):
        r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
        seen = _launch_repeatedly(r, query, T(o, device), T(d, device), exp, 12)
    assert any(s[1] for s in seen), f"no launch ran on a learned order: {seen}"
    assert any(s[3] for s in seen), f"no launch carried the sort: {seen}"
