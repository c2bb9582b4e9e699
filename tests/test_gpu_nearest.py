"""closest_point / signed_distance (libtriro_nearest.so, k_closest_point) against the host brute force.

The oracle of every comparison is tests/host_sim/nearest_sim.brute: the per-triangle function of csrc/tr_nearest.h over
every triangle with the lexicographic minimum (d2, face index), on the same float32 inputs -- itself pinned to an
independent numpy evaluation by tests/test_nearest_cpu.py.  Comparisons are bit for bit (tri, closest, distance), NaN
and +Inf included.  Every native call of this module comes back through a wrapper that runs poison.assert_written on
closest, distance and tri (the autouse fixture `checked_native`); the captured call is checked after each replay."""
import numpy as np
import pytest
import torch

import nearest_cases as NC
import poison
import workloads as W
from oracle.oracle import OracleIntersector
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

CALLS = {"native": 0}


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every native call: counted, and -- outside a graph capture -- all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    original = hops.closest_point_native

    def call(*args, **kwargs):
        res = original(*args, **kwargs)
        CALLS["native"] += 1
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize()
            poison.assert_written(*res, what="closest_point_native (closest, distance, tri)")
        return res
    hops.closest_point_native = call
    try:
        yield
    finally:
        hops.closest_point_native = original


@pytest.fixture(scope="module")
def cases():
    """(vertices, faces, points, brute force) of the hierarchical meshes, computed once"""
    import nearest_sim
    out = {}
    for name, mk in NC.HIERARCHICAL.items():
        v, f, p = mk()
        out[name] = (v, f, p, nearest_sim.brute(v, f, p))
    return out


def native(r, p, device, **kw):
    import triro.backend.ops as hops
    res = hops.closest_point_native(r.as_wrapper, T(np.ascontiguousarray(p, np.float32).reshape(-1, 3), device), **kw)
    return tuple(None if x is None else x.cpu().numpy() for x in res)


def check(r, v, f, p, device, what, want=None, **kw):
    import nearest_sim
    want = nearest_sim.brute(v, f, p) if want is None else want
    got = native(r, p, device, **kw)
    NC.assert_same_bits(got, want, what)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NC.HIERARCHICAL))
def test_hierarchical_meshes_at_every_stack_limit(device, cases, name):
    v, f, p, want = cases[name]
    r = make(v, f, device)
    if name == "deep":
        assert r.bvh_info()["depth"] > 32
    for entries in (0, 1, 2, 3):
        check(r, v, f, p, device, f"{name}, stack_entries {entries}", want=want, stack_entries=entries)


def test_kernel_matches_the_host_walk_on_the_gpu_builders_tree(device, cases):
    import nearest_sim
    from sim import SimBVH
    v, f, p, want = cases["icosphere"]
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    for entries in (0, 1):
        host = nearest_sim.walk(B, p, entries)
        NC.assert_same_bits(native(r, p, device, stack_entries=entries), host, f"GPU tree, stack_entries {entries}")
        NC.assert_same_bits(host, want, "host walk on the GPU tree against the brute force")


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_case():
    import nearest_sim
    v, f, _ = NC.icosphere()
    p = NC.hash_points(4133, 3, [-1.4] * 3, [1.4] * 3)
    return v, f, p, nearest_sim.brute(v, f, p)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, tail_case, n):
    v, f, p, want = tail_case
    r = make(v, f, device)
    want = tuple(x[:n] for x in want)
    got = check(r, v, f, p[:n], device, f"{n} points", want=want)
    assert got[0].shape == (n, 3) and got[1].shape == (n,) and got[2].shape == (n,)
    c, d, t = check(r, v, f, p[:n], device, f"{n} points, no closest", want=(None,) + want[1:], want_closest=False)
    assert c is None and d is not None
    c, d, t = check(r, v, f, p[:n], device, f"{n} points, no distance", want=(want[0], None, want[2]), want_distance=False)
    assert d is None and c is not None
    c, d, t = check(r, v, f, p[:n], device, f"{n} points, tri only", want=(None, None, want[2]), want_closest=False, want_distance=False)
    assert c is None and d is None and t.shape == (n,)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_meshes_without_a_hierarchy(device):
    v, f = W.two_triangles()
    p = np.concatenate([NC.hash_points(300, 5, [-0.8, -0.8, -1.4], [0.8, 0.8, 0.4]),
                        np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.5, -0.5, 0.0], [np.nan, 0.0, 0.0]], np.float32)])
    for nt in (2, 1, 0):
        vv, ff = v[:3 * nt], f[:nt]
        r = make(vv, ff, device)
        for entries in (0, 1):
            c, d, t = check(r, vv, ff, p, device, f"{nt} triangle(s)", stack_entries=entries)
        if nt == 0:
            assert (t == -1).all() and np.isposinf(d).all() and np.isnan(c).all()
        else:
            assert t[-1] == -1 and (t[:-1] >= 0).all() and t.max() == nt - 1
    assert native(make(v, f, device), p, device)[2][300] == 0          # between the two: the tie goes to face 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_hostile_points(device):
    v, f, _ = NC.icosphere()
    r = make(v, f, device)
    ordinary = NC.hash_points(256, 17, [-1.3] * 3, [1.3] * 3)
    p = ordinary.copy()
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p[5 + 7 * k, axis] = bad
            k += 1
    p[70] = [3e38, 3e38, 3e38]; p[71] = [-3e38, 0.1, 3e38]; p[72] = [0, 0, -3e38]; p[73] = [3e38, 0, 0]
    p[74] = [2.0 ** 60, 0, 0]; p[75] = [-(2.0 ** 60), 2.0 ** 60, 0.5]
    p[76] = [1e-45, -1e-40, 3e-39]; p[77] = [1e-39, 0, 0]; p[78] = [0, 0, 0]
    p[128:192] = np.nan                                   # a whole wave of invalid points ...
    p = np.concatenate([p, np.full((128, 3), np.inf, np.float32), ordinary[:70]])      # ... and a whole block of them
    for entries in (0, 1):
        c, d, t = check(r, v, f, p, device, f"hostile points, stack_entries {entries}", stack_entries=entries)
    bad = ~np.isfinite(p).all(1)
    assert bad.sum() == 9 + 64 + 128
    assert (t[bad] == -1).all() and np.isposinf(d[bad]).all() and np.isnan(c[bad]).all()
    assert (t[~bad] >= 0).all() and np.isfinite(c[~bad]).all() and not np.isnan(d).any()
    assert np.isposinf(d[70]) and np.isposinf(d[71]) and np.isfinite(d[72]) and np.isfinite(d[74])      # beyond the float range: +Inf on both sides


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_gpu_result_agrees_with_the_independent_numpy_evaluation(device, cases):
    v, f, p, _ = cases["icosphere"]
    c, d, t = native(make(v, f, device), p, device)
    NC.check_against_numpy(v, f, p, c, d, t, what="icosphere on the GPU")


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_closest_point_batch_shapes_and_input_types(device, cases):
    v, f, p, want = cases["icosphere"]
    r = make(v, f, device)
    c, d, t = r.closest_point(T(p[0], device))
    assert c.shape == (3,) and d.shape == () and t.shape == () and c.dtype == torch.float32 and d.dtype == torch.float32 and t.dtype == torch.int32
    NC.assert_same_bits((c.cpu().numpy().reshape(1, 3), d.cpu().numpy().reshape(1), t.cpu().numpy().reshape(1)), tuple(x[:1] for x in want), "[3]")
    c, d, t = r.closest_point(T(p[:35].reshape(5, 7, 3), device))
    assert c.shape == (5, 7, 3) and d.shape == (5, 7) and t.shape == (5, 7)
    NC.assert_same_bits((c.cpu().numpy().reshape(-1, 3), d.cpu().numpy().reshape(-1), t.cpu().numpy().reshape(-1)), tuple(x[:35] for x in want), "[5, 7, 3]")
    wide = torch.zeros((200, 6), dtype=torch.float32, device=device)
    wide[:, 1:4] = T(p[:200], device)
    sliced = wide[::2, 1:4]
    assert not sliced.is_contiguous()
    c, d, t = r.closest_point(sliced)
    NC.assert_same_bits((c.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy()), tuple(x[:200:2] for x in want), "a non-contiguous slice")
    c, d, t = r.closest_point(T(p[:100].astype(np.float64), device))
    assert c.dtype == torch.float32
    NC.assert_same_bits((c.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy()), tuple(x[:100] for x in want), "float64 input")
    with pytest.raises(ValueError):
        r.closest_point(torch.from_numpy(p[:4]))
    with pytest.raises(ValueError):
        r.signed_distance(torch.from_numpy(p[:4]))
    with pytest.raises(ValueError):
        r.closest_point(T(p[:4, :2], device))


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["icosphere", "shells"])
def test_signed_distance_is_the_distance_with_the_sign_of_contains_points(device, cases, mesh):
    if mesh == "icosphere":
        v, f, p, _ = cases["icosphere"]
    else:
        v, f = W.nested_shells(3)
        p = NC.hash_points(2048, 7, [-1.05] * 3, [1.05] * 3)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    pt = T(p, device)
    _, dist, _ = r.closest_point(pt)
    # the default direction: points a ray pair leaves unresolved are retried along torch.rand(3) - 0.5 (ray_optix.py:273),
    # drawn here from the same seed and handed to the oracle
    torch.manual_seed(7)
    retry = (torch.rand(3) - 0.5).numpy()
    torch.manual_seed(7)
    before = CALLS["native"]
    sd = r.signed_distance(pt)
    assert CALLS["native"] == before + 1 and sd.shape == (len(p),) and sd.dtype == torch.float32
    assert torch.equal(sd.abs(), dist)
    inside = R.contains_points(p, None, _retry_dirs=iter([retry]))
    assert inside.any() and not inside.all()
    assert np.array_equal(sd.cpu().numpy() > 0, inside) and (dist > 0).all()          # positive inside (trimesh's convention)
    # an explicit direction is contains_points' argument
    direction = np.array([-0.3, 0.2, 0.9], np.float32)
    sd2 = r.signed_distance(pt, T(direction, device))
    assert torch.equal(sd2.abs(), dist) and np.array_equal(sd2.cpu().numpy() > 0, R.contains_points(p, direction))
    calls = []
    original = r.contains_points
    r.contains_points = lambda points, check_direction=None: (calls.append(check_direction), original(points, check_direction))[1]
    r.signed_distance(pt[:64].reshape(4, 16, 3), T(direction, device))
    assert len(calls) == 1 and torch.equal(calls[0].cpu(), torch.from_numpy(direction))
    # a batch shape: flattened for contains_points, reshaped afterwards
    got = r.signed_distance(pt[:64].reshape(4, 16, 3), T(direction, device))
    assert got.shape == (4, 16) and torch.equal(got.abs(), dist[:64].reshape(4, 16))
    assert np.array_equal(got.cpu().numpy().reshape(-1) > 0, R.contains_points(p[:64], direction))


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_refit_update_and_load(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    p = NC.hash_points(1500, 23, [-1.4] * 3, [1.6] * 3)
    r = make(v, f, device)
    check(r, v, f, p, device, "built")
    r.refit(T(v2, device))
    check(r, v2, f, p, device, "after a refit with moved vertices")
    check(r, v2, f, p, device, "after a refit, one stack entry", stack_entries=1)
    path = str(tmp_path / "mesh.npz")
    r.save(path)
    check(RayMeshIntersector.load(path, device=device), v2, f, p, device, "loaded")
    v3, f3, _ = NC.soup_with_degenerates()
    r.update_raw(T(v3, device), T(f3, device))
    check(r, v3, f3, p, device, "update_raw to another mesh")


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_the_first_call_of_a_fresh_intersector_can_be_captured(device):
    import nearest_sim
    import triro.backend.ops as hops
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=5, amplitude=0.05)
    v2 = (v * np.float32(1.6) + np.float32([0.3, 0.0, -0.2])).astype(np.float32)
    p1 = NC.hash_points(1000, 29, [-1.4] * 3, [1.4] * 3)
    p2 = NC.hash_points(1000, 31, [-2.0] * 3, [2.0] * 3)
    r = make(v, f, device)
    pt = T(p1, device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the call neither allocates nor synchronises
        out = hops.closest_point_native(r.as_wrapper, pt)
    for step, (vv, pp) in enumerate(((v, p1), (v, p2), (v2, p2), (v2, p1))):
        if step == 2:
            r.refit(T(vv, device))                      # moves the bounds
        pt.copy_(T(pp, device))
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(*out, what=f"graph replay {step}")
        NC.assert_same_bits(tuple(x.cpu().numpy() for x in out), nearest_sim.brute(vv, f, pp), f"graph replay {step}")
