"""contains_points as one launch (libtriro_points.so, k_contains_points<COMPACT, DEEP>) against the oracle.

Every comparison is exact.  Four of them, on every case unless it says otherwise:
  (a) inside / broken / counts of tr_contains_points against the oracle's intersects_count on (p, +-d) and the decision
      rule of ray_optix.py:265-268, and RayMeshIntersector.contains_points against the oracle's contains_points;
  (b) counts against hops.intersects_count on the same 2n rays (the generic count launch);
  (c) contains_points with native_contains = True against False, under the same _retry_direction;
  (d) summary against the sums of the flags.
Every native call of this module comes back through a wrapper that runs poison.assert_written on inside, broken, counts
and summary (the autouse fixture `checked_native`); the captured call is checked after each replay."""
import os

import numpy as np
import pytest
import torch

import hostile_rays
import poison
import workloads as W
from launch_options import options
from oracle.oracle import OracleIntersector
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

DEFAULT_DIRECTION = np.array([0.4395064455, 0.617598629942, 0.652231566745], np.float32)
RETRY = np.array([0.21, -0.43, 0.37], np.float32)
CALLS = {"native": 0}


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every native call: counted, and -- outside a graph capture -- all four outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    original = hops.contains_points_native

    def call(*args, **kwargs):
        res = original(*args, **kwargs)
        CALLS["native"] += 1
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize()
            poison.assert_written(*res, what="contains_points_native (inside, broken, counts, summary)")
        return res
    hops.contains_points_native = call
    try:
        yield
    finally:
        hops.contains_points_native = original


def decision(p, box, cp, cm):
    """ray_optix.py:238-240, 265-268 on the oracle's counts: (in_box, inside, broken)"""
    in_box = (p > box[0]).all(1) & (p < box[1]).all(1)
    odd = (cp & 1).astype(bool) & (cm & 1).astype(bool)
    return in_box, in_box & odd, ~odd & ((cp == 0) | (cm == 0))


def check_all(r, R, p, d, device, what, addressing=1, box=None, retry=True):
    """(a) - (d) for points p [n, 3] and direction d on intersector r / oracle R"""
    import triro.backend.ops as hops
    p = np.ascontiguousarray(p, np.float32)
    n = len(p)
    pt, dt = T(p, device), T(d, device)
    box = R.mesh_aabb if box is None else box
    assert hops.contains_addressing(r.as_wrapper) == addressing, what
    inside, broken, counts, summary = hops.contains_points_native(r.as_wrapper, pt, dt, T(box[0], device), T(box[1], device),
                                                                  want_counts=True)
    inside, broken, counts, summary = (x.cpu().numpy() for x in (inside, broken, counts, summary))
    dirs = np.tile(d, (n, 1)).astype(np.float32)
    # (a) the oracle
    cp, cm = R.intersects_count(p, dirs), R.intersects_count(p, -dirs)
    in_box, want_inside, want_broken = decision(p, box, cp, cm)
    assert np.array_equal(counts, np.stack([cp, cm]).reshape(2, n)), f"{what}: counts differ from the oracle"
    assert np.array_equal(inside, want_inside), f"{what}: inside"
    assert np.array_equal(broken, want_broken), f"{what}: broken"
    # (d) the summary
    assert summary.tolist() == [int(in_box.sum()), int(want_broken.sum())], f"{what}: summary"
    # (b) the generic count launch on the same rays
    both = hops.intersects_count(r.as_wrapper, torch.cat([pt, pt]), torch.cat([dt.expand(n, 3), -dt.expand(n, 3)]).contiguous())
    assert np.array_equal(both.cpu().numpy().reshape(2, n), counts), f"{what}: counts differ from intersects_count"
    # without counts the flags are the same
    i2, b2, c2, s2 = hops.contains_points_native(r.as_wrapper, pt, dt, T(box[0], device), T(box[1], device))
    assert c2 is None and np.array_equal(i2.cpu().numpy(), inside) and np.array_equal(b2.cpu().numpy(), broken), what
    assert s2.tolist() == summary.tolist(), what
    # (c) the class, native against torch, explicit direction (the all-False quirk) and default direction with a retry
    same_box = box is R.mesh_aabb
    if same_box:
        assert r.native_contains is True
        before = CALLS["native"]
        got_n = r.contains_points(pt, dt)
        assert CALLS["native"] > before, f"{what}: the native route was not taken"
        r.native_contains = False
        try:
            before = CALLS["native"]
            got_t = r.contains_points(pt, dt)
            assert CALLS["native"] == before, f"{what}: native_contains = False still took the native route"
            assert torch.equal(got_n, got_t), f"{what}: explicit direction, native against torch"
            assert np.array_equal(got_n.cpu().numpy(), R.contains_points(p, d)), f"{what}: explicit direction against the oracle"
            if retry:
                got_t = r.contains_points(pt, None, _retry_direction=torch.from_numpy(RETRY))
        finally:
            r.native_contains = True
        if retry:
            got_n = r.contains_points(pt, None, _retry_direction=torch.from_numpy(RETRY))
            assert got_n.dtype == torch.bool and got_n.shape == (n,)
            assert torch.equal(got_n, got_t), f"{what}: default direction with a retry, native against torch"
            assert np.array_equal(got_n.cpu().numpy(), R.contains_points(p, None, _retry_dirs=iter([RETRY]))), f"{what}: retry against the oracle"
    return inside, broken, counts, summary


def lattice(lo, hi, k):
    ax = [np.linspace(lo[a], hi[a], k, dtype=np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def hash_points(n, seed, lo, hi):
    return np.ascontiguousarray(W.hash_rays(n, seed, np.asarray(lo, np.float32), np.asarray(hi, np.float32))[0], np.float32)


def test_cube_lattice_with_exact_ties(device):
    """9^3 lattice points of the golden cube's box, bounds included: points ON faces, edges and vertices (strict box compares:
    outside), rays through edges and vertices (exact ties of the predicate).  729 points: a partial wave, a partial block."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "cube_axis_rays.npz"))
    v, f = g["vertices"], g["faces"]
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    p = lattice(v.min(0), v.max(0), 9)
    assert len(p) == 729
    for d in (DEFAULT_DIRECTION, np.array([0, 0, 1], np.float32)):
        inside, broken, counts, summary = check_all(r, R, p, d, device, f"cube lattice, direction {d}")
        assert int(summary[0]) == 7 ** 3                     # the strict compares keep the 7^3 interior lattice points
    assert inside.sum() > 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129])
def test_tails_of_the_lane_and_block_indexing(device, n):
    v, f = W.icosphere(2)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    p = hash_points(129, 3, [-1.1] * 3, [1.1] * 3)[:n]
    inside, broken, counts, summary = check_all(r, R, p, DEFAULT_DIRECTION, device, f"icosphere, {n} points")
    assert inside.shape == (n,) and counts.shape == (2, n)
    if n >= 63:
        assert inside.any() and not inside.all()


def test_two_triangles_and_a_mesh_without_a_hierarchy(device):
    v, f = W.two_triangles()
    p = np.concatenate([hash_points(300, 5, [-0.6, -0.6, -1.4], [0.6, 0.6, 0.4]),
                        np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.0, 0.0, -1.5]], np.float32)])
    for nt in (2, 1):
        vv, ff = v[:3 * nt], f[:nt]
        r, R = make(vv, ff, device), OracleIntersector(vv, ff, 1)
        for d in (np.array([0, 0, 1], np.float32), DEFAULT_DIRECTION):
            inside, broken, counts, summary = check_all(r, R, p, d, device, f"{nt} triangle(s), direction {d}")
        assert counts.max() >= 1
    # between the two triangles a vertical line meets one each way; the flat box of ONE triangle holds no point at all
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    inside, *_ = check_all(r, R, p, np.array([0, 0, 1], np.float32), device, "two triangles, vertical")
    assert inside[300]


def test_nested_shells_count_up_to_eight(device):
    v, f = W.nested_shells(3)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    p = hash_points(4096, 7, [-1.05] * 3, [1.05] * 3)
    inside, broken, counts, summary = check_all(r, R, p, DEFAULT_DIRECTION, device, "nested shells")
    assert counts.max() == 8 and set(np.unique(counts & 1)) == {0, 1} and inside.any() and (~inside).any()


def test_open_soup_breaks_points_and_retries(device):
    """an open mesh: broken points, the retry recursion under _retry_direction, and -- with an explicit direction -- the
    reference's all-False answer (ray_optix.py:272-279)"""
    v, f = W.random_soup(400)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    p = hash_points(4096, 9, v.min(0), v.max(0))
    inside, broken, counts, summary = check_all(r, R, p, DEFAULT_DIRECTION, device, "soup, default direction")
    assert broken.any() and inside.any() and int(summary[0]) > 0
    d = np.array([0.3, -0.5, 0.8], np.float32)
    inside, broken, counts, summary = check_all(r, R, p, d, device, "soup, explicit direction", retry=False)
    assert broken.any() and inside.any()
    assert not r.contains_points(T(p, device), T(d, device)).any()        # the quirk: unresolved points, explicit direction
    # no point in the box: zeros, and no retry direction is drawn (the global generator stays where it is)
    far = p + np.float32(10.0)
    state = torch.get_rng_state()
    assert not r.contains_points(T(far, device)).any()
    assert torch.equal(torch.get_rng_state(), state)


def test_every_addressing_flavour_matches_the_oracle(device):
    """deep (a hierarchy of more than 32 levels), generic (option compact = 0) and compact on the same kind of points"""
    v, f = W.deep_tree_mesh(3000)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    assert r.bvh_info()["depth"] > 32
    p = np.concatenate([hash_points(1500, 13, [-0.2] * 3, [1.2] * 3),
                        np.array([[1e-10, 1e-10, 0.5], [3e-10, 2e-10, -0.5]], np.float32)])       # above / below the pile of 3000
    inside, broken, counts, summary = check_all(r, R, p, np.array([0, 0, 1], np.float32), device, "deep tree", addressing=2)
    assert counts.max() >= 1
    check_all(r, R, p, DEFAULT_DIRECTION, device, "deep tree, default direction", addressing=2)
    v, f = W.nested_shells(3)
    R = OracleIntersector(v, f, 1)
    p = hash_points(4096, 7, [-1.05] * 3, [1.05] * 3)
    with options(compact=0):
        r = make(v, f, device)
        g_inside, _, g_counts, _ = check_all(r, R, p, DEFAULT_DIRECTION, device, "shells, generic addressing", addressing=0)
    c_inside, _, c_counts, _ = check_all(r, R, p, DEFAULT_DIRECTION, device, "shells, compact addressing", addressing=1)
    assert np.array_equal(g_inside, c_inside) and np.array_equal(g_counts, c_counts) and g_counts.max() == 8


def test_hostile_points(device):
    """origins of tests/hostile_rays.py as points -- NaN, +-Inf, denormal, 3.4e38, 2^60 components among ordinary ones -- and
    points far out along the direction, which the ray set-up anchors like the count path's rays"""
    v, f, o, d, target, _ = hostile_rays.scene("shells", 1024)
    batch = hostile_rays.hostile_batch(o, d, target, "interleaved", per=65)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    inner = hash_points(512, 17, [-0.9] * 3, [0.9] * 3)
    far = np.concatenate([inner[k::4] - np.float32(t) * DEFAULT_DIRECTION for k, t in enumerate((1e2, 1e4, 3e6, 2e7))]).astype(np.float32)
    p = np.concatenate([batch.o, far, inner])
    bad = ~np.isfinite(p).all(1)
    assert bad.sum() >= 100 and np.isnan(p).any() and np.isinf(p).any() and (np.abs(p) > 1e38).any() and (np.abs(p) == 2.0 ** 60).any()
    assert ((p != 0) & (np.abs(p) < 1e-38)).any()
    inside, broken, counts, summary = check_all(r, R, p, DEFAULT_DIRECTION, device, "hostile points")
    assert not counts[:, bad].any() and not inside[bad].any() and broken[bad].all()      # invalid rays count 0; a NaN is in no box
    m = len(batch.o)
    assert counts[0, m:m + 3 * 128].max() >= 2 and not counts[1, m:m + len(far)].any()     # anchored: the far points see the shells ahead, nothing behind
    assert not counts[0, m + 3 * 128:m + len(far)].any()                                   # 2e7 away: beyond the reference's tmax
    assert inside[m + len(far):].any()
    check_all(r, R, p, np.array([0, 0, -1], np.float32), device, "hostile points, axis direction", retry=False)


def test_the_box_comes_from_the_arguments(device):
    """mesh_aabb overridden through the setter: the native route passes the caller's box, not the handle's bounds"""
    v, f = W.icosphere(3)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    p = hash_points(2000, 21, [-1.0] * 3, [1.0] * 3)
    full = r.contains_points(T(p, device))
    lo, hi = np.array([-0.25, -0.5, -1.0], np.float32), np.array([0.5, 0.25, 0.125], np.float32)
    r.mesh_aabb = (T(lo, device), T(hi, device))
    R.mesh_aabb = (lo, hi)
    inside, broken, counts, summary = check_all(r, R, p, DEFAULT_DIRECTION, device, "overridden box")
    in_small = (p > lo).all(1) & (p < hi).all(1)
    assert 0 < in_small.sum() < len(p) and int(summary[0]) == int(in_small.sum())
    assert np.array_equal(inside, full.cpu().numpy() & in_small) and full.cpu().numpy()[~in_small].any()
    # bounds that are not float32 keep the torch statements (they compare in the bounds' own type)
    r.mesh_aabb = (T(lo, device).double() + 1e-12, T(hi, device).double())
    before = CALLS["native"]
    got64 = r.contains_points(T(p, device), T(DEFAULT_DIRECTION, device))
    assert CALLS["native"] == before and torch.equal(got64, r._contains_points_torch(T(p, device), T(DEFAULT_DIRECTION, device)))
    r.mesh_aabb = (T(lo, device), T(hi, device))
    # and no box at all: every point passes
    import triro.backend.ops as hops
    i3, b3, _, s3 = hops.contains_points_native(r.as_wrapper, T(p, device), T(DEFAULT_DIRECTION, device), None, None)
    assert int(s3[0]) == len(p) and np.array_equal(i3.cpu().numpy(), full.cpu().numpy())


def test_lifecycle_refit_update_load_and_a_captured_call(device, tmp_path):
    """refit that moves the bounds (the grid frame and the anchor box change), update_raw, save / load; one capture of the
    native call on a side stream (h_summary2 == NULL: no synchronisation, no allocation), replayed after each refit"""
    import triro.backend.ops as hops
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(3)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    p = hash_points(3000, 23, [-1.4] * 3, [1.6] * 3)
    r = make(v, f, device)
    check_all(r, OracleIntersector(v, f, 1), p, DEFAULT_DIRECTION, device, "built")
    pt, dt = T(p, device), T(DEFAULT_DIRECTION, device)
    lo, hi = (t.clone() for t in r.mesh_aabb)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        hops.contains_points_native(r.as_wrapper, pt, dt, lo, hi, want_counts=True)      # warm-up on the capture stream
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = hops.contains_points_native(r.as_wrapper, pt, dt, lo, hi, want_counts=True)
    dirs = np.tile(DEFAULT_DIRECTION, (len(p), 1))
    for vv in (v, v2, v):
        r.refit(T(vv, device))
        R = OracleIntersector(vv, f, 1)
        lo.copy_(T(R.mesh_aabb[0], device)); hi.copy_(T(R.mesh_aabb[1], device))
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(*out, what="graph replay after a refit")
        cp, cm = R.intersects_count(p, dirs), R.intersects_count(p, -dirs)
        in_box, want_inside, want_broken = decision(p, R.mesh_aabb, cp, cm)
        assert np.array_equal(out[2].cpu().numpy(), np.stack([cp, cm])), "replay: counts"
        assert np.array_equal(out[0].cpu().numpy(), want_inside) and np.array_equal(out[1].cpu().numpy(), want_broken)
        assert out[3].tolist() == [int(in_box.sum()), int(want_broken.sum())]
        check_all(r, R, p, DEFAULT_DIRECTION, device, "after a refit")
    r.refit(T(v2, device))
    check_all(r, OracleIntersector(v2, f, 1), p, DEFAULT_DIRECTION, device, "refit to other bounds")
    path = str(tmp_path / "mesh.npz")
    r.save(path)
    loaded = RayMeshIntersector.load(path, device=device)
    check_all(loaded, OracleIntersector(v2, f, 1), p, DEFAULT_DIRECTION, device, "loaded")
    v3, f3 = W.nested_shells(2)
    r.update_raw(T(v3, device), T(f3, device))
    check_all(r, OracleIntersector(v3, f3, 1), p, DEFAULT_DIRECTION, device, "update_raw")
