"""within_any / within_count / faces_within / closest_point(max_distance) (libtriro_within.so: k_within<>, k_within_rows,
k_within_closest) against the host brute force.

The oracle of every comparison is tests/host_sim/within_sim.brute: the per-triangle function of csrc/tr_nearest.h over every
active triangle, kept where d2 <= R2, on the same float32 inputs -- itself pinned to an exact rational reference and to an
independent numpy evaluation by tests/test_within_cpu.py.  Comparisons are bit for bit (any, count, offsets, faces, distance,
closest, the bounded nearest), NaN and +Inf included.  Every native call of this module comes back through a wrapper that
runs poison.assert_written on its outputs (the autouse fixture `checked_native`); captured calls are checked after each
replay."""
import ctypes

import numpy as np
import pytest
import torch

import hostile_meshes as M
import nearest_cases as NC
import poison
import within_cases as WC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("within_native", "within_fill_native", "within_closest_native", "closest_point_native")
CALLS = {name: 0 for name in NATIVES}


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every native call: counted, and -- outside a graph capture -- all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    originals = {name: getattr(hops, name) for name in NATIVES}

    def wrap(name):
        original = originals[name]

        def call(*args, **kwargs):
            res = original(*args, **kwargs)
            CALLS[name] += 1
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
                poison.assert_written(*(res if isinstance(res, tuple) else (res,)), what=name)
            return res
        return call
    for name in NATIVES:
        setattr(hops, name, wrap(name))
    try:
        yield
    finally:
        for name, original in originals.items():
            setattr(hops, name, original)


def host(x):
    return None if x is None else x.cpu().numpy()


def dev_radius(radius, device):
    """a scalar stays a Python float (the `radius` argument of the entries), an array becomes the dense d_radius"""
    return float(radius) if np.ndim(radius) == 0 else T(np.asarray(radius, np.float32), device)


def native(r, p, radius, device, stack_entries=0, want_distance=True, want_closest=True, nearest_entries=None):
    """every entry once -> a within_sim.Result of numpy arrays"""
    import triro.backend.ops as hops
    import within_sim
    pt = T(np.ascontiguousarray(p, np.float32).reshape(-1, 3), device)
    rd = dev_radius(radius, device)
    any_ = hops.within_native(r.as_wrapper, pt, rd, "any", stack_entries)
    count = hops.within_native(r.as_wrapper, pt, rd, "count", stack_entries)
    offsets, face, distance, closest = hops.faces_within_native(r.as_wrapper, pt, rd, want_distance, want_closest, stack_entries)
    torch.cuda.synchronize()
    poison.assert_written(offsets, what="faces_within_native offsets")
    nearest = hops.within_closest_native(r.as_wrapper, pt, rd, stack_entries if nearest_entries is None else nearest_entries)
    assert any_.dtype == torch.bool and count.dtype == torch.int32 and offsets.dtype == torch.int64 and face.dtype == torch.int32
    return within_sim.Result(host(any_), host(count), host(offsets), host(face), host(distance), host(closest), tuple(host(x) for x in nearest))


def check(r, v, f, p, radius, device, what, want=None, **kw):
    import within_sim
    want = within_sim.brute(v, f, p, radius) if want is None else want
    got = native(r, p, radius, device, **kw)
    WC.assert_same(got, want, what)
    return got


@pytest.fixture(scope="module")
def cases():
    """{case: (v, f, p, [(label, radius, brute force)])}, computed once"""
    import within_sim
    out = {}
    for name, mk in WC.CASES.items():
        v, f, p = mk()
        out[name] = (v, f, p, [(label, r, within_sim.brute(v, f, p, r)) for label, r in WC.radii(v, len(p))])
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WC.CASES))
def test_kernels_match_the_brute_force_at_every_stack_limit(device, cases, name):
    v, f, p, rows = cases[name]
    r = make(v, f, device)
    if name == "deep":
        assert r.bvh_info()["depth"] > 32
    for label, radius, want in rows:
        for entries in (0, 1, 2, 3):
            check(r, v, f, p, radius, device, f"{name}, r = {label}, stack_entries {entries}", want=want, stack_entries=entries)


def test_kernels_match_the_host_walk_on_the_gpu_builders_tree(device, cases):
    import within_sim
    from sim import SimBVH
    v, f, p, rows = cases["icosphere"]
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    for label, radius, want in rows[2:]:
        for entries in (0, 1):
            walked = within_sim.walk(B, p, radius, entries)
            WC.assert_same(native(r, p, radius, device, stack_entries=entries), walked, f"GPU tree, r = {label}, stack_entries {entries}")
            WC.assert_same(walked, want, "host walk on the GPU tree against the brute force")


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_case():
    import within_sim
    v, f, _ = NC.icosphere()
    p = NC.hash_points(4133, 3, [-1.4] * 3, [1.4] * 3)
    radius = WC.hashed_radii(len(p), WC.extent(v), seed=1)
    return v, f, p, radius


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, tail_case, n):
    import within_sim
    v, f, p, radius = tail_case
    r = make(v, f, device)
    want = within_sim.brute(v, f, p[:n], radius[:n])
    got = check(r, v, f, p[:n], radius[:n], device, f"{n} points", want=want)
    total = int(want.offsets[-1])
    assert got.any.shape == (n,) and got.count.shape == (n,) and got.offsets.shape == (n + 1,)
    assert got.faces.shape == (total,) and got.distance.shape == (total,) and got.closest.shape == (total, 3)
    assert got.nearest[0].shape == (n, 3) and got.nearest[1].shape == (n,) and got.nearest[2].shape == (n,)
    # each optional output left out in turn (every row 0 .. total of what is given is written: checked_native)
    g = check(r, v, f, p[:n], radius[:n], device, f"{n} points, no distance", want=want, want_distance=False)
    assert g.distance is None and g.closest is not None
    g = check(r, v, f, p[:n], radius[:n], device, f"{n} points, no closest", want=want, want_closest=False)
    assert g.closest is None and g.distance is not None
    g = check(r, v, f, p[:n], radius[:n], device, f"{n} points, faces only", want=want, want_distance=False, want_closest=False)
    assert g.distance is None and g.closest is None
    # one radius for all points, and the bounded nearest without its optional outputs
    import triro.backend.ops as hops
    scalar = float(np.float32(0.25 * WC.extent(v)))
    want1 = within_sim.brute(v, f, p[:n], scalar)
    check(r, v, f, p[:n], scalar, device, f"{n} points, one radius", want=want1)
    c, d, t = hops.within_closest_native(r.as_wrapper, T(p[:n], device), scalar, want_closest=False, want_distance=False)
    assert c is None and d is None and np.array_equal(host(t), want1.nearest[2])


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_meshes_without_a_hierarchy(device):
    v, f = W.two_triangles()
    p = np.concatenate([NC.hash_points(300, 5, [-0.8, -0.8, -1.4], [0.8, 0.8, 0.4]),
                        np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.5, -0.5, 0.0], [np.nan, 0.0, 0.0]], np.float32)])
    for nt in (2, 1, 0):
        vv, ff = v[:3 * nt], f[:nt]
        r = make(vv, ff, device)
        seen = set()
        for label, radius in WC.radii(v, len(p)):
            for entries in (0, 1):
                got = check(r, vv, ff, p, radius, device, f"{nt} triangle(s), r = {label}", stack_entries=entries)
            seen |= set(np.unique(got.count))
            assert got.count[-1] == 0 and got.nearest[2][-1] == -1
        assert seen == set(range(nt + 1))
        if nt == 0:
            assert len(got.faces) == 0 and (got.nearest[2] == -1).all() and np.isposinf(got.nearest[1]).all() and np.isnan(got.nearest[0]).all()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_hostile_points_and_radii(device):
    import within_sim
    v, f, _ = NC.icosphere()
    r = make(v, f, device)
    ordinary = NC.hash_points(256, 17, [-1.3] * 3, [1.3] * 3)
    p = ordinary.copy()
    radius = np.full(len(p), 0.75, np.float32)
    with np.errstate(over="ignore"):
        bad_r = np.array([np.nan, -1.0, -np.inf, -1e-45, -0.0, np.inf, 1e-45, 1e-39, 3e38, 0.0, 0.5, 3.4028235e38], np.float32)
    radius[80:80 + len(bad_r)] = bad_r
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p[5 + 7 * k, axis] = bad
            k += 1
    p[70] = [3e38, 3e38, 3e38]; p[71] = [-3e38, 0.1, 3e38]; p[72] = [0, 0, -3e38]; p[73] = [3e38, 0, 0]
    p[74] = [2.0 ** 60, 0, 0]; p[75] = [-(2.0 ** 60), 2.0 ** 60, 0.5]
    p[76] = [1e-45, -1e-40, 3e-39]; p[77] = [1e-39, 0, 0]; p[78] = [0, 0, 0]
    radius[70:76] = [np.inf, 3e38, 3e38, 1.0, 2.0 ** 61, np.inf]
    p[128:192] = np.nan                                   # a whole wave of invalid points ...
    p = np.concatenate([p, ordinary[:128], ordinary[:70]])
    radius = np.concatenate([radius, np.full(128, np.nan, np.float32), np.full(70, 0.75, np.float32)])      # ... and a whole block of invalid radii
    radius[256 + 64:256 + 128] = -1.0
    for entries in (0, 1):
        got = check(r, v, f, p, radius, device, f"hostile queries, stack_entries {entries}", stack_entries=entries)
    bad = ~(np.isfinite(p).all(1) & (radius >= 0))
    assert bad.sum() == 9 + 64 + 4 + 128
    c, d, t = got.nearest
    assert not got.any[bad].any() and not got.count[bad].any()
    assert (t[bad] == -1).all() and np.isposinf(d[bad]).all() and np.isnan(c[bad]).all()
    assert got.count[70] == len(f) and np.isposinf(d[70]) and t[70] >= 0          # within +Inf, its distance beyond the float range
    assert got.count[85] == len(f) and got.count[88] == len(f) and got.count[84] == 0 and got.count[89] == 0
    # the same hostile radius for every point, as the scalar argument
    for scalar in (np.nan, -1.0, -0.0, np.inf, 3e38, 1e-45):
        g = check(r, v, f, ordinary, np.float32(scalar), device, f"radius {scalar!r} for all points")
        if not scalar >= 0:
            assert not g.any.any() and (g.nearest[2] == -1).all()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_hostile_meshes(device, name, seed):
    c = M.case(name, seed)
    fa, _ = M.active_faces(c.v, c.f)
    ext = WC.extent(c.v[np.unique(fa)]) if len(fa) else 1.0
    r = make(c.v, c.f, device)
    for radius in (np.float32(0.25 * ext), np.float32(np.inf), WC.hashed_radii(len(c.p), 2 * ext, seed=3)):
        for entries in (0, 1, 3):
            got = check(r, c.v, c.f, c.p, radius, device, f"{c.name}, stack_entries {entries}", stack_entries=entries)
        assert not c.inactive[got.faces].any()
        if np.ndim(radius) == 0 and np.isinf(radius):
            assert (got.count == len(fa)).all()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_cube_lattice_matches_the_exact_reference(device):
    v, f, _ = NC.cube()
    r = make(v, f, device)
    at = WC.check_cube_lattice(lambda p, radius: native(r, p, radius, device, stack_entries=2), "GPU")
    assert at == [540, 540, 540, 540]


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_fill_with_counts_of_a_smaller_radius_stays_inside_its_rows(device, cases):
    """the caller's error: count / offsets computed for a smaller radius (and a total cut short) handed to a fill at a larger
    one.  Wrong rows are allowed; a write outside the rows of those counts is not: guard rows on both sides stay poisoned."""
    import triro.backend.ops as hops
    import within_sim
    v, f, p, rows = cases["soup"]
    r = make(v, f, device)
    small, large = rows[2][2], rows[4][2]              # 1/8 and 1/2 of the extent
    assert (large.count >= small.count).all() and large.offsets[-1] > 4 * small.offsets[-1] > 0
    lib = hops.get_within_module()
    pt = T(p, device)
    count, offsets = T(small.count, device), T(small.offsets[:-1].copy(), device)
    G = 4096
    for total in (int(small.offsets[-1]), int(small.offsets[-1]) - 37):
        face = poison.poisoned((G + total + G,), torch.int32, device)
        slot = poison.poisoned((G + total + G,), torch.int32, device)
        dist = poison.poisoned((G + total + G,), torch.float32, device)
        clo = poison.poisoned((G + total + G, 3), torch.float32, device)
        for entries in (0, 1):
            with torch.cuda.device(device):
                rc = lib.tr_within_fill(r.as_wrapper._inner, pt.data_ptr(), len(p), None, float(rows[4][1]), count.data_ptr(), offsets.data_ptr(),
                                        total, face.data_ptr() + 4 * G, dist.data_ptr() + 4 * G, clo.data_ptr() + 12 * G, slot.data_ptr() + 4 * G,
                                        entries, hops._stream_ptr(device))
            assert rc == 0, hops.get_module().tr_last_error()
            torch.cuda.synchronize()
            for name, t in (("face", face), ("slot", slot), ("distance", dist), ("closest", clo)):
                stale = poison.stale_mask(t).reshape(len(t), -1).all(1)
                assert stale[:G].all() and stale[G + total:].all(), f"{name}: a guard row was written (total {total}, stack_entries {entries})"
                assert not stale[G:G + total].any(), f"{name}: a row inside was not written"
            # wrong rows, but rows: each point got faces that are within the large radius, ascending, with their own distances
            got = host(face)[G:G + total]
            gd = host(dist)[G:G + total]
            for i in (0, 1, 2, len(p) // 2, len(p) - 1):
                a, b = int(small.offsets[i]), min(int(small.offsets[i + 1]), total)
                mine = large.faces[large.offsets[i]:large.offsets[i + 1]]
                assert (np.diff(got[a:b]) > 0).all() and np.isin(got[a:b], mine).all()
                at = large.offsets[i] + np.searchsorted(mine, got[a:b])
                assert np.array_equal(NC.bits(gd[a:b]), NC.bits(large.distance[at]))


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_python_methods_batch_shapes_and_input_types(device, cases):
    import within_sim
    v, f, p, rows = cases["icosphere"]
    label, radius, want = rows[3]
    radius = float(radius)
    r = make(v, f, device)
    a, n, (c, d, t) = r.within_any(T(p[0], device), radius), r.within_count(T(p[0], device), radius), r.closest_point(T(p[0], device), max_distance=radius)
    assert a.shape == () and a.dtype == torch.bool and n.shape == () and n.dtype == torch.int32
    assert c.shape == (3,) and d.shape == () and t.shape == () and c.dtype == torch.float32 and d.dtype == torch.float32 and t.dtype == torch.int32
    assert bool(a) == bool(want.any[0]) and int(n) == int(want.count[0]) and int(t) == int(want.nearest[2][0])
    out = r.faces_within(T(p[0], device), radius, return_distance=True, return_closest=True)
    assert len(out) == 4 and out[0].shape == (2,) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32
    assert np.array_equal(host(out[1]), want.faces[:want.count[0]])

    def flat(points, rad, **kw):
        """the four methods on one batch -> a Result of flat numpy arrays (+ the batch shapes seen)"""
        a, n = r.within_any(points, rad), r.within_count(points, rad)
        off, tri, dist, clo = r.faces_within(points, rad, return_distance=True, return_closest=True)
        c, d, t = r.closest_point(points, max_distance=rad)
        b = tuple(points.shape[:-1])
        assert a.shape == b and n.shape == b and d.shape == b and t.shape == b and c.shape == b + (3,)
        return within_sim.Result(host(a).reshape(-1), host(n).reshape(-1), host(off), host(tri), host(dist), host(clo),
                                 (host(c).reshape(-1, 3), host(d).reshape(-1), host(t).reshape(-1)))
    WC.assert_same(flat(T(p[:35].reshape(5, 7, 3), device), radius), within_sim.brute(v, f, p[:35], radius), "[5, 7, 3]")
    wide = torch.zeros((200, 6), dtype=torch.float32, device=device)
    wide[:, 1:4] = T(p[:200], device)
    sliced = wide[::2, 1:4]
    assert not sliced.is_contiguous()
    WC.assert_same(flat(sliced, radius), within_sim.brute(v, f, p[:200:2], radius), "a non-contiguous slice")
    WC.assert_same(flat(T(p[:100].astype(np.float64), device), radius), within_sim.brute(v, f, p[:100], radius), "float64 input")
    # radii that broadcast: one per row of a [5, 7] batch, a 0-dim tensor, a float64 tensor, a numpy array
    per_row = np.float32([0.1, 0.25, 0.5, 0.0, np.inf])
    want_b = within_sim.brute(v, f, p[:35], np.repeat(per_row, 7))
    WC.assert_same(flat(T(p[:35].reshape(5, 7, 3), device), T(per_row.reshape(5, 1), device)), want_b, "a [5, 1] radius on a [5, 7] batch")
    WC.assert_same(flat(T(p[:35].reshape(5, 7, 3), device), T(per_row.astype(np.float64).reshape(5, 1), device)), want_b, "a float64 radius")
    WC.assert_same(flat(T(p[:35].reshape(5, 7, 3), device), per_row.reshape(5, 1)), want_b, "a numpy radius")
    WC.assert_same(flat(T(p[:35], device), torch.tensor(radius, device=device)), within_sim.brute(v, f, p[:35], radius), "a 0-dim radius")
    # refusals
    for call in (lambda: r.within_any(torch.from_numpy(p[:4]), radius), lambda: r.within_count(torch.from_numpy(p[:4]), radius),
                 lambda: r.faces_within(torch.from_numpy(p[:4]), radius), lambda: r.closest_point(torch.from_numpy(p[:4]), max_distance=radius),
                 lambda: r.within_any(T(p[:4, :2], device), radius), lambda: r.within_count(T(p[:4], device), T(per_row, device)),
                 lambda: r.closest_point(T(p[:4], device), max_distance=T(per_row[:3], device))):
        with pytest.raises(ValueError):
            call()
    # max_distance=None is today's path: the same launch, the same bits
    before = dict(CALLS)
    c0, d0, t0 = r.closest_point(T(p, device))
    c1, d1, t1 = r.closest_point(T(p, device), max_distance=None)
    assert CALLS["closest_point_native"] == before["closest_point_native"] + 2 and CALLS["within_closest_native"] == before["within_closest_native"]
    NC.assert_same_bits((host(c1), host(d1), host(t1)), (host(c0), host(d0), host(t0)), "max_distance=None")
    # one count launch, one fill
    before = dict(CALLS)
    r.faces_within(T(p, device), radius)
    assert CALLS["within_native"] == before["within_native"] + 1 and CALLS["within_fill_native"] == before["within_fill_native"] + 1


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_refit_update_and_load(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    p = NC.hash_points(1500, 23, [-1.4] * 3, [1.6] * 3)
    radius = WC.hashed_radii(len(p), 1.5, seed=2)
    r = make(v, f, device)
    check(r, v, f, p, radius, device, "built")
    r.refit(T(v2, device))
    check(r, v2, f, p, radius, device, "after a refit with moved vertices")
    check(r, v2, f, p, 0.4, device, "after a refit, one stack entry", stack_entries=1)
    path = str(tmp_path / "mesh.npz")
    r.save(path)
    check(RayMeshIntersector.load(path, device=device), v2, f, p, radius, device, "loaded")
    v3, f3, _ = NC.soup_with_degenerates()
    r.update_raw(T(v3, device), T(f3, device))
    check(r, v3, f3, p, radius, device, "update_raw to another mesh")


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_the_first_calls_of_a_fresh_intersector_can_be_captured(device):
    import triro.backend.ops as hops
    import within_sim
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=5, amplitude=0.05)
    v2 = (v * np.float32(1.6) + np.float32([0.3, 0.0, -0.2])).astype(np.float32)
    p1 = NC.hash_points(1000, 29, [-1.4] * 3, [1.4] * 3)
    p2 = NC.hash_points(1000, 31, [-2.0] * 3, [2.0] * 3)
    radius = WC.hashed_radii(1000, 1.2, seed=4)
    n = len(p1)
    r = make(v, f, device)
    pt, rd = T(p1, device), T(radius, device)
    # the rows of the captured fill: preallocated for the largest total of the four steps, counts and offsets refreshed per step
    steps = ((v, p1), (v, p2), (v2, p2), (v2, p1))
    wants = [within_sim.brute(vv, f, pp, radius) for vv, pp in steps]
    rows = max(int(w.offsets[-1]) for w in wants) + 64
    count_in = torch.zeros(n, dtype=torch.int32, device=device)
    offsets_in = torch.zeros(n, dtype=torch.int64, device=device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the calls neither allocate nor synchronise
        any_ = hops.within_native(r.as_wrapper, pt, rd, "any")
        count = hops.within_native(r.as_wrapper, pt, rd, "count")
        nearest = hops.within_closest_native(r.as_wrapper, pt, rd)
        face, dist, clo = hops.within_fill_native(r.as_wrapper, pt, rd, count_in, offsets_in, rows, want_distance=True, want_closest=True)
    for step, ((vv, pp), want) in enumerate(zip(steps, wants)):
        if step == 2:
            r.refit(T(vv, device))                      # moves the bounds
        pt.copy_(T(pp, device))
        count_in.copy_(T(want.count, device))
        offsets_in.copy_(T(want.offsets[:-1].copy(), device))
        graph.replay()
        torch.cuda.synchronize()
        total = int(want.offsets[-1])
        assert 0 < total <= rows - 64
        poison.assert_written(any_, count, *nearest, face[:total], dist[:total], clo[:total], what=f"graph replay {step}")
        for name, t in (("face", face), ("distance", dist), ("closest", clo)):
            assert poison.stale_mask(t[total:]).all(), f"graph replay {step}: {name} rows beyond the total were written"
        got = within_sim.Result(host(any_), host(count), want.offsets, host(face[:total]), host(dist[:total]), host(clo[:total]),
                                tuple(host(x) for x in nearest))
        WC.assert_same(got, want, f"graph replay {step}")
