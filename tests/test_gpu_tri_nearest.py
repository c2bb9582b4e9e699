"""triangles_nearest / mesh_distance (libtriro_tri_nearest.so: k_triangles_nearest) against the host brute force.

The oracle of every comparison is tests/host_sim/tri_nearest_sim.brute: the distance function of csrc/tr_tri_nearest.h over
every active triangle, on the same float32 inputs -- itself pinned to an exact evaluation in integers and fractions and to an
independent numpy evaluation by tests/test_tri_nearest_cpu.py, and once more to the exact one here on the GPU's own results.
Comparisons are bit for bit (tri, distance, closest_mesh, closest_query): there is no tolerance.  Every native call of this
module comes back through a wrapper that runs poison.assert_written on its outputs (the autouse fixture `checked_native`);
captured calls are checked after each replay."""
import itertools

import numpy as np
import pytest
import torch

import hostile_meshes as M
import nearest_cases as NC
import poison
import tri_nearest_cases as TN
import tris_cases as TC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVE = "triangles_nearest_native"
CALLS = []          # the max_distance of every native call, in order


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every native call: recorded, and -- outside a graph capture -- all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    original = getattr(hops, NATIVE)

    def call(accel_structure, tri, max_distance=None, *args, **kwargs):
        res = original(accel_structure, tri, max_distance, *args, **kwargs)
        CALLS.append(max_distance)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize()
            poison.assert_written(*res, what=NATIVE)
        return res
    setattr(hops, NATIVE, call)
    try:
        yield
    finally:
        setattr(hops, NATIVE, original)


def host(x):
    return None if x is None else x.cpu().numpy()


def native(r, tri, device, max_distance=None, stack_entries=0, want=(True, True, True)):
    """one launch -> (tri, distance, closest_mesh, closest_query) of numpy arrays (None where not wanted)"""
    import tri_nearest_sim
    import triro.backend.ops as hops
    tt = T(tri_nearest_sim.triangles(tri).reshape(-1, 3, 3), device)
    if isinstance(max_distance, np.ndarray):
        max_distance = T(max_distance.astype(np.float32), device)
    res = hops.triangles_nearest_native(r.as_wrapper, tt, max_distance, stack_entries, want)
    torch.cuda.synchronize()
    assert res[0].dtype == torch.int32 and all(x is None or x.dtype == torch.float32 for x in res[1:])
    return tuple(host(x) for x in res)


def check(r, v, f, tri, device, what, want=None, max_distance=None, **kw):
    import tri_nearest_sim
    want = tri_nearest_sim.brute(v, f, tri, max_distance) if want is None else want
    got = native(r, tri, device, max_distance, **kw)
    TN.assert_same(got, want, what)
    return got


@pytest.fixture(scope="module")
def cases():
    """{case: (v, f, triangles, brute force, bound, bounded brute force)}: every query set of the case as one batch, computed
    once"""
    import tri_nearest_sim
    out = {}
    for name, mk in TN.CASES.items():
        v, f, _ = mk()
        tri = TN.all_queries(v, f)
        free = tri_nearest_sim.brute(v, f, tri)
        r = TN.half_bound(free[1])
        out[name] = (v, f, tri, free, r, tri_nearest_sim.brute(v, f, tri, r))
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TN.CASES))
def test_kernel_matches_the_brute_force_at_every_stack_limit(device, cases, name):
    v, f, tri, free, bound, bounded = cases[name]
    r = make(v, f, device)
    if name == "deep":
        assert r.bvh_info()["depth"] > 32
    for entries in (0, 1, 2):
        check(r, v, f, tri, device, f"{name}, stack_entries {entries}", want=free, stack_entries=entries)
        check(r, v, f, tri, device, f"{name}, within {bound}, stack_entries {entries}", want=bounded, max_distance=float(bound),
              stack_entries=entries)
    assert (free[1] == 0).sum() >= 12 and (free[1] > 0).sum() >= 100
    assert (bounded[0] >= 0).sum() >= len(tri) // 4 and (bounded[0] < 0).sum() >= len(tri) // 8
    # per-query bounds, the invalid ones of tr_within.h among them
    radii = np.where(np.arange(len(tri)) % 2 == 0, np.float32(np.inf), bound).astype(np.float32)
    radii[1:40:4] = np.nan
    radii[3:40:4] = -1.0
    got = check(r, v, f, tri, device, f"{name}, per-query bounds", max_distance=radii, stack_entries=1)
    TN.check_no_result(got, np.isnan(radii) | (radii < 0), name)


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_kernel_matches_the_host_walk_on_the_gpu_builders_tree(device, cases):
    import tri_nearest_sim
    from sim import SimBVH
    v, f, tri, free, bound, bounded = cases["icosphere"]
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    for entries in (0, 1):
        for md, want in ((None, free), (float(bound), bounded)):
            walked = tri_nearest_sim.walk(B, tri, md, entries)
            TN.assert_same(native(r, tri, device, md, stack_entries=entries), walked, f"GPU tree, stack_entries {entries}, bound {md}")
            TN.assert_same(walked, want, "host walk on the GPU tree against the brute force")


# ---- 3 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_case():
    import tri_nearest_sim
    v, f, _ = NC.icosphere()
    tri = TC.hashed_triangles(4133, [-1.2] * 3, [1.2] * 3, TC.extent(v), seed=1)
    return v, f, tri, tri_nearest_sim.brute(v, f, tri)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, tail_case, n):
    v, f, tri, whole = tail_case
    r = make(v, f, device)
    got = check(r, v, f, tri[:n], device, f"{n} triangles", want=tuple(a[:n] for a in whole))
    assert got[0].shape == (n,) and got[1].shape == (n,) and got[2].shape == (n, 3) and got[3].shape == (n, 3)
    if n == 4133:
        assert (got[1] == 0).sum() > 100 and (got[1] > 0).sum() > 100


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_meshes_without_a_hierarchy(device):
    v, f = W.two_triangles()
    for nt in (2, 1, 0):
        vv, ff = v[:3 * nt], f[:nt]
        r = make(vv, ff, device)
        seen = set()
        for label, tri in TN.query_sets(v, f):
            tri = np.concatenate([tri, np.full((1, 3, 3), np.nan, np.float32)])
            for entries in (0, 1):
                got = check(r, vv, ff, tri, device, f"{nt} triangle(s), {label}", stack_entries=entries)
            seen |= set(np.unique(got[0]))
            TN.check_no_result(got, [-1] if nt else slice(None), f"{nt} triangle(s), {label}")
        assert seen == set(range(-1, nt))


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_hostile_triangles(device):
    v, f, _ = NC.icosphere()
    r = make(v, f, device)
    tri, valid, degenerate = TC.hostile_triangles(TC.hashed_triangles(704, v.min(0), v.max(0), TC.extent(v), seed=3))
    tri[128:192] = np.nan                                 # a whole wave of invalid queries ...
    tri[256:384, 2] = tri[256:384, 1]                     # ... a whole block of degenerate ones (a doubled vertex) ...
    tri[448:512] = tri[448:512, :1]                       # ... and a whole wave of points
    valid = np.isfinite(tri).all(axis=(1, 2))
    assert (~valid).sum() == 27 + 64
    for entries in (0, 1):
        got = check(r, v, f, tri, device, f"hostile triangles, stack_entries {entries}", stack_entries=entries)
    TN.check_no_result(got, ~valid, "invalid queries")
    assert (got[0][valid] >= 0).all() and not np.isnan(got[1]).any() and np.isfinite(got[2][valid]).all() and np.isfinite(got[3][valid]).all()
    assert np.isfinite(got[1][256:384]).all() and np.isfinite(got[1][448:512]).all()      # segments and points are answered
    assert got[1][32] == 0 and got[1][33] == 0 and got[1][34] > 1e38 and got[0][34] >= 0
    # +-FLT_MAX on the mesh's side
    bv, bf = tri[32:37].reshape(-1, 3), np.arange(15, dtype=np.int32).reshape(-1, 3)
    back = check(make(bv, bf, device), bv, bf, tri, device, "a mesh of huge triangles", stack_entries=1)
    assert not np.isnan(back[1]).any() and (back[1][32:37] == 0).all()


HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_hostile_meshes(device, name, seed):
    c = M.case(name, seed)
    fa, _ = M.active_faces(c.v, c.f)
    r = make(c.v, c.f, device)
    for tri in TC.hostile_mesh_triangles(c, fa):
        for entries in (0, 1, 3):
            got = check(r, c.v, c.f, tri, device, f"{c.name}, stack_entries {entries}", stack_entries=entries)
        found = got[0] >= 0
        assert np.array_equal(found, np.isfinite(tri).all(axis=(1, 2)) & (len(fa) > 0))      # (a query may have overflowed)
        assert not c.inactive[got[0][found]].any() and not np.isnan(got[1]).any()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_snapped_inputs_equal_the_exact_reference(device):
    """inputs on the grid k * 2^-10, |k| <= 2^11 (asserted by tris_cases.snapped): the GPU's distance is 0 exactly where a pair
    with area meets, within eps of the exact one elsewhere, and its winner an exact minimiser within eps"""
    import tri_nearest_sim
    for name, (v, f, tri, *_) in TN.exact_reference().items():
        got = check(make(v, f, device), v, f, tri, device, f"snapped {name}", want=tri_nearest_sim.brute(v, f, tri), stack_entries=2)
        TN.check_exact_winner(name, got, "GPU")


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs_gives_the_same_bits(device, cases):
    v, f, tri, free, bound, bounded = cases["soup"]
    r = make(v, f, device)
    for want in itertools.product((True, False), repeat=3):
        got = native(r, tri, device, float(bound), want=want)
        assert got[0] is not None and [x is not None for x in got[1:]] == list(want)
        TN.assert_same(got, bounded, f"optional outputs {want}")


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_python_methods_batch_shapes_and_input_types(device, cases):
    import tri_nearest_sim
    v, f, tri, free, bound, bounded = cases["icosphere"]
    r = make(v, f, device)
    tri = tri[128:]                                   # from the own faces displaced by 1/32 of the extent on
    free = tuple(a[128:] for a in free)
    out = r.triangles_nearest(T(tri[0], device))
    assert len(out) == 4 and out[0].shape == () and out[0].dtype == torch.int32 and out[1].shape == () and out[1].dtype == torch.float32
    assert out[2].shape == (3,) and out[3].shape == (3,) and out[2].dtype == out[3].dtype == torch.float32
    TN.assert_same(tuple(host(x).reshape((1,) + tuple(x.shape)) for x in out), tuple(a[:1] for a in free), "()")

    def flat(t, shape, max_distance=None):
        """the method on one batch -> flat numpy arrays (the batch shape is checked)"""
        a, d, cm, cq = r.triangles_nearest(t, max_distance)
        assert tuple(a.shape) == shape and tuple(d.shape) == shape and tuple(cm.shape) == shape + (3,) and tuple(cq.shape) == shape + (3,)
        return host(a).reshape(-1), host(d).reshape(-1), host(cm).reshape(-1, 3), host(cq).reshape(-1, 3)
    TN.assert_same(flat(T(tri[:35].reshape(5, 7, 3, 3), device), (5, 7)), tuple(a[:35] for a in free), "[5, 7, 3, 3]")
    wide = torch.zeros((60, 3, 8), dtype=torch.float32, device=device)
    wide[:, :, 2:5] = T(tri[:60], device)
    assert not wide[::2, :, 2:5].is_contiguous()
    TN.assert_same(flat(wide[::2, :, 2:5], (30,)), tuple(a[:60:2] for a in free), "non-contiguous slices")
    TN.assert_same(flat(T(tri[:50].astype(np.float64), device), (50,)), tuple(a[:50] for a in free), "float64 input")
    TN.assert_same(flat(tri[:50], (50,)), tuple(a[:50] for a in free), "numpy input")
    TN.assert_same(flat(T(tri[:0], device), (0,)), tuple(a[:0] for a in free), "no triangles")
    # max_distance: a number, a tensor per query (broadcast to the batch shape), a host array
    b = float(bound)
    want = tri_nearest_sim.brute(v, f, tri[:35], b)
    assert (want[0] >= 0).any() and (want[0] < 0).any()
    TN.assert_same(flat(T(tri[:35].reshape(5, 7, 3, 3), device), (5, 7), b), want, "a scalar bound")
    radii = np.where(np.arange(35) % 2 == 0, np.float32(np.inf), np.float32(b)).astype(np.float32)
    want = tri_nearest_sim.brute(v, f, tri[:35], radii)
    TN.assert_same(flat(T(tri[:35].reshape(5, 7, 3, 3), device), (5, 7), T(radii.reshape(5, 7), device)), want, "a bound per query")
    TN.assert_same(flat(T(tri[:35], device), (35,), radii), want, "a bound per query from the host")
    row = tri_nearest_sim.brute(v, f, tri[:35], np.tile(radii[:7], 5))
    TN.assert_same(flat(T(tri[:35].reshape(5, 7, 3, 3), device), (5, 7), T(radii[:7], device)), row, "a bound that broadcasts")
    # refusals: those of triangles_any, and a bound that does not broadcast
    calls = [lambda: r.triangles_nearest(torch.from_numpy(tri[:4])), lambda: r.triangles_nearest(T(tri[:4, :2], device)),
             lambda: r.triangles_nearest(T(tri[:4].reshape(4, 9), device)), lambda: r.triangles_nearest(T(tri[:4, :, :2], device)),
             lambda: r.triangles_nearest(T(tri[0, 0], device)), lambda: r.triangles_nearest(T(tri[:4], device), T(radii[:3], device))]
    if torch.cuda.device_count() > 1:                 # a tensor on another GPU raises
        other = torch.device("cuda", (torch.device(device).index or 0) ^ 1)
        calls += [lambda: r.triangles_nearest(T(tri[:4], other))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    # one launch per call
    before = len(CALLS)
    r.triangles_nearest(T(tri, device))
    r.triangles_nearest(T(tri, device), b)
    assert len(CALLS) == before + 2


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_mesh_distance(device):
    import tri_nearest_sim
    v, f, _ = NC.icosphere()
    r = make(v, f, device)
    ext = TC.extent(v)
    near = (v + np.float32([0.3, -0.1, 0.2]) * np.float32(ext / 4)).astype(np.float32)
    far = (v + np.float32([5.0, 0.0, 0.0]) * np.float32(ext)).astype(np.float32)
    # the other mesh with its faces in another order and a vertex nobody uses
    f2 = np.ascontiguousarray(f[::-1])

    def result(out):
        assert len(out) == 5 and all(x.device.type == "cuda" for x in out)
        assert out[0].dtype == torch.float32 and out[0].shape == () and out[1].shape == () and out[2].shape == ()
        assert out[3].dtype == out[4].dtype == torch.float32 and out[3].shape == (3,) and out[4].shape == (3,)
        return host(out[0]), int(out[1]), int(out[2]), host(out[3]), host(out[4])

    def nothing(got):
        return np.isposinf(got[0]) and got[1] == -1 and got[2] == -1 and np.isnan(got[3]).all() and np.isnan(got[4]).all()
    for name, vv in (("displaced", near), ("far away", far)):
        vv = np.concatenate([vv, np.float32([[9, 9, 9]])])
        rows = tri_nearest_sim.brute(v, f, vv[f2])
        want = TN.reduce_rows(rows)
        if name == "displaced":       # they collide: 0, with the lexicographically first pair that meets
            import tris_sim
            met = tris_sim.brute(v, f, vv[f2])
            first = int(np.flatnonzero(met.count)[0])
            assert want[0] == 0 and want[1] == first and want[2] == met.faces[met.offsets[first]]
        else:
            assert 4 * ext <= want[0] < 5 * ext
        for chunk in (1 << 20, 7):
            before = len(CALLS)
            got = result(r.mesh_distance(T(vv, device), T(f2, device), chunk=chunk))
            TN.assert_same_pair(got, want, f"{name}, chunk {chunk}")
            # one launch per chunk, every one after the first with the best distance so far as its bound
            bounds = CALLS[before:]
            assert len(bounds) == -(-len(f2) // chunk) and bounds[0] is None
            assert all(isinstance(b, float) and b >= want[0] for b in bounds[1:]) and (len(bounds) == 1 or bounds[-1] == want[0])
            assert all(a >= b for a, b in zip(bounds[1:], bounds[2:]))
        TN.assert_same_pair(result(r.mesh_distance(vv, f2.astype(np.int64))), want, f"{name}, numpy input")
        if name == "far away":
            # a bound: at the answer it is kept (its d2 is within the square of its own rounded distance or the row below shows
            # the float64 rule), below it nothing is
            for md in (float(want[0]) * 2, float(np.nextafter(want[0], np.float32(0)))):
                bounded = TN.reduce_rows(tri_nearest_sim.brute(v, f, vv[f2], md), 7)
                for chunk in (1 << 20, 7):
                    TN.assert_same_pair(result(r.mesh_distance(T(vv, device), T(f2, device), md, chunk=chunk)), bounded, f"bound {md}, chunk {chunk}")
            assert nothing(bounded) and nothing(result(r.mesh_distance(T(vv, device), T(f2, device), float("nan"))))
            assert nothing(result(r.mesh_distance(T(vv, device), T(f2, device), -1.0)))
    assert nothing(result(r.mesh_distance(T(near, device), T(f[:0], device))))
    for bad in (lambda: r.mesh_distance(T(near, device), T(f, device), chunk=0), lambda: r.mesh_distance(T(near[:5], device), T(f, device)),
                lambda: r.mesh_distance(T(near[:, :2], device), T(f, device)), lambda: r.mesh_distance(T(near, device), T(f[:, :2], device))):
        with pytest.raises(ValueError):
            bad()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_lifecycle_refit_update_and_load(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    tri = TC.hashed_triangles(600, [-1.8] * 3, [2.0] * 3, 2.0, seed=2)
    r = make(v, f, device)
    check(r, v, f, tri, device, "built")
    r.refit(T(v2, device))
    check(r, v2, f, tri, device, "after a refit with moved vertices")
    check(r, v2, f, tri, device, "after a refit, one stack entry", stack_entries=1)
    path = str(tmp_path / "mesh.npz")
    r.save(path)
    check(RayMeshIntersector.load(path, device=device), v2, f, tri, device, "loaded")
    v3, f3, _ = NC.soup_with_degenerates()
    r.update_raw(T(v3, device), T(f3, device))
    check(r, v3, f3, tri, device, "update_raw to another mesh")


# ---- 11 -----------------------------------------------------------------------------------------------------------------
def test_the_first_call_of_a_fresh_intersector_can_be_captured(device):
    import tri_nearest_sim
    import triro.backend.ops as hops
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=5, amplitude=0.05)
    v2 = (v * np.float32(1.6) + np.float32([0.3, 0.0, -0.2])).astype(np.float32)
    n = 600
    t1 = TC.hashed_triangles(n, [-1.4] * 3, [1.4] * 3, 1.6, seed=4)
    t2 = TC.hashed_triangles(n, [-2.5] * 3, [2.5] * 3, 1.6, seed=5)
    r = make(v, f, device)
    tt = T(t1, device)
    radii = torch.full((n,), float("inf"), dtype=torch.float32, device=device)
    steps = ((v, t1, np.inf), (v, t2, np.inf), (v2, t2, 0.5), (v2, t1, 0.25))
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the call neither allocates nor synchronises
        outs = hops.triangles_nearest_native(r.as_wrapper, tt, radii)
    for step, (vv, q, md) in enumerate(steps):
        if step == 2:
            r.refit(T(vv, device))                      # moves the bounds
        tt.copy_(T(q, device))
        radii.fill_(md)
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(*outs, what=f"graph replay {step}")
        want = tri_nearest_sim.brute(vv, f, q, md)
        assert (want[0] >= 0).any() and (step < 2 or (want[0] < 0).any())
        TN.assert_same(tuple(host(x) for x in outs), want, f"graph replay {step}")
