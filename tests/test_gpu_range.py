"""Range queries (libtriro_range.so, k_range_query<any | closest>) against the host brute force.

The oracle of every comparison is tests/host_sim/range_sim.brute: the per-triangle predicate of csrc/tr_range.h over every
triangle, any and the lexicographic closest (t, face index), on the same float32 inputs -- itself pinned to the oracle's
filtered multi-hit list, to the old contract at default bounds and to a scene with exact distances by
tests/test_range_cpu.py.  Comparisons are bit for bit, +Inf included.  Every native call of this module comes back through
a wrapper that runs poison.assert_written on everything it returns (the autouse fixture `checked_native`); the captured
calls are checked after each replay."""
import ctypes as C

import numpy as np
import pytest
import torch

import hostile_meshes as M
import poison
import range_cases as RC
import workloads as W
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
    originals = {name: getattr(hops, name) for name in ("range_any_native", "range_closest_native")}

    def wrap(name):
        def call(*args, **kwargs):
            res = originals[name](*args, **kwargs)
            CALLS["native"] += 1
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
                poison.assert_written(*(res if isinstance(res, tuple) else (res,)), what=name)
            return res
        return call
    for name in originals:
        setattr(hops, name, wrap(name))
    try:
        yield
    finally:
        for name, fn in originals.items():
            setattr(hops, name, fn)


def bound(x, n, device):
    return None if x is None else T(np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (n,))), device)


def as_dict(any_, closest):
    out = {}
    if any_ is not None:
        out["any"] = any_.cpu().numpy().reshape(-1)
    if closest is not None:
        for k, x in zip(("hit", "front", "tri", "loc", "uv", "t"), closest):
            out[k] = None if x is None else x.cpu().numpy()
    return out


def native(r, o, d, lo, hi, device, **kw):
    """both queries on dense rays: the dict of range_sim"""
    import triro.backend.ops as hops
    n = len(o)
    ot, dt, lt, ht = T(o, device), T(d, device), bound(lo, n, device), bound(hi, n, device)
    return as_dict(hops.range_any_native(r.as_wrapper, ot, dt, lt, ht, **kw), hops.range_closest_native(r.as_wrapper, ot, dt, lt, ht, **kw))


def check(r, v, f, o, d, lo, hi, device, what, want=None, **kw):
    import range_sim
    want = range_sim.brute(v, f, o, d, lo, hi) if want is None else want
    got = native(r, o, d, lo, hi, device, **kw)
    RC.assert_same_bits(got, want, what)
    return got


@pytest.fixture(scope="module")
def cases():
    """(vertices, faces, origins, directions, tmin, tmax, brute force) of every mesh, computed once"""
    import range_sim
    out = {}
    for name, mk in RC.MESHES.items():
        v, f, o, d, lo, hi = mk()
        out[name] = (v, f, o, d, lo, hi, range_sim.brute(v, f, o, d, lo, hi))
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.MESHES))
def test_meshes_at_every_stack_limit(device, cases, name):
    v, f, o, d, lo, hi, want = cases[name]
    r = make(v, f, device)
    if name == "deep":
        assert r.bvh_info()["depth"] > 32
    for entries in (0, 1, 2, 3):
        check(r, v, f, o, d, lo, hi, device, f"{name}, stack_entries {entries}", want=want, stack_entries=entries)


def test_kernel_matches_the_host_walk_on_the_gpu_builders_tree(device, cases):
    import range_sim
    from sim import SimBVH
    v, f, o, d, lo, hi, want = cases["icosphere"]
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    for entries in (0, 1):
        host = range_sim.walk(B, o, d, lo, hi, entries)
        RC.assert_same_bits(native(r, o, d, lo, hi, device, stack_entries=entries), host, f"GPU tree, stack_entries {entries}")
        RC.assert_same_bits(host, want, "host walk on the GPU tree against the brute force")
        assert host["lost"].any() == (entries == 1)


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def raw_closest(r, o, d, lo, hi, device, leave_out=()):
    """tr_range_closest itself, with the optional outputs named in leave_out passed as NULL"""
    import triro.backend.ops as hops
    n = len(o)
    ot, dt, lt, ht = T(o, device), T(d, device), bound(lo, n, device), bound(hi, n, device)
    spec = dict(tri=((n,), torch.int32), t=((n,), torch.float32), hit=((n,), torch.bool), front=((n,), torch.bool),
                loc=((n, 3), torch.float32), uv=((n, 2), torch.float32))
    outs = {k: None if k in leave_out else hops._new_output(sh, dt_, ot.device) for k, (sh, dt_) in spec.items()}
    ptr = lambda x: None if x is None else x.data_ptr()      # noqa: E731
    with torch.cuda.device(ot.device):
        hops._check(hops.get_range_module().tr_range_closest(
            r.as_wrapper._inner, C.byref(hops.make_rays(ot, dt)), ptr(lt), ptr(ht), *(ptr(outs[k]) for k in ("tri", "t", "hit", "front", "loc", "uv")),
            0, torch.cuda.current_stream(ot.device).cuda_stream))
    torch.cuda.synchronize()
    poison.assert_written(*outs.values(), what=f"tr_range_closest without {leave_out}")
    return {k: None if x is None else x.cpu().numpy() for k, x in outs.items()}


@pytest.fixture(scope="module")
def tail_case(cases):
    v, f, o, d, lo, hi, want = cases["icosphere"]
    return v, f, o[:4133], d[:4133], lo[:4133], hi[:4133], {k: x[:4133] for k, x in want.items()}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, tail_case, n):
    import triro.backend.ops as hops
    v, f, o, d, lo, hi, want = tail_case
    r = make(v, f, device)
    want = {k: x[:n] for k, x in want.items()}
    o, d, lo, hi = o[:n], d[:n], lo[:n], hi[:n]
    got = check(r, v, f, o, d, lo, hi, device, f"{n} rays", want=want)
    assert got["any"].shape == (n,) and got["loc"].shape == (n, 3) and got["uv"].shape == (n, 2) and got["t"].shape == (n,)
    for leave_out in ("t", "hit", "front", "loc", "uv"):
        got = raw_closest(r, o, d, lo, hi, device, (leave_out,))
        assert got[leave_out] is None
        RC.assert_same_bits(got, want, f"{n} rays, no {leave_out}", keys=RC.KEYS_CLOSEST)
    got = raw_closest(r, o, d, lo, hi, device, ("t", "hit", "front", "loc", "uv"))
    RC.assert_same_bits(got, want, f"{n} rays, tri only", keys=("tri",))
    # the switches of the binding
    ot, dt, lt, ht = T(o, device), T(d, device), bound(lo, n, device), bound(hi, n, device)
    hit, front, tri, loc, uv, t = hops.range_closest_native(r.as_wrapper, ot, dt, lt, ht, want_t=False, want_dense=False)
    assert hit is None and front is None and loc is None and uv is None and t is None and np.array_equal(tri.cpu().numpy(), want["tri"])
    # one bound alone
    check(r, v, f, o, d, None, hi, device, f"{n} rays, tmax alone", want=None if n else want)
    check(r, v, f, o, d, lo, None, device, f"{n} rays, tmin alone", want=None if n else want)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_strided_rays_with_a_broadcast_origin(device, cases):
    import range_sim
    import triro.backend.ops as hops
    v, f = cases["icosphere"][:2]
    H, Wd = 37, 53
    n = H * Wd
    d = cases["icosphere"][3][:n]
    lo, hi = RC.hash_bounds(n, 91, 2.5)
    origin = np.array([0.2, -0.1, 0.3], np.float32)
    wide = torch.zeros((H, Wd, 5), dtype=torch.float32, device=device)
    wide[..., 1:4] = T(d.reshape(H, Wd, 3), device)
    dirs = wide[..., 1:4]
    origins = T(origin, device).expand(H, Wd, 3)
    assert not dirs.is_contiguous() and origins.stride() == (0, 0, 1)
    r = make(v, f, device)
    want = range_sim.brute(v, f, np.tile(origin, (n, 1)), d, lo, hi)
    assert want["hit"].sum() > 100
    lt, ht = T(lo, device), T(hi, device)
    a = hops.range_any_native(r.as_wrapper, origins, dirs, lt, ht)
    c = hops.range_closest_native(r.as_wrapper, origins, dirs, lt, ht)
    assert a.shape == (H, Wd) and c[3].shape == (H, Wd, 3) and c[4].shape == (H, Wd, 2) and c[5].shape == (H, Wd)
    RC.assert_same_bits(as_dict(a, c), want, "[H, W, 3] view, broadcast origin")
    # rows of a transposed tensor: the general stride path for both
    ot = T(np.tile(origin, (n, 1)).reshape(H, Wd, 3), device).transpose(0, 1)
    dtr = T(d.reshape(H, Wd, 3), device).transpose(0, 1)
    want_t = {k: np.ascontiguousarray(x.reshape(H, Wd, *x.shape[1:]).swapaxes(0, 1)).reshape(n, *x.shape[1:]) for k, x in want.items() if k in RC.KEYS_ANY + RC.KEYS_CLOSEST}
    lt2 = T(np.ascontiguousarray(lo.reshape(H, Wd).T).reshape(-1), device)
    ht2 = T(np.ascontiguousarray(hi.reshape(H, Wd).T).reshape(-1), device)
    RC.assert_same_bits(as_dict(hops.range_any_native(r.as_wrapper, ot, dtr, lt2, ht2), hops.range_closest_native(r.as_wrapper, ot, dtr, lt2, ht2)),
                        want_t, "transposed rays")


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["interior", "diagonal", "vertex"])
def test_exact_bounds_on_the_sheet_scene(device, kind):
    import range_sim
    v, f = RC.sheets()
    o, d, lo, hi, first, count = RC.sheet_cases(kind)
    want = range_sim.brute(v, f, o, d, lo, hi)
    RC.check_sheet_results(want, first, count, kind)
    r = make(v, f, device)
    for entries in (0, 1):
        check(r, v, f, o, d, lo, hi, device, f"sheets, {kind}, stack_entries {entries}", want=want, stack_entries=entries)


def test_meshes_without_a_hierarchy(device):
    v, f = W.two_triangles()
    o, d = W.hash_rays(500, 5, [-0.6, -0.6, -1.5], [0.6, 0.6, 0.5])
    d[:, 2] = np.abs(d[:, 2]) * np.sign(-0.5 - o[:, 2])
    lo, hi = RC.hash_bounds(500, 6, 3.0)
    for nt in (2, 1, 0):
        vv, ff = v[:3 * nt], f[:nt]
        r = make(vv, ff, device)
        for entries in (0, 1):
            got = check(r, vv, ff, o, d, lo, hi, device, f"{nt} triangle(s)", stack_entries=entries)
        if nt == 0:
            assert not got["any"].any() and (got["tri"] == -1).all() and np.isposinf(got["t"]).all()
        else:
            assert got["hit"].any() and not got["hit"].all() and got["tri"].max() == nt - 1


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "shells5"])
def test_default_bounds_are_the_direct_launches_of_the_same_handle(device, cases, name):
    v, f, o, d = cases[name][:4]
    r = make(v, f, device)
    ot, dt = T(o, device), T(d, device)
    hit, front, tri, loc, uv = r.intersects_closest(ot, dt)
    got = r.intersects_closest_range(ot, dt)
    assert hit.sum() > 1000
    for a, b, what in zip(got[:5], (hit, front, tri, loc, uv), ("hit", "front", "tri", "loc", "uv")):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what
    assert torch.equal(torch.isposinf(got[5]), ~hit)
    assert torch.equal(r.intersects_any_range(ot, dt), r.intersects_any(ot, dt))
    assert torch.equal(r.intersects_any_range(ot, dt, -3.0, float("inf")), r.intersects_any(ot, dt))


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_hostile_rays_and_bounds(device, cases):
    v, f = cases["icosphere"][:2]
    o, d, lo, hi, bad = RC.hostile_rays(*cases["icosphere"][2:6])
    r = make(v, f, device)
    for entries in (0, 1):
        got = check(r, v, f, o, d, lo, hi, device, f"hostile rays, stack_entries {entries}", stack_entries=entries)
    RC.check_miss_rule(got, bad, "hostile rays")
    assert got["hit"][~bad].sum() > 50


def test_a_mesh_with_non_finite_vertices(device):
    import range_sim
    c = M.case("faraway_nonfinite", 0)
    lo, hi = RC.hash_bounds(len(c.o), 97, 3.0)
    r = make(c.v, c.f, device)
    want = range_sim.brute(c.v, c.f, c.o, c.d, lo, hi)
    assert want["hit"].sum() > 100 and not np.isfinite(c.v).all()
    for entries in (0, 1):
        got = check(r, c.v, c.f, c.o, c.d, lo, hi, device, f"{c.name}, stack_entries {entries}", want=want, stack_entries=entries)
    assert c.inactive.any() and not c.inactive[got["tri"][got["hit"]]].any()          # no hit names a face with a non-finite coordinate
    check(r, c.v, c.f, c.o, c.d, None, None, device, f"{c.name}, default bounds")


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_the_first_call_of_a_fresh_intersector_can_be_captured(device):
    import range_sim
    import triro.backend.ops as hops
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=5, amplitude=0.05)
    n = 1000
    o1, d1 = W.hash_rays(n, 29, v.min(0), v.max(0))
    o2, d2 = W.hash_rays(n, 31, v.min(0), v.max(0))
    b1, b2 = RC.hash_bounds(n, 33, 3.0), RC.hash_bounds(n, 35, 3.0)
    r = make(v, f, device)
    ot, dt, lt, ht = T(o1, device), T(d1, device), T(b1[0], device), T(b1[1], device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the calls neither allocate nor synchronise
        out_any = hops.range_any_native(r.as_wrapper, ot, dt, lt, ht)
        out_closest = hops.range_closest_native(r.as_wrapper, ot, dt, lt, ht)
    for step, (o, d, (lo, hi)) in enumerate(((o1, d1, b1), (o2, d2, b2))):
        for src, dst in ((o, ot), (d, dt), (lo, lt), (hi, ht)):
            dst.copy_(T(src, device))
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(out_any, *out_closest, what=f"graph replay {step}")
        RC.assert_same_bits(as_dict(out_any, out_closest), range_sim.brute(v, f, o, d, lo, hi), f"graph replay {step}")


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_update_raw_and_refit(device, cases):
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    n = 3000
    o, d = W.hash_rays(n, 23, [-1.4] * 3, [1.6] * 3)
    lo, hi = RC.hash_bounds(n, 25, 3.0)
    r = make(v, f, device)
    check(r, v, f, o, d, lo, hi, device, "built")
    r.refit(T(v2, device))
    check(r, v2, f, o, d, lo, hi, device, "after a refit with moved vertices")
    check(r, v2, f, o, d, lo, hi, device, "after a refit, one stack entry", stack_entries=1)
    v3, f3 = RC.sheets()
    r.update_raw(T(v3, device), T(f3, device))
    so, sd, slo, shi, _, _ = RC.sheet_cases("interior")
    check(r, v3, f3, so, sd, slo, shi, device, "update_raw to another mesh")


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_python_api_shapes_bounds_segments_and_errors(device, cases):
    import range_sim
    v, f, o, d, lo, hi, want = cases["shells5"]
    r = make(v, f, device)
    n = 35
    # [3]: a single ray, scalar bounds
    w1 = range_sim.brute(v, f, o[:1], d[:1], 0.25, 1.5)
    a = r.intersects_any_range(T(o[0], device), T(d[0], device), 0.25, 1.5)
    c = r.intersects_closest_range(T(o[0], device), T(d[0], device), 0.25, 1.5)
    assert a.shape == () and a.dtype == torch.bool and c[3].shape == (3,) and c[4].shape == (2,) and c[5].shape == ()
    assert [x.dtype for x in c] == [torch.bool, torch.bool, torch.int32, torch.float32, torch.float32, torch.float32]
    RC.assert_same_bits(as_dict(a, c), w1, "[3] with scalar bounds")
    # [5, 7, 3] with tensor bounds of the batch shape
    ot, dt = T(o[:n].reshape(5, 7, 3), device), T(d[:n].reshape(5, 7, 3), device)
    a = r.intersects_any_range(ot, dt, T(lo[:n].reshape(5, 7), device), T(hi[:n].reshape(5, 7), device))
    c = r.intersects_closest_range(ot, dt, T(lo[:n].reshape(5, 7), device), T(hi[:n].reshape(5, 7), device))
    assert a.shape == (5, 7) and c[0].shape == (5, 7) and c[3].shape == (5, 7, 3) and c[4].shape == (5, 7, 2) and c[5].shape == (5, 7)
    RC.assert_same_bits(as_dict(a, c), {k: x[:n] for k, x in want.items()}, "[5, 7, 3]")
    # bounds that broadcast: a row [7], a numpy array, a python float, a float64 tensor; one bound alone
    row = hi[:7]
    wb = range_sim.brute(v, f, o[:n], d[:n], 0.1, np.tile(row, 5))
    RC.assert_same_bits(as_dict(r.intersects_any_range(ot, dt, 0.1, row), r.intersects_closest_range(ot, dt, np.float64(0.1), T(row.astype(np.float64), device))),
                        wb, "broadcast bounds")
    wb = range_sim.brute(v, f, o[:n], d[:n], None, 0.75)
    RC.assert_same_bits(as_dict(r.intersects_any_range(ot, dt, tmax=0.75), r.intersects_closest_range(ot, dt, None, torch.tensor(0.75))), wb, "tmax alone")
    # segments: the float32 difference and the range [0, 1]
    p0, p1 = o[:2000], (o[:2000] + d[:2000] * hi[:2000, None]).astype(np.float32)
    so, sd, slo, shi = RC.segment_rays(p0, p1)
    ws = range_sim.brute(v, f, so, sd, slo, shi)
    assert ws["hit"].sum() > 200 and (~ws["hit"]).sum() > 200
    a, c = r.segments_any(T(p0, device), T(p1, device)), r.segments_closest(T(p0, device), T(p1, device))
    RC.assert_same_bits(as_dict(a, c), ws, "segments")
    assert ((c[5][c[0]] >= 0) & (c[5][c[0]] <= 1)).all()
    a = r.segments_any(T(p0[:24].reshape(2, 3, 4, 3), device), T(p1[:24].reshape(2, 3, 4, 3), device))
    assert a.shape == (2, 3, 4) and np.array_equal(a.cpu().numpy().reshape(-1), ws["any"][:24])
    # the sheet scene: p1 exactly on a sheet blocks, one ulp short of it does not
    sv, sf = RC.sheets()
    s = make(sv, sf, device)
    q0 = RC.sheet_origins("interior")
    q0[:, 2] = 0.25
    on, short = q0.copy(), q0.copy()
    on[:, 2], short[:, 2] = 1.0, np.nextafter(np.float32(1), np.float32(0))
    assert s.segments_any(T(q0, device), T(on, device)).all() and not s.segments_any(T(q0, device), T(short, device)).any()
    assert (s.segments_closest(T(q0, device), T(on, device))[5] == 1.0).all()
    # errors: CPU tensors, shapes, bounds that do not broadcast
    with pytest.raises(ValueError):
        r.intersects_any_range(torch.from_numpy(o[:4]), torch.from_numpy(d[:4]))
    with pytest.raises(ValueError):
        r.segments_any(torch.from_numpy(o[:4]), T(d[:4], device))
    with pytest.raises(ValueError):
        r.intersects_closest_range(T(o[:4, :2], device), T(d[:4, :2], device))
    with pytest.raises(ValueError):
        r.intersects_any_range(T(o[:4], device), T(d[:5], device))
    with pytest.raises(ValueError):
        r.intersects_any_range(ot, dt, tmin=T(lo[:6], device))
    with pytest.raises(ValueError):
        r.segments_closest(T(o[:4], device), T(o[:5], device))
