"""intersects_count_range / intersects_all_range / segments_count / segments_all (libtriro_cross.so: k_cross<>, k_cross_rows)
against the host brute force.

The oracle of every comparison is tests/host_sim/cross_sim.brute: the per-triangle predicate of csrc/tr_range.h over every
triangle, the rows ordered by numpy.lexsort, on the same float32 inputs -- itself pinned to range_sim's brute force, to scenes
with known lists and to integer arithmetic by tests/test_cross_cpu.py.  Comparisons are bit for bit (count, offsets, face, t,
front, loc, uv, ray).  Every native call of the bindings comes back through a wrapper that runs poison.assert_written on its
outputs (the autouse fixture `checked_native`); the row arrays of the direct calls (fill) carry poisoned guard rows on both
sides of the `total` rows, checked after every call; captured calls are checked after each replay."""
import ctypes as C

import numpy as np
import pytest
import torch

import cross_cases as CC
import hostile_meshes as M
import poison
import range_cases as RC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("cross_count_native", "cross_fill_native")
CALLS = {name: 0 for name in NATIVES}
GUARD = 1024
ROWS = dict(faces=((), torch.int32), t=((), torch.float32), front=((), torch.bool), loc=((3,), torch.float32), uv=((2,), torch.float32),
            ray=((), torch.int64), slot=((), torch.int32))
OPTIONAL = ("front", "loc", "uv", "ray")


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


def bound(x, n, device):
    return None if x is None else T(np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (n,))), device)


def guarded_fill(r, ot, dt, lt, ht, count, offsets, total, stack_entries=0, leave_out=(), ray_base=0, expect_full=True):
    """tr_cross_fill itself into row arrays with GUARD poisoned rows on either side of the `total` rows; the optional outputs
    named in leave_out are passed as NULL (and d_slot with them when no row is to be evaluated).  After the call every guard
    row still holds its poison and (expect_full) every row inside was written.  -> {name: tensor of the total rows}"""
    import triro.backend.ops as hops
    dev = ot.device
    need_slot = any(k not in leave_out for k in ("front", "loc", "uv"))
    bufs = {}
    for k, (tail, ty) in ROWS.items():
        if k in leave_out or (k == "slot" and not need_slot):
            bufs[k] = None
        else:
            bufs[k] = poison.poisoned((GUARD + total + GUARD,) + tail, ty, dev)
    ptr = lambda k: None if bufs[k] is None else bufs[k][GUARD:].data_ptr()      # noqa: E731
    with torch.cuda.device(dev):
        hops._check(hops.get_cross_module().tr_cross_fill(
            r.as_wrapper._inner, C.byref(hops.make_rays(ot, dt)), None if lt is None else lt.data_ptr(), None if ht is None else ht.data_ptr(),
            count.data_ptr(), offsets.data_ptr(), total, ptr("faces"), ptr("t"), ptr("front"), ptr("loc"), ptr("uv"), ptr("ray"), ray_base,
            ptr("slot"), int(stack_entries), hops._stream_ptr(dev)))
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        if b is None:
            out[k] = None
            continue
        stale = poison.stale_mask(b).reshape(len(b), -1).all(1)
        assert stale[:GUARD].all() and stale[GUARD + total:].all(), f"{k}: a guard row was written (total {total}, stack_entries {stack_entries})"
        if expect_full:
            assert not stale[GUARD:GUARD + total].any(), f"{k}: a row inside was not written"
        out[k] = b[GUARD:GUARD + total]
    return out


def native(r, o, d, lo, hi, device, stack_entries=0, leave_out=(), ray_base=0):
    """the count entry through its binding, then the fill into guarded rows -> a cross_sim.Result of numpy arrays"""
    import cross_sim
    import triro.backend.ops as hops
    n = len(o)
    ot, dt = T(np.ascontiguousarray(o, np.float32).reshape(-1, 3), device), T(np.ascontiguousarray(d, np.float32).reshape(-1, 3), device)
    lt, ht = bound(lo, n, device), bound(hi, n, device)
    count = hops.cross_count_native(r.as_wrapper, ot, dt, lt, ht, stack_entries)
    assert count.dtype == torch.int32 and count.shape == (n,)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    offsets[1:] = torch.cumsum(count, 0)
    total = int(offsets[-1])
    rows = guarded_fill(r, ot, dt, lt, ht, count, offsets[:n].contiguous(), total, stack_entries, leave_out, ray_base)
    front = rows["front"]
    return cross_sim.Result(host(count), host(offsets), host(rows["faces"]), host(rows["t"]), None if front is None else host(front),
                            host(rows["loc"]), host(rows["uv"]), host(rows["ray"]))


def check(r, v, f, o, d, lo, hi, device, what, want=None, **kw):
    import cross_sim
    want = cross_sim.brute(v, f, o, d, lo, hi, ray_base=kw.get("ray_base", 0)) if want is None else want
    got = native(r, o, d, lo, hi, device, **kw)
    CC.assert_same(got, want, what)
    return got


@pytest.fixture(scope="module")
def cases():
    """(vertices, faces, origins, directions, tmin, tmax, brute force) of every mesh, computed once"""
    import cross_sim
    out = {}
    for name, mk in RC.MESHES.items():
        v, f, o, d, lo, hi = mk()
        out[name] = (v, f, o, d, lo, hi, cross_sim.brute(v, f, o, d, lo, hi))
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.MESHES))
def test_kernels_match_the_brute_force_at_every_stack_limit(device, cases, name):
    v, f, o, d, lo, hi, want = cases[name]
    r = make(v, f, device)
    if name == "deep":
        assert r.bvh_info()["depth"] > 32 and want.count.max() >= 3000
    for entries in (0, 1, 2, 3):
        check(r, v, f, o, d, lo, hi, device, f"{name}, stack_entries {entries}", want=want, stack_entries=entries)


def test_kernels_match_the_host_walk_on_the_gpu_builders_tree(device, cases):
    import cross_sim
    from sim import SimBVH
    v, f, o, d, lo, hi, want = cases["icosphere"]
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    for entries in (0, 1):
        walked, lost = cross_sim.walk(B, o, d, lo, hi, entries, want_lost=True)
        CC.assert_same(native(r, o, d, lo, hi, device, stack_entries=entries), walked, f"GPU tree, stack_entries {entries}")
        CC.assert_same(walked, want, "host walk on the GPU tree against the brute force")
        assert lost.any() == (entries == 1)


def test_the_binding_of_the_whole_query_is_the_count_the_scan_and_the_fill(device, cases):
    import cross_sim
    import triro.backend.ops as hops
    v, f, o, d, lo, hi, _ = cases["shells5"]
    r = make(v, f, device)
    n = 5000
    want = cross_sim.brute(v, f, o[:n], d[:n], lo[:n], hi[:n], ray_base=11)
    before = dict(CALLS)
    res = hops.cross_all_native(r.as_wrapper, T(o[:n], device), T(d[:n], device), T(lo[:n], device), T(hi[:n], device), True, True, True, True, 11)
    assert CALLS["cross_count_native"] == before["cross_count_native"] + 1 and CALLS["cross_fill_native"] == before["cross_fill_native"] + 1
    torch.cuda.synchronize()
    poison.assert_written(res[0], what="cross_all_native offsets")
    assert res[0].dtype == torch.int64 and res[1].dtype == torch.int32 and res[3].dtype == torch.bool and res[6].dtype == torch.int64
    got = cross_sim.Result(want.count, *(host(x) for x in res))
    CC.assert_same(got, want, "cross_all_native")


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, cases, n):
    import cross_sim
    v, f, o, d, lo, hi, _ = cases["icosphere"]
    o, d, lo, hi = o[:n], d[:n], lo[:n], hi[:n]
    r = make(v, f, device)
    want = cross_sim.brute(v, f, o, d, lo, hi)
    got = check(r, v, f, o, d, lo, hi, device, f"{n} rays", want=want)
    total = int(want.offsets[-1])
    assert got.count.shape == (n,) and got.offsets.shape == (n + 1,) and got.faces.shape == (total,) and got.t.shape == (total,)
    assert got.front.shape == (total,) and got.loc.shape == (total, 3) and got.uv.shape == (total, 2) and got.ray.shape == (total,)
    # each optional output left out in turn, then all of them (no slot scratch either)
    for leave_out in [(k,) for k in OPTIONAL] + [OPTIONAL, ("front", "loc", "uv")]:
        g = check(r, v, f, o, d, lo, hi, device, f"{n} rays, without {leave_out}", want=want, leave_out=leave_out)
        assert all(getattr(g, k) is None for k in leave_out) and all(getattr(g, k) is not None for k in OPTIONAL if k not in leave_out)
    # one bound alone, and none
    check(r, v, f, o, d, None, hi, device, f"{n} rays, tmax alone")
    check(r, v, f, o, d, lo, None, device, f"{n} rays, tmin alone")
    check(r, v, f, o, d, None, None, device, f"{n} rays, default bounds", ray_base=1 << 40)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_strided_rays_with_a_broadcast_origin(device, cases):
    import cross_sim
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
    want = cross_sim.brute(v, f, np.tile(origin, (n, 1)), d, lo, hi)
    assert (want.count > 0).sum() > 100
    lt, ht = T(lo, device), T(hi, device)

    def run(ot, dt, lt, ht, want, what):
        count = hops.cross_count_native(r.as_wrapper, ot, dt, lt, ht)
        assert count.shape == ot.shape[:-1]
        offsets = T(want.offsets, device)
        rows = guarded_fill(r, ot, dt, lt, ht, count.reshape(-1), offsets[:n].contiguous(), int(want.offsets[-1]))
        got = cross_sim.Result(host(count).reshape(-1), want.offsets, host(rows["faces"]), host(rows["t"]), host(rows["front"]), host(rows["loc"]),
                               host(rows["uv"]), host(rows["ray"]))
        CC.assert_same(got, want, what)
    run(origins, dirs, lt, ht, want, "[H, W, 3] view, broadcast origin")
    # rows of a transposed tensor: the general stride path for both
    ot = T(np.tile(origin, (n, 1)).reshape(H, Wd, 3), device).transpose(0, 1)
    dtr = T(d.reshape(H, Wd, 3), device).transpose(0, 1)
    tr = lambda x: np.ascontiguousarray(x.reshape(H, Wd, *x.shape[1:]).swapaxes(0, 1)).reshape(n, *x.shape[1:])      # noqa: E731
    want_t = cross_sim.brute(v, f, np.tile(origin, (n, 1)), tr(d), tr(lo), tr(hi))
    run(ot, dtr, T(tr(lo), device), T(tr(hi), device), want_t, "transposed rays")


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["interior", "diagonal", "vertex"])
def test_exact_lists_on_the_sheet_scene(device, kind):
    v, f = RC.sheets()
    o, d, lo, hi, first, count = RC.sheet_cases(kind)
    r = make(v, f, device)
    for entries in (0, 1):
        got = check(r, v, f, o, d, lo, hi, device, f"sheets, {kind}, stack_entries {entries}", stack_entries=entries)
        CC.check_sheets(got, lo, hi, count, f"sheets, {kind}, stack_entries {entries}")


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_long_and_uneven_rows_in_one_wave(device, cases):
    import cross_sim
    # deep: aimed rays with 3 000 ties each (default bounds: every one of them counts) between hash rays that cross nothing
    v, f, o, d = cases["deep"][:4]
    aimed = np.flatnonzero(cases["deep"][6].count >= 3000)          # (not every aimed float32 direction meets triangles of 1e-9)
    assert len(aimed) >= 64
    pick = np.empty(192, np.int64)
    pick[0::3], pick[1::3], pick[2::3] = np.arange(64), aimed[:64], 100 + np.arange(64)
    o, d = o[pick], d[pick]
    want = cross_sim.brute(v, f, o, d)
    assert (want.count[1::3] >= 3000).all() and (want.count[0::3] == 0).sum() > 32
    r = make(v, f, device)
    for entries in (0, 1):
        got = check(r, v, f, o, d, None, None, device, f"deep, aimed rays between misses, stack_entries {entries}", want=want, stack_entries=entries)
    rows = CC.rows_of(got, 1)
    values, times = np.unique(got.t[rows], return_counts=True)
    ties = got.faces[rows][got.t[rows] == values[times.argmax()]]
    assert len(ties) >= 3000 and (np.diff(ties) > 0).all()          # equal distances: ascending faces
    # a stack of 40 quads: rays that cross 0, 1, 2, 3, 33 and 40 of them side by side in every block
    v, f, o, d, expected = CC.quad_stack()
    r = make(v, f, device)
    for tmax in (None, 20.75):
        for entries in (0, 1):
            got = check(r, v, f, o, d, None, tmax, device, f"quads, tmax {tmax}, stack_entries {entries}", stack_entries=entries)
            CC.check_quad_stack(got, expected, tmax, f"quads, tmax {tmax}")


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "shells5"])
def test_default_bounds_are_the_direct_launches_of_the_same_handle(device, cases, name):
    v, f, o, d = cases[name][:4]
    r = make(v, f, device)
    ot, dt = T(o, device), T(d, device)
    count = r.intersects_count_range(ot, dt)
    assert torch.equal(count, r.intersects_count(ot, dt)) and int(count.max()) >= 2
    offsets, tri, t, loc = r.intersects_all_range(ot, dt, return_locations=True)
    loc8, ray8, tri8 = r.intersects_location(ot, dt)
    few = (count <= 8)
    rows = torch.repeat_interleave(few, count.long())
    assert few.sum() > 1000
    keep8 = few[ray8.long()]
    assert torch.equal(tri[rows], tri8[keep8]) and torch.equal(loc[rows].view(torch.int32), loc8[keep8].view(torch.int32))
    assert torch.equal(torch.repeat_interleave(torch.arange(len(o), device=device), count.long())[rows], ray8[keep8].long())


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_fill_with_counts_of_a_narrower_interval_stays_inside_its_rows(device, cases):
    """the caller's error: count / offsets computed for a narrower interval (and a total cut short) handed to a fill on the
    wider one.  Wrong rows are allowed; a write outside the rows of those counts is not: the guard rows stay poisoned, and
    what is written at a ray's rows are crossings of the wider interval of that ray, ordered, with their own outputs."""
    import cross_sim
    v, f, o, d, lo, hi, wide = cases["shells5"]
    lo2, hi2 = CC.narrower(lo, hi)
    small = cross_sim.brute(v, f, o, d, lo2, hi2)
    assert (wide.count >= small.count).all() and wide.offsets[-1] > 1.5 * small.offsets[-1] > 1000
    r = make(v, f, device)
    ot, dt, lt, ht = T(o, device), T(d, device), T(lo, device), T(hi, device)
    count, offsets = T(small.count, device), T(small.offsets[:-1].copy(), device)
    key = wide.ray * len(f) + wide.faces
    order = np.argsort(key)
    for total in (int(small.offsets[-1]), int(small.offsets[-1]) - 37):
        for entries in (0, 1):
            rows = guarded_fill(r, ot, dt, lt, ht, count, offsets, total, entries)
            face, t, ray = host(rows["faces"]), host(rows["t"]), host(rows["ray"])
            mine = np.repeat(np.arange(len(o)), small.count)[:total]
            assert np.array_equal(ray, mine)
            at = np.minimum(np.searchsorted(key[order], mine * len(f) + face), len(key) - 1)
            assert np.array_equal(key[order][at], mine * len(f) + face), "a row is no crossing of its ray on the wider interval"
            at = order[at]
            for k, got in (("t", t), ("front", host(rows["front"])), ("loc", host(rows["loc"])), ("uv", host(rows["uv"]))):
                assert np.array_equal(RC.bits(got), RC.bits(getattr(wide, k)[at])), k
            same_ray = mine[1:] == mine[:-1]
            assert ((t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & (face[1:] > face[:-1])))[same_ray].all()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_hostile_rays_and_bounds(device, cases):
    v, f = cases["icosphere"][:2]
    o, d, lo, hi, bad = RC.hostile_rays(*cases["icosphere"][2:6])
    r = make(v, f, device)
    for entries in (0, 1):
        got = check(r, v, f, o, d, lo, hi, device, f"hostile rays, stack_entries {entries}", stack_entries=entries)
    assert not got.count[bad].any() and (got.count[~bad] > 0).sum() > 50
    assert not np.isin(got.ray, np.flatnonzero(bad)).any() and not np.isnan(got.t).any()


HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_hostile_meshes(device, name, seed):
    c = M.case(name, seed)
    lo, hi = RC.hash_bounds(len(c.o), 97, 3.0)
    r = make(c.v, c.f, device)
    for entries in (0, 1):
        got = check(r, c.v, c.f, c.o, c.d, lo, hi, device, f"{c.name}, stack_entries {entries}", stack_entries=entries)
    assert not c.inactive[got.faces].any()          # no row names a face with a non-finite coordinate
    check(r, c.v, c.f, c.o, c.d, None, None, device, f"{c.name}, default bounds")


# ---- 9 ------------------------------------------------------------------------------------------------------------------
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
        wide = check(r, vv, ff, o, d, None, None, device, f"{nt} triangle(s), default bounds")
        if nt == 0:
            assert not got.count.any() and len(got.faces) == 0 and not wide.count.any()
        else:
            assert got.count.any() and not got.count.all() and wide.faces.max() == nt - 1 and wide.count.max() <= nt


# ---- 10 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube5", "nested3", "heightfield", "fan64"])
def test_lattice_lists_match_the_integer_arithmetic_ideal(device, name):
    s, ideal, _ = CC.lattice_lists(name)
    r = make(s["v"], s["f"], device)
    got = native(r, s["o"], s["d"], None, None, device, stack_entries=2)
    lists, ties = CC.check_lattice(name, got, f"{name}, GPU")
    assert lists == np.count_nonzero(ideal.count >= 2) > 0 and ties > 0


# ---- 11 -----------------------------------------------------------------------------------------------------------------
def test_python_methods_shapes_inputs_bounds_segments_and_errors(device, cases):
    import cross_sim
    v, f, o, d, lo, hi, want = cases["shells5"]
    r = make(v, f, device)
    n = 35

    def result(count, out, want_like):
        """the tuple of intersects_all_range(front, loc, uv) -> a Result"""
        offsets, tri, t, front, loc, uv = out
        assert offsets.dtype == torch.int64 and tri.dtype == torch.int32 and t.dtype == torch.float32 and front.dtype == torch.bool
        assert int(offsets[-1]) == len(tri) == len(t) == len(front) == len(loc) == len(uv) and loc.shape[1:] == (3,) and uv.shape[1:] == (2,)
        return cross_sim.Result(host(count).reshape(-1), host(offsets), host(tri), host(t), host(front), host(loc), host(uv), None)
    every = dict(return_front=True, return_locations=True, return_uv=True)
    # [3]: a single ray, scalar bounds
    w1 = cross_sim.brute(v, f, o[:1], d[:1], 0.25, 1.5)
    c = r.intersects_count_range(T(o[0], device), T(d[0], device), 0.25, 1.5)
    assert c.shape == () and c.dtype == torch.int32
    CC.assert_same(result(c, r.intersects_all_range(T(o[0], device), T(d[0], device), 0.25, 1.5, **every), w1), w1, "[3] with scalar bounds")
    # [5, 7, 3] with tensor bounds of the batch shape; the optional parts in the order front, loc, uv
    ot, dt = T(o[:n].reshape(5, 7, 3), device), T(d[:n].reshape(5, 7, 3), device)
    lt, ht = T(lo[:n].reshape(5, 7), device), T(hi[:n].reshape(5, 7), device)
    wn = cross_sim.brute(v, f, o[:n], d[:n], lo[:n], hi[:n])
    c = r.intersects_count_range(ot, dt, lt, ht)
    assert c.shape == (5, 7)
    CC.assert_same(result(c, r.intersects_all_range(ot, dt, lt, ht, **every), wn), wn, "[5, 7, 3]")
    plain = r.intersects_all_range(ot, dt, lt, ht)
    assert len(plain) == 3 and np.array_equal(host(plain[1]), wn.faces) and np.array_equal(RC.bits(host(plain[2])), RC.bits(wn.t))
    for kw, k, shape in ((dict(return_front=True), "front", ()), (dict(return_locations=True), "loc", (3,)), (dict(return_uv=True), "uv", (2,))):
        out = r.intersects_all_range(ot, dt, lt, ht, **kw)
        assert len(out) == 4 and out[3].shape == (len(wn.faces),) + shape and np.array_equal(RC.bits(host(out[3])), RC.bits(getattr(wn, k)))
    out = r.intersects_all_range(ot, dt, lt, ht, return_uv=True, return_front=True)
    assert len(out) == 5 and out[3].dtype == torch.bool and out[4].shape[1:] == (2,)
    # lists, numpy arrays and float64 tensors as rays; bounds that broadcast: a row [7], a numpy array, a python float, a float64 tensor
    row = hi[:7]
    wb = cross_sim.brute(v, f, o[:n], d[:n], 0.1, np.tile(row, 5))
    for oo, dd, a, b in ((ot, dt, 0.1, row), (o[:n].reshape(5, 7, 3), d[:n].reshape(5, 7, 3), np.float64(0.1), T(row.astype(np.float64), device)),
                         (o[:n].reshape(5, 7, 3).tolist(), d[:n].reshape(5, 7, 3).tolist(), 0.1, row.tolist()),
                         (T(o[:n].reshape(5, 7, 3).astype(np.float64), device), T(d[:n].reshape(5, 7, 3).astype(np.float64), device), torch.tensor(0.1), T(row, device))):
        CC.assert_same(result(r.intersects_count_range(oo, dd, a, b), r.intersects_all_range(oo, dd, a, b, **every), wb), wb, "broadcast bounds")
    wb = cross_sim.brute(v, f, o[:n], d[:n], None, 0.75)
    CC.assert_same(result(r.intersects_count_range(ot, dt, tmax=0.75), r.intersects_all_range(ot, dt, None, torch.tensor(0.75), **every), wb), wb, "tmax alone")
    # segments: the float32 difference and the range [0, 1]; t is the fraction along the segment
    p0, p1 = o[:2000], (o[:2000] + d[:2000] * hi[:2000, None]).astype(np.float32)
    so, sd, slo, shi = RC.segment_rays(p0, p1)
    ws = cross_sim.brute(v, f, so, sd, slo, shi)
    assert (ws.count > 1).sum() > 100 and (ws.count == 0).sum() > 200
    sc = r.segments_count(T(p0, device), T(p1, device))
    got = result(sc, r.segments_all(T(p0, device), T(p1, device), **every), ws)
    CC.assert_same(got, ws, "segments")
    assert ((got.t >= 0) & (got.t <= 1)).all() and len(r.segments_all(T(p0, device), T(p1, device))) == 3
    sc = r.segments_count(T(p0[:24].reshape(2, 3, 4, 3), device), T(p1[:24].reshape(2, 3, 4, 3), device))
    assert sc.shape == (2, 3, 4) and np.array_equal(host(sc).reshape(-1), ws.count[:24])
    # an empty batch
    e = torch.zeros((0, 3), dtype=torch.float32, device=device)
    assert r.intersects_count_range(e, e).shape == (0,) and r.segments_count(e, e).shape == (0,)
    out = r.intersects_all_range(e, e, **every)
    assert out[0].shape == (1,) and int(out[0][0]) == 0 and all(len(x) == 0 for x in out[1:]) and out[4].shape == (0, 3)
    assert r.intersects_count_range(torch.zeros((4, 0, 3), device=device), torch.zeros((4, 0, 3), device=device)).shape == (4, 0)
    # one count launch, one fill
    before = dict(CALLS)
    r.intersects_all_range(ot, dt, lt, ht)
    assert CALLS["cross_count_native"] == before["cross_count_native"] + 1 and CALLS["cross_fill_native"] == before["cross_fill_native"] + 1
    # errors: CPU tensors, the wrong device, shapes, bounds that do not broadcast
    calls = [lambda: r.intersects_count_range(torch.from_numpy(o[:4]), torch.from_numpy(d[:4])),
             lambda: r.intersects_all_range(torch.from_numpy(o[:4]), T(d[:4], device)),
             lambda: r.segments_count(torch.from_numpy(o[:4]), T(d[:4], device)),
             lambda: r.segments_all(T(o[:4], device), torch.from_numpy(d[:4])),
             lambda: r.intersects_count_range(T(o[:4, :2], device), T(d[:4, :2], device)),
             lambda: r.intersects_all_range(T(o[:4], device), T(d[:5], device)),
             lambda: r.segments_all(T(o[:4], device), T(o[:5], device)),
             lambda: r.intersects_count_range(ot, dt, tmin=T(lo[:6], device)),
             lambda: r.intersects_all_range(ot, dt, tmax=T(hi[:6], device))]
    if torch.cuda.device_count() > 1:
        other = torch.device("cuda", (torch.device(device).index or 0) ^ 1)
        calls += [lambda: r.intersects_count_range(ot.to(other), dt.to(other)), lambda: r.segments_all(ot.to(other), dt.to(other)),
                  lambda: r.intersects_all_range(ot, dt, tmin=lt.to(other))]
    for call in calls:
        with pytest.raises(ValueError):
            call()


# ---- 12 -----------------------------------------------------------------------------------------------------------------
def test_lifecycle_refit_update_and_load(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
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
    path = str(tmp_path / "mesh.npz")
    r.save(path)
    check(RayMeshIntersector.load(path, device=device), v2, f, o, d, lo, hi, device, "loaded")
    v3, f3 = RC.sheets()
    r.update_raw(T(v3, device), T(f3, device))
    so, sd, slo, shi, _, count = RC.sheet_cases("interior")
    got = check(r, v3, f3, so, sd, slo, shi, device, "update_raw to another mesh")
    CC.check_sheets(got, slo, shi, count, "update_raw to another mesh")


# ---- 13 -----------------------------------------------------------------------------------------------------------------
def test_the_first_calls_of_a_fresh_intersector_can_be_captured(device):
    import cross_sim
    import triro.backend.ops as hops
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=5, amplitude=0.05)
    n = 1000
    o1, d1 = W.hash_rays(n, 29, v.min(0), v.max(0))
    o2, d2 = W.hash_rays(n, 31, v.min(0), v.max(0))
    b1, b2 = RC.hash_bounds(n, 33, 3.0), RC.hash_bounds(n, 35, 3.0)
    steps = ((o1, d1, b1), (o2, d2, b2))
    wants = [cross_sim.brute(v, f, o, d, lo, hi, ray_base=5) for o, d, (lo, hi) in steps]
    rows = max(int(w.offsets[-1]) for w in wants) + 64
    # the count, captured as the very first call on a fresh intersector
    r = make(v, f, device)
    ot, dt, lt, ht = T(o1, device), T(d1, device), T(b1[0], device), T(b1[1], device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the call neither allocates nor synchronises
        count = hops.cross_count_native(r.as_wrapper, ot, dt, lt, ht)
    # the fill with known counts, captured as the very first call on another fresh intersector
    r2 = make(v, f, device)
    count_in = torch.zeros(n, dtype=torch.int32, device=device)
    offsets_in = torch.zeros(n, dtype=torch.int64, device=device)
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=side):
        face, t, front, loc, uv, ray = hops.cross_fill_native(r2.as_wrapper, ot, dt, lt, ht, count_in, offsets_in, rows, True, True, True, True, 5)
    for step, ((o, d, (lo, hi)), want) in enumerate(zip(steps, wants)):
        for src, dst in ((o, ot), (d, dt), (lo, lt), (hi, ht)):
            dst.copy_(T(src, device))
        count_in.copy_(T(want.count, device))
        offsets_in.copy_(T(want.offsets[:-1].copy(), device))
        graph.replay()
        graph2.replay()
        torch.cuda.synchronize()
        total = int(want.offsets[-1])
        assert 0 < total <= rows - 64
        outs = (face, t, front, loc, uv, ray)
        poison.assert_written(count, *(x[:total] for x in outs), what=f"graph replay {step}")
        for name, x in zip(("face", "t", "front", "loc", "uv", "ray"), outs):
            assert poison.stale_mask(x[total:]).all(), f"graph replay {step}: {name} rows beyond the total were written"
        got = cross_sim.Result(host(count), want.offsets, *(host(x[:total]) for x in outs))
        CC.assert_same(got, want, f"graph replay {step}")
        # ... and the eager results
        eager = native(r, o, d, lo, hi, device, ray_base=5)
        CC.assert_same(got, eager, f"graph replay {step} against the eager calls")
