"""triangles_any / triangles_count / faces_meeting_triangles / mesh_collides / mesh_contacts (libtriro_tris.so: k_tris<>,
k_tris_rows) against the host brute force.

The oracle of every comparison is tests/host_sim/tris_sim.brute: the predicate of csrc/tr_tris.h over every active triangle,
on the same float32 inputs -- itself pinned to an exact integer reference that is no separating-axis test by
tests/test_tris_cpu.py, and once more here on the GPU's own results.  Comparisons are element for element (any, count, offsets,
faces): there is no tolerance.  Every native call of this module comes back through a wrapper that runs poison.assert_written
on its outputs (the autouse fixture `checked_native`); captured calls are checked after each replay."""
import numpy as np
import pytest
import torch

import hostile_meshes as M
import nearest_cases as NC
import poison
import tris_cases as TC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("tris_native", "tris_fill_native")
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


def native(r, tri, device, stack_entries=0):
    """every entry once -> a tris_sim.Result of numpy arrays"""
    import tris_sim
    import triro.backend.ops as hops
    tt = T(tris_sim.triangles(tri).reshape(-1, 3, 3), device)
    any_ = hops.tris_native(r.as_wrapper, tt, "any", stack_entries)
    count = hops.tris_native(r.as_wrapper, tt, "count", stack_entries)
    offsets, face = hops.faces_meeting_triangles_native(r.as_wrapper, tt, stack_entries)
    torch.cuda.synchronize()
    poison.assert_written(offsets, what="faces_meeting_triangles_native offsets")
    assert any_.dtype == torch.bool and count.dtype == torch.int32 and offsets.dtype == torch.int64 and face.dtype == torch.int32
    return tris_sim.Result(host(any_), host(count), host(offsets), host(face))


def check(r, v, f, tri, device, what, want=None, **kw):
    import tris_sim
    want = tris_sim.brute(v, f, tri) if want is None else want
    got = native(r, tri, device, **kw)
    TC.assert_same(got, want, what)
    return got


@pytest.fixture(scope="module")
def cases():
    """{case: (v, f, [(label, triangles, brute force)])}, computed once"""
    import tris_sim
    out = {}
    for name, mk in TC.CASES.items():
        v, f, _ = mk()
        out[name] = (v, f, [(label, tri, tris_sim.brute(v, f, tri)) for label, tri in TC.query_sets(v, f)])
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.CASES))
def test_kernels_match_the_brute_force_at_every_stack_limit(device, cases, name):
    v, f, rows = cases[name]
    r = make(v, f, device)
    if name == "deep":
        assert r.bvh_info()["depth"] > 32
    for label, tri, want in rows:
        for entries in (0, 1, 2):
            check(r, v, f, tri, device, f"{name}, {label}, stack_entries {entries}", want=want, stack_entries=entries)
    assert rows[0][2].count.min() >= (0 if name in ("soup", "deep") else 1)          # an own face with area meets itself


def test_kernels_match_the_host_walk_on_the_gpu_builders_tree(device, cases):
    import tris_sim
    from sim import SimBVH
    v, f, rows = cases["icosphere"]
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    for label, tri, want in rows[2:]:
        for entries in (0, 1):
            walked = tris_sim.walk(B, tri, entries)
            TC.assert_same(native(r, tri, device, stack_entries=entries), walked, f"GPU tree, {label}, stack_entries {entries}")
            TC.assert_same(walked, want, "host walk on the GPU tree against the brute force")


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_case():
    import tris_sim
    v, f, _ = NC.icosphere()
    tri = TC.hashed_triangles(4133, [-1.2] * 3, [1.2] * 3, TC.extent(v), seed=1)
    return v, f, tri, tris_sim.brute(v, f, tri)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, tail_case, n):
    import tris_sim
    v, f, tri, whole = tail_case
    r = make(v, f, device)
    total = int(whole.offsets[n])
    want = tris_sim.Result(whole.any[:n], whole.count[:n], whole.offsets[:n + 1], whole.faces[:total])
    got = check(r, v, f, tri[:n], device, f"{n} triangles", want=want)
    assert got.any.shape == (n,) and got.count.shape == (n,) and got.offsets.shape == (n + 1,) and got.faces.shape == (total,)
    if n == 4133:
        assert total > 2000 and (want.count == 0).any() and want.count.max() > 8


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_meshes_without_a_hierarchy(device):
    v, f = W.two_triangles()
    for nt in (2, 1, 0):
        vv, ff = v[:3 * nt], f[:nt]
        r = make(vv, ff, device)
        seen = set()
        for label, tri in TC.query_sets(v, f):
            tri = np.concatenate([tri, np.full((1, 3, 3), np.nan, np.float32)])
            for entries in (0, 1):
                got = check(r, vv, ff, tri, device, f"{nt} triangle(s), {label}", stack_entries=entries)
            seen |= set(np.unique(got.count))
            assert got.count[-1] == 0 and not got.any[-1]
        assert seen == set(range(nt + 1))
        if nt == 0:
            assert len(got.faces) == 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_hostile_triangles(device):
    v, f, _ = NC.icosphere()
    r = make(v, f, device)
    tri, valid, degenerate = TC.hostile_triangles(TC.hashed_triangles(704, v.min(0), v.max(0), TC.extent(v), seed=3))
    tri[128:192] = np.nan                                 # a whole wave of invalid queries ...
    tri[256:384, 2] = tri[256:384, 1]                     # ... a whole block of degenerate ones (a doubled vertex) ...
    tri[448:512] = tri[448:512, :1]                       # ... and a whole wave of points
    valid = np.isfinite(tri).all(axis=(1, 2))
    degenerate[256:384] = True
    degenerate[448:512] = True
    assert (~valid).sum() == 27 + 64 and degenerate.sum() == 5 + 128 + 64
    for entries in (0, 1):
        got = check(r, v, f, tri, device, f"hostile triangles, stack_entries {entries}", stack_entries=entries)
    assert not got.any[~valid].any() and not got.count[~valid].any() and not got.count[degenerate].any()
    assert got.count[32] > 0 and got.count[33] > 0 and got.count[34] == 0
    live = valid & ~degenerate
    assert got.any[live].sum() >= 10 and (~got.any[live]).sum() >= 10
    # +-FLT_MAX on the mesh's side
    bv, bf = tri[32:37].reshape(-1, 3), np.arange(15, dtype=np.int32).reshape(-1, 3)
    back = check(make(bv, bf, device), bv, bf, tri, device, "a mesh of huge triangles", stack_entries=1)
    assert back.count[32:37].min() >= 1


# ---- 5 ------------------------------------------------------------------------------------------------------------------
HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_hostile_meshes(device, name, seed):
    c = M.case(name, seed)
    fa, _ = M.active_faces(c.v, c.f)
    r = make(c.v, c.f, device)
    for tri in TC.hostile_mesh_triangles(c, fa):
        for entries in (0, 1, 3):
            got = check(r, c.v, c.f, tri, device, f"{c.name}, stack_entries {entries}", stack_entries=entries)
        assert not c.inactive[got.faces].any()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_snapped_inputs_equal_the_exact_reference(device):
    """inputs on the grid k * 2^-10, |k| <= 2^11 (asserted by tris_cases.snapped), where every float64 operation of the
    predicate is exact: the kernels must EQUAL the exact integer reference pair for pair, pairs that only touch and coplanar
    pairs included"""
    stats = TC.check_snapped(lambda v, f, tri: native(make(v, f, device), tri, device, stack_entries=2), "GPU")
    print("(pairs, met, only touching, coplanar) per mesh:", stats)
    print("(pairs, met, only touching, coplanar) in all:", TC.check_coverage(stats))


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_fill_with_counts_of_other_queries_stays_inside_its_rows(device, cases):
    """the caller's error: count / offsets computed for other queries (and a total cut short) handed to a fill.  Wrong rows are
    allowed; a write outside the rows of those counts is not: guard rows on both sides stay poisoned, and no row >= total is
    written."""
    import triro.backend.ops as hops
    v, f, rows = cases["icosphere"]
    r = make(v, f, device)
    lib = hops.get_tris_module()
    G = 4096
    # the own faces (12 or 13 faces each) with the counts of the displaced ones (at most 5): every list is cut; and the
    # displaced ones with the counts of the own faces: every list leaves rows alone
    for a_, b_ in ((0, 1), (1, 0)):
        (_, mine, own), (_, _, other) = rows[a_], rows[b_]
        n = len(mine)
        assert len(other.count) == n and other.offsets[-1] > 40
        assert (own.count > other.count).all() if a_ == 0 else (own.count < other.count).all()
        tt = T(mine, device)
        count, offsets = T(other.count, device), T(other.offsets[:-1].copy(), device)
        for total in (int(other.offsets[-1]), int(other.offsets[-1]) - 37):
            for entries in (0, 1):
                face = poison.poisoned((G + total + G,), torch.int32, device)
                with torch.cuda.device(device):
                    rc = lib.tr_tris_fill(r.as_wrapper._inner, tt.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total,
                                          face.data_ptr() + 4 * G, entries, hops._stream_ptr(device))
                assert rc == 0, hops.get_module().tr_last_error()
                torch.cuda.synchronize()
                stale = host(poison.stale_mask(face))
                assert stale[:G].all() and stale[G + total:].all(), f"a guard row was written (total {total}, stack_entries {entries})"
                # wrong rows, but rows: query i wrote min(its own count, the rows handed to it) faces of its own list; the
                # ordering pass sorted its whole segment, rows left alone (poison, a negative number) first
                got = host(face)[G:G + total]
                for i in range(n):
                    a, b = int(other.offsets[i]), min(int(other.offsets[i + 1]), total)
                    if b <= a:
                        continue
                    seg = got[a:b]
                    written = seg[~stale[G + a:G + b]]
                    true = own.faces[own.offsets[i]:own.offsets[i + 1]]
                    assert len(written) == min(len(true), b - a), (i, total, entries)
                    assert (np.diff(written) > 0).all() and np.isin(written, true).all()
                    assert (seg[:len(seg) - len(written)] == poison.INT32).all()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_python_methods_batch_shapes_and_input_types(device, cases):
    import tris_sim
    v, f, rows = cases["icosphere"]
    label, tri, want = rows[1]                        # own faces displaced by 1/32 of the extent
    r = make(v, f, device)
    a, n = r.triangles_any(T(tri[0], device)), r.triangles_count(T(tri[0], device))
    assert a.shape == () and a.dtype == torch.bool and n.shape == () and n.dtype == torch.int32
    assert bool(a) == bool(want.any[0]) and int(n) == int(want.count[0])
    out = r.faces_meeting_triangles(T(tri[0], device))
    assert len(out) == 2 and out[0].shape == (2,) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32
    assert np.array_equal(host(out[1]), want.faces[:want.count[0]])

    def flat(t, shape):
        """the three methods on one batch -> a Result of flat numpy arrays (the batch shape is checked)"""
        a, n = r.triangles_any(t), r.triangles_count(t)
        off, idx = r.faces_meeting_triangles(t)
        assert tuple(a.shape) == shape and tuple(n.shape) == shape
        return tris_sim.Result(host(a).reshape(-1), host(n).reshape(-1), host(off), host(idx))
    TC.assert_same(flat(T(tri[:35].reshape(5, 7, 3, 3), device), (5, 7)), tris_sim.brute(v, f, tri[:35]), "[5, 7, 3, 3]")
    wide = torch.zeros((60, 3, 8), dtype=torch.float32, device=device)
    wide[:, :, 2:5] = T(tri[:60], device)
    assert not wide[::2, :, 2:5].is_contiguous()
    TC.assert_same(flat(wide[::2, :, 2:5], (30,)), tris_sim.brute(v, f, tri[:60:2]), "non-contiguous slices")
    TC.assert_same(flat(T(tri[:50].astype(np.float64), device), (50,)), tris_sim.brute(v, f, tri[:50]), "float64 input")
    TC.assert_same(flat(tri[:50], (50,)), tris_sim.brute(v, f, tri[:50]), "numpy input")
    TC.assert_same(flat(T(tri[:0], device), (0,)), tris_sim.brute(v, f, tri[:0]), "no triangles")
    # refusals
    calls = [lambda: r.triangles_any(torch.from_numpy(tri[:4])), lambda: r.triangles_count(torch.from_numpy(tri[:4])),
             lambda: r.faces_meeting_triangles(torch.from_numpy(tri[:4])),
             lambda: r.triangles_any(T(tri[:4, :2], device)), lambda: r.triangles_count(T(tri[:4].reshape(4, 9), device)),
             lambda: r.faces_meeting_triangles(T(tri[:4, :, :2], device)), lambda: r.triangles_any(T(tri[0, 0], device))]
    if torch.cuda.device_count() > 1:                 # a tensor on another GPU raises
        other = torch.device("cuda", (torch.device(device).index or 0) ^ 1)
        calls += [lambda: r.triangles_any(T(tri[:4], other)), lambda: r.faces_meeting_triangles(T(tri[:4], other))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    # one count launch, one fill
    before = dict(CALLS)
    r.faces_meeting_triangles(T(tri, device))
    assert CALLS["tris_native"] == before["tris_native"] + 1 and CALLS["tris_fill_native"] == before["tris_fill_native"] + 1


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_mesh_collides_and_mesh_contacts(device):
    import tris_sim
    v, f, _ = NC.icosphere()
    r = make(v, f, device)
    ext = TC.extent(v)
    near = (v + np.float32([0.3, -0.1, 0.2]) * np.float32(ext / 4)).astype(np.float32)
    far = (v + np.float32([5.0, 0.0, 0.0]) * np.float32(ext)).astype(np.float32)
    # the other mesh with its faces in another order and a vertex nobody uses
    f2 = np.ascontiguousarray(f[::-1])
    for name, vv in (("displaced", near), ("far away", far)):
        vv = np.concatenate([vv, np.float32([[9, 9, 9]])])
        want = tris_sim.brute(v, f, vv[f2])
        pairs = np.stack([np.repeat(np.arange(len(f2)), want.count), want.faces.astype(np.int64)], 1)
        assert (len(pairs) > 40) if name == "displaced" else (len(pairs) == 0)
        for chunk in (1 << 20, 7):
            got = r.mesh_contacts(T(vv, device), T(f2, device), chunk=chunk)
            assert got.dtype == torch.int64 and got.device.type == "cuda" and tuple(got.shape) == (len(pairs), 2)
            g = host(got)
            assert np.array_equal(g, pairs), f"{name}, chunk {chunk}"
            if len(g) > 1:      # lexicographic: the other mesh's face first, then this mesh's
                d = np.diff(g, axis=0)
                assert ((d[:, 0] > 0) | ((d[:, 0] == 0) & (d[:, 1] > 0))).all()
            assert r.mesh_collides(T(vv, device), T(f2, device), chunk=chunk) is (len(pairs) > 0)
        assert np.array_equal(host(r.mesh_contacts(vv, f2.astype(np.int64))), pairs)           # numpy input
    # the first chunk that says yes ends mesh_collides
    before = CALLS["tris_native"]
    assert r.mesh_collides(T(near, device), T(f, device), chunk=16) is True
    assert CALLS["tris_native"] - before < len(f) // 16
    assert r.mesh_contacts(T(near, device), T(f[:0], device)).shape == (0, 2) and r.mesh_collides(T(near, device), T(f[:0], device)) is False
    for bad in (lambda: r.mesh_contacts(T(near, device), T(f, device), chunk=0), lambda: r.mesh_collides(T(near[:5], device), T(f, device)),
                lambda: r.mesh_contacts(T(near[:, :2], device), T(f, device)), lambda: r.mesh_collides(T(near, device), T(f[:, :2], device))):
        with pytest.raises(ValueError):
            bad()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_lifecycle_refit_update_and_load(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    tri = TC.hashed_triangles(1500, [-1.4] * 3, [1.6] * 3, 2.0, seed=2)
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
def test_the_first_calls_of_a_fresh_intersector_can_be_captured(device):
    import tris_sim
    import triro.backend.ops as hops
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=5, amplitude=0.05)
    v2 = (v * np.float32(1.6) + np.float32([0.3, 0.0, -0.2])).astype(np.float32)
    n = 1000
    t1 = TC.hashed_triangles(n, [-1.4] * 3, [1.4] * 3, 1.6, seed=4)
    t2 = TC.hashed_triangles(n, [-2.0] * 3, [2.0] * 3, 1.6, seed=5)
    r = make(v, f, device)
    tt = T(t1, device)
    # the rows of the captured fill: preallocated for the largest total of the four steps, counts and offsets refreshed per step
    steps = ((v, t1), (v, t2), (v2, t2), (v2, t1))
    wants = [tris_sim.brute(vv, f, q) for vv, q in steps]
    rows = max(int(w.offsets[-1]) for w in wants) + 64
    count_in = torch.zeros(n, dtype=torch.int32, device=device)
    offsets_in = torch.zeros(n, dtype=torch.int64, device=device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the calls neither allocate nor synchronise
        any_ = hops.tris_native(r.as_wrapper, tt, "any")
        count = hops.tris_native(r.as_wrapper, tt, "count")
        face = hops.tris_fill_native(r.as_wrapper, tt, count_in, offsets_in, rows)
    for step, ((vv, q), want) in enumerate(zip(steps, wants)):
        if step == 2:
            r.refit(T(vv, device))                      # moves the bounds
        tt.copy_(T(q, device))
        count_in.copy_(T(want.count, device))
        offsets_in.copy_(T(want.offsets[:-1].copy(), device))
        graph.replay()
        torch.cuda.synchronize()
        total = int(want.offsets[-1])
        assert 0 < total <= rows - 64
        poison.assert_written(any_, count, face[:total], what=f"graph replay {step}")
        assert poison.stale_mask(face[total:]).all(), f"graph replay {step}: rows beyond the total were written"
        got = tris_sim.Result(host(any_), host(count), want.offsets, host(face[:total]))
        TC.assert_same(got, want, f"graph replay {step}")
