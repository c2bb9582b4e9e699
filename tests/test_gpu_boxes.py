"""boxes_any / boxes_count / faces_in_boxes / surface_voxels (libtriro_boxes.so: k_boxes<>, k_boxes_rows) against the host brute
force.

The oracle of every comparison is tests/host_sim/boxes_sim.brute: the predicate of csrc/tr_boxes.h over every active triangle,
on the same float32 inputs -- itself pinned to an exact integer reference that is no separating-axis test by
tests/test_boxes_cpu.py, and once more here on the GPU's own results.  Comparisons are element for element (any, count, offsets,
faces, inside).  Every native call of this module comes back through a wrapper that runs poison.assert_written on its outputs
(the autouse fixture `checked_native`); captured calls are checked after each replay."""
import numpy as np
import pytest
import torch

import boxes_cases as BC
import hostile_meshes as M
import nearest_cases as NC
import poison
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("boxes_native", "boxes_fill_native")
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


def native(r, lo, hi, device, stack_entries=0, want_inside=True):
    """every entry once -> a boxes_sim.Result of numpy arrays"""
    import boxes_sim
    import triro.backend.ops as hops
    lo, hi = boxes_sim.boxes(lo, hi)
    lt, ht = T(lo, device), T(hi, device)
    any_ = hops.boxes_native(r.as_wrapper, lt, ht, "any", stack_entries)
    count = hops.boxes_native(r.as_wrapper, lt, ht, "count", stack_entries)
    offsets, face, inside = hops.faces_in_boxes_native(r.as_wrapper, lt, ht, want_inside, stack_entries)
    torch.cuda.synchronize()
    poison.assert_written(offsets, what="faces_in_boxes_native offsets")
    assert any_.dtype == torch.bool and count.dtype == torch.int32 and offsets.dtype == torch.int64 and face.dtype == torch.int32
    assert inside is None or inside.dtype == torch.bool
    return boxes_sim.Result(host(any_), host(count), host(offsets), host(face), host(inside))


def check(r, v, f, lo, hi, device, what, want=None, **kw):
    import boxes_sim
    want = boxes_sim.brute(v, f, lo, hi) if want is None else want
    got = native(r, lo, hi, device, **kw)
    BC.assert_same(got, want, what)
    return got


@pytest.fixture(scope="module")
def cases():
    """{case: (v, f, [(label, lo, hi, brute force)])}, computed once"""
    import boxes_sim
    out = {}
    for name, mk in BC.CASES.items():
        v, f, p = mk()
        out[name] = (v, f, [(label, lo, hi, boxes_sim.brute(v, f, lo, hi)) for label, lo, hi in BC.box_sets(v, p)])
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.CASES))
def test_kernels_match_the_brute_force_at_every_stack_limit(device, cases, name):
    v, f, rows = cases[name]
    r = make(v, f, device)
    if name == "deep":
        assert r.bvh_info()["depth"] > 32
    for label, lo, hi, want in rows:
        for entries in (0, 1, 2):
            check(r, v, f, lo, hi, device, f"{name}, {label}, stack_entries {entries}", want=want, stack_entries=entries)


def test_kernels_match_the_host_walk_on_the_gpu_builders_tree(device, cases):
    import boxes_sim
    from sim import SimBVH
    v, f, rows = cases["icosphere"]
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    for label, lo, hi, want in rows[2:]:
        for entries in (0, 1):
            walked = boxes_sim.walk(B, lo, hi, entries)
            BC.assert_same(native(r, lo, hi, device, stack_entries=entries), walked, f"GPU tree, {label}, stack_entries {entries}")
            BC.assert_same(walked, want, "host walk on the GPU tree against the brute force")


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_case():
    v, f, _ = NC.icosphere()
    p = NC.hash_points(4133, 3, [-1.4] * 3, [1.4] * 3)
    lo, hi = BC.hashed_boxes(p, 2 * BC.extent(v), seed=1)
    return v, f, lo, hi


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, tail_case, n):
    import boxes_sim
    v, f, lo, hi = tail_case
    r = make(v, f, device)
    want = boxes_sim.brute(v, f, lo[:n], hi[:n])
    got = check(r, v, f, lo[:n], hi[:n], device, f"{n} boxes", want=want)
    total = int(want.offsets[-1])
    assert got.any.shape == (n,) and got.count.shape == (n,) and got.offsets.shape == (n + 1,)
    assert got.faces.shape == (total,) and got.inside.shape == (total,)
    if n == 4133:
        assert total > 10000 and 0 < want.inside.sum() < total and (want.count == 0).any()
    # without the optional output (every row 0 .. total of what is given is written: checked_native)
    g = native(r, lo[:n], hi[:n], device, want_inside=False)
    assert g.inside is None
    BC.assert_same(g, want, f"{n} boxes, faces only")


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_meshes_without_a_hierarchy(device):
    v, f = W.two_triangles()
    p = np.concatenate([NC.hash_points(300, 5, [-0.8, -0.8, -1.4], [0.8, 0.8, 0.4]),
                        np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.5, -0.5, 0.0], [np.nan, 0.0, 0.0]], np.float32)])
    for nt in (2, 1, 0):
        vv, ff = v[:3 * nt], f[:nt]
        r = make(vv, ff, device)
        seen = set()
        for label, lo, hi in BC.box_sets(v, p):
            if label == "the whole mesh":
                lo, hi = lo.copy(), hi.copy()
                lo[-1, 0] = np.nan
            for entries in (0, 1):
                got = check(r, vv, ff, lo, hi, device, f"{nt} triangle(s), {label}", stack_entries=entries)
            seen |= set(np.unique(got.count))
            assert got.count[-1] == 0 and not got.any[-1]
        assert seen == set(range(nt + 1))
        if nt == 0:
            assert len(got.faces) == 0 and len(got.inside) == 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_hostile_boxes(device):
    v, f, _ = NC.icosphere()
    r = make(v, f, device)
    p = NC.hash_points(454, 17, [-1.3] * 3, [1.3] * 3)
    lo0, hi0 = BC.hashed_boxes(p, BC.extent(v), seed=3)
    lo, hi, valid, whole = BC.hostile_boxes(lo0, hi0)
    lo[128:192] = np.nan                                  # a whole wave of invalid boxes ...
    hi[256:384, 1] = lo[256:384, 1] - np.float32(1.0)     # ... and a whole block of boxes with lo > hi
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(lo).all(1) & np.isfinite(hi).all(1) & (lo <= hi).all(1)
    assert (~valid).sum() == 24 + 64 + 128
    for entries in (0, 1):
        got = check(r, v, f, lo, hi, device, f"hostile boxes, stack_entries {entries}", stack_entries=entries)
    assert not got.any[~valid].any() and not got.count[~valid].any()
    assert (got.count[whole] == len(f)).all() and got.inside[got.offsets[24]:got.offsets[25]].all()
    assert got.count[27] == 0 and got.count[28] >= 2 and got.count[30] == 0
    assert got.any[valid].sum() >= 10 and (~got.any[valid]).sum() >= 10


# ---- 5 ------------------------------------------------------------------------------------------------------------------
HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_hostile_meshes(device, name, seed):
    c = M.case(name, seed)
    fa, _ = M.active_faces(c.v, c.f)
    ext = BC.extent(c.v[np.unique(fa)]) if len(fa) else 1.0
    big = np.full((len(c.p), 3), BC.FLT_MAX, np.float32)
    r = make(c.v, c.f, device)
    for k, (lo, hi) in enumerate((BC.hashed_boxes(c.p, 2 * ext, seed=3), (-big, big))):
        for entries in (0, 1, 3):
            got = check(r, c.v, c.f, lo, hi, device, f"{c.name}, stack_entries {entries}", stack_entries=entries)
        assert not c.inactive[got.faces].any()
        if k == 1:
            assert (got.count == len(fa)).all() and got.inside.all()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_snapped_inputs_equal_the_exact_reference(device):
    """inputs on the grid k * 2^-10, |k| <= 2^12 (asserted by boxes_cases.snapped), where every float64 operation of the
    predicate is exact: the kernels must EQUAL the exact integer reference, pairs that only touch included"""
    stats = BC.check_snapped(lambda v, f, lo, hi: native(make(v, f, device), lo, hi, device, stack_entries=2), "GPU")
    print("(pairs, met, only touching) per mesh:", stats)
    assert all(t > 100 for _, _, t in stats.values())


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_fill_with_counts_of_smaller_boxes_stays_inside_its_rows(device, cases):
    """the caller's error: count / offsets computed for smaller boxes (and a total cut short) handed to a fill with larger ones.
    Wrong rows are allowed; a write outside the rows of those counts is not: guard rows on both sides stay poisoned."""
    import triro.backend.ops as hops
    v, f, rows = cases["soup"]
    r = make(v, f, device)
    (_, _, _, small), (_, llo, lhi, large) = rows[2], rows[3]              # half sizes 1/8 and 1/2 of the extent
    n = len(llo)
    assert (large.count >= small.count).all() and large.offsets[-1] > 4 * small.offsets[-1] > 0
    lib = hops.get_boxes_module()
    lt, ht = T(llo, device), T(lhi, device)
    count, offsets = T(small.count, device), T(small.offsets[:-1].copy(), device)
    G = 4096
    for total in (int(small.offsets[-1]), int(small.offsets[-1]) - 37):
        face = poison.poisoned((G + total + G,), torch.int32, device)
        inside = poison.poisoned((G + total + G,), torch.bool, device)
        for entries in (0, 1):
            with torch.cuda.device(device):
                rc = lib.tr_boxes_fill(r.as_wrapper._inner, lt.data_ptr(), ht.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total,
                                       face.data_ptr() + 4 * G, inside.data_ptr() + G, entries, hops._stream_ptr(device))
            assert rc == 0, hops.get_module().tr_last_error()
            torch.cuda.synchronize()
            for name, t in (("face", face), ("inside", inside)):
                stale = poison.stale_mask(t)
                assert stale[:G].all() and stale[G + total:].all(), f"{name}: a guard row was written (total {total}, stack_entries {entries})"
                assert not stale[G:G + total].any(), f"{name}: a row inside was not written"
            # wrong rows, but rows: each box got faces that meet the large box, ascending, with their own inside flags
            got, gi = host(face)[G:G + total], host(inside)[G:G + total]
            for i in (0, 1, 2, n // 2, n - 1):
                a, b = int(small.offsets[i]), min(int(small.offsets[i + 1]), total)
                mine = large.faces[large.offsets[i]:large.offsets[i + 1]]
                assert (np.diff(got[a:b]) > 0).all() and np.isin(got[a:b], mine).all()
                at = large.offsets[i] + np.searchsorted(mine, got[a:b])
                assert np.array_equal(gi[a:b], large.inside[at])


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_python_methods_batch_shapes_and_input_types(device, cases):
    import boxes_sim
    v, f, rows = cases["icosphere"]
    label, lo, hi, want = rows[3]                     # half size 1/2 of the extent
    r = make(v, f, device)
    a, n = r.boxes_any(T(lo[0], device), T(hi[0], device)), r.boxes_count(T(lo[0], device), T(hi[0], device))
    assert a.shape == () and a.dtype == torch.bool and n.shape == () and n.dtype == torch.int32
    assert bool(a) == bool(want.any[0]) and int(n) == int(want.count[0])
    out = r.faces_in_boxes(T(lo[0], device), T(hi[0], device), return_inside=True)
    assert len(out) == 3 and out[0].shape == (2,) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32 and out[2].dtype == torch.bool
    assert np.array_equal(host(out[1]), want.faces[:want.count[0]]) and np.array_equal(host(out[2]), want.inside[:want.count[0]])
    assert len(r.faces_in_boxes(T(lo[:3], device), T(hi[:3], device))) == 2

    def flat(lo_, hi_, shape):
        """the three methods on one batch -> a Result of flat numpy arrays (the batch shape is checked)"""
        a, n = r.boxes_any(lo_, hi_), r.boxes_count(lo_, hi_)
        off, tri, ins = r.faces_in_boxes(lo_, hi_, return_inside=True)
        assert tuple(a.shape) == shape and tuple(n.shape) == shape
        return boxes_sim.Result(host(a).reshape(-1), host(n).reshape(-1), host(off), host(tri), host(ins))
    BC.assert_same(flat(T(lo[:35].reshape(5, 7, 3), device), T(hi[:35].reshape(5, 7, 3), device), (5, 7)),
                   boxes_sim.brute(v, f, lo[:35], hi[:35]), "[5, 7, 3]")
    wide = torch.zeros((200, 8), dtype=torch.float32, device=device)
    wide[:, 1:4] = T(lo[:200], device)
    wide[:, 4:7] = T(hi[:200], device)
    assert not wide[::2, 1:4].is_contiguous()
    BC.assert_same(flat(wide[::2, 1:4], wide[::2, 4:7], (100,)), boxes_sim.brute(v, f, lo[:200:2], hi[:200:2]), "non-contiguous slices")
    BC.assert_same(flat(T(lo[:100].astype(np.float64), device), T(hi[:100].astype(np.float64), device), (100,)),
                   boxes_sim.brute(v, f, lo[:100], hi[:100]), "float64 input")
    BC.assert_same(flat(lo[:50], hi[:50], (50,)), boxes_sim.brute(v, f, lo[:50], hi[:50]), "numpy input")
    BC.assert_same(flat(lo[:50], T(hi[:50], device), (50,)), boxes_sim.brute(v, f, lo[:50], hi[:50]), "numpy lo, GPU hi")
    # lo against hi: one lower corner for seven upper ones per row, and one upper corner for all
    lo5 = lo[:5].reshape(5, 1, 3)
    hi57 = (lo[:5].reshape(5, 1, 3) + np.float32([0.0, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2]).reshape(1, 7, 1)).astype(np.float32)
    BC.assert_same(flat(T(lo5, device), T(hi57, device), (5, 7)),
                   boxes_sim.brute(v, f, np.broadcast_to(lo5, (5, 7, 3)).reshape(-1, 3), hi57.reshape(-1, 3)), "lo [5, 1, 3] against hi [5, 7, 3]")
    top = np.float32([2.0, 2.0, 2.0])
    BC.assert_same(flat(T(lo[:35].reshape(5, 7, 3), device), T(top, device), (5, 7)),
                   boxes_sim.brute(v, f, lo[:35], np.tile(top, (35, 1))), "hi [3] against lo [5, 7, 3]")
    BC.assert_same(flat(T(-top, device), T(hi[:9], device), (9,)), boxes_sim.brute(v, f, np.tile(-top, (9, 1)), hi[:9]), "lo [3] against hi [9, 3]")
    # refusals
    calls = [lambda: r.boxes_any(torch.from_numpy(lo[:4]), T(hi[:4], device)), lambda: r.boxes_count(T(lo[:4], device), torch.from_numpy(hi[:4])),
             lambda: r.faces_in_boxes(torch.from_numpy(lo[:4]), torch.from_numpy(hi[:4])),
             lambda: r.boxes_any(T(lo[:4, :2], device), T(hi[:4], device)), lambda: r.boxes_count(T(lo[:4], device), T(hi[:3], device)),
             lambda: r.faces_in_boxes(T(lo[:4], device), T(hi[:4].reshape(-1), device))]
    if torch.cuda.device_count() > 1:                 # a tensor on another GPU raises
        other = torch.device("cuda", (torch.device(device).index or 0) ^ 1)
        calls += [lambda: r.boxes_any(T(lo[:4], other), T(hi[:4], device)), lambda: r.boxes_count(T(lo[:4], device), T(hi[:4], other)),
                  lambda: r.faces_in_boxes(T(lo[:4], other), T(hi[:4], other))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    # one count launch, one fill
    before = dict(CALLS)
    r.faces_in_boxes(T(lo, device), T(hi, device))
    assert CALLS["boxes_native"] == before["boxes_native"] + 1 and CALLS["boxes_fill_native"] == before["boxes_fill_native"] + 1


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_refit_update_and_load(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    p = NC.hash_points(1500, 23, [-1.4] * 3, [1.6] * 3)
    lo, hi = BC.hashed_boxes(p, 3.0, seed=2)
    r = make(v, f, device)
    check(r, v, f, lo, hi, device, "built")
    r.refit(T(v2, device))
    check(r, v2, f, lo, hi, device, "after a refit with moved vertices")
    check(r, v2, f, lo, hi, device, "after a refit, one stack entry", stack_entries=1)
    path = str(tmp_path / "mesh.npz")
    r.save(path)
    check(RayMeshIntersector.load(path, device=device), v2, f, lo, hi, device, "loaded")
    v3, f3, _ = NC.soup_with_degenerates()
    r.update_raw(T(v3, device), T(f3, device))
    check(r, v3, f3, lo, hi, device, "update_raw to another mesh")


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_the_first_calls_of_a_fresh_intersector_can_be_captured(device):
    import boxes_sim
    import triro.backend.ops as hops
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=5, amplitude=0.05)
    v2 = (v * np.float32(1.6) + np.float32([0.3, 0.0, -0.2])).astype(np.float32)
    b1 = BC.hashed_boxes(NC.hash_points(1000, 29, [-1.4] * 3, [1.4] * 3), 2.4, seed=4)
    b2 = BC.hashed_boxes(NC.hash_points(1000, 31, [-2.0] * 3, [2.0] * 3), 2.4, seed=5)
    n = 1000
    r = make(v, f, device)
    lt, ht = T(b1[0], device), T(b1[1], device)
    # the rows of the captured fill: preallocated for the largest total of the four steps, counts and offsets refreshed per step
    steps = ((v, b1), (v, b2), (v2, b2), (v2, b1))
    wants = [boxes_sim.brute(vv, f, *bb) for vv, bb in steps]
    rows = max(int(w.offsets[-1]) for w in wants) + 64
    count_in = torch.zeros(n, dtype=torch.int32, device=device)
    offsets_in = torch.zeros(n, dtype=torch.int64, device=device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the calls neither allocate nor synchronise
        any_ = hops.boxes_native(r.as_wrapper, lt, ht, "any")
        count = hops.boxes_native(r.as_wrapper, lt, ht, "count")
        face, inside = hops.boxes_fill_native(r.as_wrapper, lt, ht, count_in, offsets_in, rows, want_inside=True)
    for step, ((vv, bb), want) in enumerate(zip(steps, wants)):
        if step == 2:
            r.refit(T(vv, device))                      # moves the bounds
        lt.copy_(T(bb[0], device))
        ht.copy_(T(bb[1], device))
        count_in.copy_(T(want.count, device))
        offsets_in.copy_(T(want.offsets[:-1].copy(), device))
        graph.replay()
        torch.cuda.synchronize()
        total = int(want.offsets[-1])
        assert 0 < total <= rows - 64
        poison.assert_written(any_, count, face[:total], inside[:total], what=f"graph replay {step}")
        for name, t in (("face", face), ("inside", inside)):
            assert poison.stale_mask(t[total:]).all(), f"graph replay {step}: {name} rows beyond the total were written"
        got = boxes_sim.Result(host(any_), host(count), want.offsets, host(face[:total]), host(inside[:total]))
        BC.assert_same(got, want, f"graph replay {step}")


# ---- 11 -----------------------------------------------------------------------------------------------------------------
VOXEL_CASES = [("cube", 0.5, (-1.0, -1.0, -1.0)), ("cube", 0.3, None), ("cube", 0.75, (-1.1, -0.9, -1.3)),
               ("icosphere", 0.25, None), ("icosphere", 0.11, (-1.0, -1.0, -1.0))]


@pytest.mark.parametrize("name,pitch,origin", VOXEL_CASES, ids=[f"{n}-{p}-{'default' if o is None else o[0]}" for n, p, o in VOXEL_CASES])
def test_surface_voxels_match_the_cells_of_the_brute_force(device, name, pitch, origin):
    import boxes_sim
    v, f, _ = BC.CASES[name]()
    r = make(v, f, device)
    want = BC.voxel_cells(v, f, pitch, origin, lambda lo, hi: boxes_sim.brute(v, f, lo, hi).any)
    for chunk in (1 << 20, 1000):
        got = r.surface_voxels(pitch, origin=origin, chunk=chunk)
        assert got.dtype == torch.int64 and got.device.type == "cuda" and got.dim() == 2 and got.shape[1] == 3
        g = host(got)
        assert np.array_equal(g, want), f"{len(g)} cells, expected {len(want)}"
        assert len(g) > 20 and np.array_equal(g, np.unique(g, axis=0))          # lexicographic, no cell twice
    if name == "cube" and pitch == 0.5:
        # the cube's faces lie in cell planes: each occupies the cells on both sides of its plane -- the grid is 4^3 cells with a
        # shell of touching cells around it: every cell of the 6^3 block except the 2^3 strictly inside the cube
        block = np.stack(np.meshgrid(*[np.arange(-1, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
        inner = ((block >= 1) & (block <= 2)).all(1)
        assert np.array_equal(g, block[~inner])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            r.surface_voxels(bad)
