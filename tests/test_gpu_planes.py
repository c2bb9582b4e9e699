"""planes_any / planes_count / faces_on_planes / section_segments / section_multiplane (libtriro_planes.so: k_planes<>,
k_planes_rows, k_planes_segments) against the host brute force, bit for bit.

The oracle of every comparison is tests/host_sim/planes_sim.brute: the predicates and the segment of csrc/tr_planes.h over every
active triangle, on the same float32 inputs -- itself pinned to an integer restatement, to the closed-loop identity and to known
answers by tests/test_planes_cpu.py, and once more here on the GPU's own results.  Comparisons are element for element (any,
count, offsets, faces; segments as bits).  Every native call of this module comes back through a wrapper that runs
poison.assert_written on its outputs (the autouse fixture `checked_native`)."""
import subprocess

import numpy as np
import pytest
import torch

import planes_cases as PC
import poison
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("planes_native", "planes_fill_native")
CALLS = {name: 0 for name in NATIVES}


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every native call: counted, and all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    originals = {name: getattr(hops, name) for name in NATIVES}

    def wrap(name):
        original = originals[name]

        def call(*args, **kwargs):
            res = original(*args, **kwargs)
            CALLS[name] += 1
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


def native(r, origins, normals, device, cut=False, frontier_entries=0):
    """every entry once -> a planes_sim.Result of numpy arrays (segments with cut)"""
    import planes_sim
    import triro.backend.ops as hops
    o, nr = planes_sim.planes(origins, normals)
    ot, nt = T(o, device), T(nr, device)
    any_ = hops.planes_native(r.as_wrapper, ot, nt, "any", cut, frontier_entries)
    count = hops.planes_native(r.as_wrapper, ot, nt, "count", cut, frontier_entries)
    offsets, face, seg = hops.faces_on_planes_native(r.as_wrapper, ot, nt, cut, cut, frontier_entries)
    torch.cuda.synchronize()
    poison.assert_written(offsets, what="faces_on_planes_native offsets")
    assert any_.dtype == torch.bool and count.dtype == torch.int32 and offsets.dtype == torch.int64 and face.dtype == torch.int32
    assert seg is None or (seg.dtype == torch.float32 and tuple(seg.shape) == (face.shape[0], 2, 3))
    return planes_sim.Result(host(any_), host(count), host(offsets), host(face), host(seg))


@pytest.fixture(scope="module")
def cases():
    """{mesh: (v, f, origins, normals, {cut: brute force})} for 257 hashed planes per mesh, computed once"""
    import planes_sim
    out = {}
    for k, name in enumerate(PC.MESHES):
        v, f = PC.mesh(name)
        o, nr = PC.hashed_planes(v, max(PC.BATCHES), seed=10 * k)
        out[name] = (v, f, o, nr, {c: planes_sim.brute(v, f, o, nr, cut=c) for c in (False, True)})
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.MESHES))
def test_kernels_match_the_brute_force_at_every_frontier_capacity(device, cases, name):
    v, f, o, nr, want = cases[name]
    r = make(v, f, device)
    for cut in (False, True):
        for entries in PC.FRONTIERS:
            got = native(r, o, nr, device, cut=cut, frontier_entries=entries)
            PC.assert_same(got, want[cut], f"{name}, cut={cut}, frontier_entries {entries}")
    if name == "hostile":
        inactive = ~np.isfinite(v[f]).all(axis=(1, 2))
        assert inactive.sum() > 0 and not inactive[want[False].faces].any()


@pytest.mark.parametrize("name", ["icosphere1280", "cube16"])
def test_kernels_match_the_host_walk_on_the_gpu_builders_tree(device, cases, name):
    """the simulated wave on the very tree the kernels walk reports what the kernels cannot: a frontier of one or two entries
    overflowed for every plane that meets sixteen faces, the whole capacity for none -- and all of them return the same bits"""
    import planes_sim
    from sim import SimBVH
    v, f, o, nr, want = cases[name]
    assert len(f) >= 1280
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    busy = want[False].count >= 16
    assert busy.sum() >= 100
    for cut in (False, True):
        for entries in PC.FRONTIERS:
            walked, stats = planes_sim.walk(B, o, nr, cut=cut, frontier_entries=entries, want_stats=True)
            PC.assert_same(walked, want[cut], f"host walk on the GPU tree, {name}, cut={cut}, frontier_entries {entries}")
            PC.assert_same(native(r, o, nr, device, cut=cut, frontier_entries=entries), walked, f"GPU tree, {name}, cut={cut}, {entries}")
            if entries in (1, 2):
                assert (stats.overflows[busy] > 0).all() and (stats.sub_steps[busy] > 0).all()
            if entries == 0:
                assert not stats.overflows.any()


def test_frontiers_next_to_the_wave_width_overflow_and_agree(device):
    """63 and 64 entries overflow where a round pushes more than fits: planes through the middle of the 5 120-face icosphere hold
    a hundred nodes and more at once (the simulated wave on the GPU builder's tree reports the pushes that did not fit)"""
    import planes_sim
    import workloads as W
    from sim import SimBVH
    v, f = W.icosphere(4)
    r = make(v, f, device)
    B = SimBVH(arrays=r.as_wrapper.download())
    c = np.float32(0.5 * (v.min(0) + v.max(0)))
    mo, mn = np.tile(c, (3, 1)), np.float32([[1, 1, 1], [0, 0, 1], [1, 2, 3]])
    for cut in (False, True):
        want = planes_sim.brute(v, f, mo, mn, cut=cut)
        assert (want.count >= 96).all()
        for entries in (63, 64, 65):
            walked, stats = planes_sim.walk(B, mo, mn, cut=cut, frontier_entries=entries, want_stats=True)
            assert (stats.overflows > 0).all(), entries
            PC.assert_same(walked, want, f"planes through the middle, host walk, cut={cut}, frontier_entries {entries}")
            PC.assert_same(native(r, mo, mn, device, cut=cut, frontier_entries=entries), want, f"planes through the middle, cut={cut}, {entries}")


def test_a_plane_with_more_rows_than_the_ordering_tile(device):
    """6 000 rows of one plane: k_planes_rows orders them in place in global memory, the slots riding in the segments' first word,
    where the planes of the other tests are ordered in the LDS tile"""
    import planes_sim
    v, f = PC.comb()
    o, nr = PC.COMB_PLANES
    r = make(v, f, device)
    for cut in (False, True):
        want = planes_sim.brute(v, f, o, nr, cut=cut)
        assert want.count[0] == len(f) == 6000 and want.count[1] > 4096 and want.count[2] > 0
        assert want.count[3:].tolist() == ([1200, 0] if cut else [6000, 6000])      # edges in the plane; faces that hang from it
        for entries in (0, 1, 64):
            PC.assert_same(native(r, o, nr, device, cut=cut, frontier_entries=entries), want, f"comb, cut={cut}, frontier_entries {entries}")


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_batch_sizes_and_one_large_batch(device, cases):
    import planes_sim
    v, f, o, nr, want = cases["icosphere80"]
    r = make(v, f, device)
    for n in (0,) + PC.BATCHES:
        for cut in (False, True):
            got = native(r, o[:n], nr[:n], device, cut=cut)
            assert got.any.shape == (n,) and got.count.shape == (n,) and got.offsets.shape == (n + 1,)
            PC.assert_same(got, planes_sim.brute(v, f, o[:n], nr[:n], cut=cut), f"{n} planes, cut={cut}")
    # the index math of a launch with many workgroups: one wave, one workgroup of the ordering and many rows per plane
    n = 100003
    bo, bn = PC.hashed_planes(v, n, seed=77)
    big = planes_sim.brute(v, f, bo, bn, cut=True)
    assert big.offsets[-1] > 500000 and (big.count == 0).sum() > 1000
    PC.assert_same(native(r, bo, bn, device, cut=True), big, f"{n} planes")
    PC.loops_close(big, f"{n} planes")


def test_hostile_planes_yield_empty_rows(device):
    import planes_sim
    v, f = PC.mesh("icosphere1280")
    r = make(v, f, device)
    o0, n0 = PC.hashed_planes(v, 200, seed=5)
    o, nr, valid, empty = PC.hostile_planes(o0, n0)
    nr[64:128] = 0.0                                      # a run of zero normals ...
    o[130:140, 1] = np.nan                                # ... and of NaN origins
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(o).all(1) & np.isfinite(nr).all(1) & (nr != 0).any(1)
    empty |= ~valid
    assert (~valid).sum() == 20 + 64 + 10
    for cut in (False, True):
        want = planes_sim.brute(v, f, o, nr, cut=cut)
        for entries in (0, 1):
            got = native(r, o, nr, device, cut=cut, frontier_entries=entries)
            PC.assert_same(got, want, f"hostile planes, cut={cut}, frontier_entries {entries}")
        assert not got.any[empty].any() and not got.count[empty].any()
        assert (got.count[29:33] > 0).all() and got.any[valid].sum() >= 50
        if cut:
            assert np.isfinite(got.segments).all()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_snapped_inputs_equal_the_exact_reference(device):
    """inputs on the grid k * 2^-10, |k| <= 2^12, integer normals (asserted by planes_cases.snapped / exact_tables), where s is
    exact: the kernels must EQUAL the integer restatement -- planes through vertices, along edges and coplanar with faces"""
    v, f = PC.mesh("cube4")
    o, nr = PC.lattice_planes()
    r = make(v, f, device)
    stats = PC.check_exact(lambda o_, n_, c: native(r, o_, n_, device, cut=c, frontier_entries=2), v, f, o, nr, "GPU, cube4")
    print("(pairs, met, cut, met with a vertex in the plane):", stats)
    assert 0 < stats[2] < stats[1] < stats[0] and stats[3] > 10000
    iv, i_f = PC.mesh("icosphere80")
    iv = PC.snap(iv)
    io, inr = PC.vertex_planes(iv)
    ri = make(iv, i_f, device)
    PC.check_exact(lambda o_, n_, c: native(ri, o_, n_, device, cut=c), iv, i_f, io, inr, "GPU, snapped icosphere")


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere80", "icosphere320", "icosphere1280", "cube4", "cube16"])
def test_segments_of_a_closed_mesh_pair_up_end_for_end(device, name):
    """needs no reference: for every plane the multiset of p0 (three float32 as bits) EQUALS the multiset of p1"""
    import planes_sim
    v, f = PC.mesh(name)
    r = make(v, f, device)
    rows = 0
    for label, (o, nr) in (("200 hashed planes", PC.hashed_planes(v, 200, seed=17)), ("vertex planes", PC.vertex_planes(v)),
                           ("lattice planes", PC.lattice_planes())):
        got = native(r, o, nr, device, cut=True, frontier_entries=0 if label != "vertex planes" else 3)
        assert np.isfinite(got.segments).all()
        rows += PC.loops_close(got, f"{name}, {label}")
        PC.assert_same(got, planes_sim.brute(v, f, o, nr, cut=True), f"{name}, {label}")
    assert rows > 1000


def test_known_answers_on_the_four_cell_cube(device):
    v, f = PC.mesh("cube4")
    r = make(v, f, device)
    for entries in (0, 1):
        PC.check_known(lambda o, nr, c: native(r, o, nr, device, cut=c, frontier_entries=entries), f"GPU, frontier_entries {entries}")


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_the_ordering_network_alone(device):
    """k_planes_rows on keys of the test's own: segments of 0 .. 4097 keys (in LDS up to 4096, in place beyond) with duplicates,
    both ends of the int32 range and sorted runs equal numpy.sort, and the words just outside each segment keep their poison"""
    import planes_sim
    import triro.backend.ops as hops
    lib = hops.get_planes_module()
    parts, count, offsets, size = PC.order_case()
    keys = poison.poisoned((size,), torch.int32, device)
    inside = np.zeros(size, bool)
    want = np.full(size, poison.INT32, np.int32)
    for p, off in zip(parts, offsets):
        keys[off:off + len(p)] = T(p, device)
        want[off:off + len(p)] = np.sort(p)
        inside[off:off + len(p)] = True
    before = host(keys)
    ct, ot = T(count, device), T(offsets, device)
    index = torch.device(device).index or 0
    with torch.cuda.device(device):
        rc = lib.tr_planes_order(index, len(count), ct.data_ptr(), ot.data_ptr(), size, keys.data_ptr(), hops._stream_ptr(device))
    assert rc == 0, hops.get_module().tr_last_error()
    torch.cuda.synchronize()
    got = host(keys)
    assert np.array_equal(got, want)
    assert (got[~inside] == poison.INT32).all() and (~inside).sum() >= 5 * len(parts)
    assert np.array_equal(planes_sim.order(before, count, offsets), want)
    # a total that cuts the last segment short
    keys2 = T(before, device)
    total = int(offsets[-1]) + 1
    with torch.cuda.device(device):
        rc = lib.tr_planes_order(index, len(count), ct.data_ptr(), ot.data_ptr(), total, keys2.data_ptr(), hops._stream_ptr(device))
    assert rc == 0
    torch.cuda.synchronize()
    got2 = host(keys2)
    assert np.array_equal(got2[total:], before[total:]) and np.array_equal(got2[:offsets[-1]], want[:offsets[-1]])


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_misdirected_fills_stay_inside_their_rows(device):
    """the caller's error: counts that are too small, too large or negative, offsets outside, a total cut short.  Wrong rows are
    allowed; a write outside [0, total) is not: guard rows on both sides stay poisoned.  Correct counts give the exact list."""
    import planes_sim
    import triro.backend.ops as hops
    v, f = PC.mesh("icosphere1280")
    r = make(v, f, device)
    o, nr = PC.hashed_planes(v, 300, seed=31)
    want = planes_sim.brute(v, f, o, nr, cut=True)
    total = int(want.offsets[-1])
    n = len(o)
    assert total > 5000 and want.count.max() > 64
    lib = hops.get_planes_module()
    ot, nt = T(o, device), T(nr, device)
    G = 4096

    def run(count, offsets, tot, entries, with_segments=True):
        ct, ft = T(np.ascontiguousarray(count, np.int32), device), T(np.ascontiguousarray(offsets, np.int64), device)
        face = poison.poisoned((G + total + G,), torch.int32, device)
        seg = poison.poisoned((G + total + G, 2, 3), torch.float32, device)
        with torch.cuda.device(device):
            rc = lib.tr_planes_fill(r.as_wrapper._inner, ot.data_ptr(), nt.data_ptr(), n, ct.data_ptr(), ft.data_ptr(), tot,
                                    face.data_ptr() + 4 * G, seg.data_ptr() + 24 * G if with_segments else None, 1, entries,
                                    hops._stream_ptr(device))
        assert rc == 0, hops.get_module().tr_last_error()
        torch.cuda.synchronize()
        for name, t in (("face", face), ("segments", seg)):
            stale = poison.stale_mask(t)
            assert stale[:G].all() and stale[G + tot:].all(), f"{name}: a guard row was written (total {tot}, frontier_entries {entries})"
        if not with_segments:
            assert poison.stale_mask(seg).all()
        return host(face)[G:G + tot], host(seg)[G:G + tot]
    for entries in (0, 1):
        face, seg = run(want.count, want.offsets[:-1], total, entries)
        assert np.array_equal(face, want.faces) and np.array_equal(PC.bits(seg), PC.bits(want.segments))
        face, _ = run(want.count, want.offsets[:-1], total, entries, with_segments=False)
        assert np.array_equal(face, want.faces)
        small = np.maximum(want.count - 3, 0).astype(np.int32)
        face, seg = run(small, want.offsets[:-1], total, entries)
        for i in (0, 1, 2, n // 2, n - 1):
            a = int(want.offsets[i])
            mine = want.faces[want.offsets[i]:want.offsets[i + 1]]
            assert (np.diff(face[a:a + small[i]]) > 0).all() and np.isin(face[a:a + small[i]], mine).all()
            at = want.offsets[i] + np.searchsorted(mine, face[a:a + small[i]])
            assert np.array_equal(PC.bits(seg[a:a + small[i]]), PC.bits(want.segments[at]))      # a row is a function of (plane, face)
        run(want.count + 5, want.offsets[:-1], total, entries)                      # too large
        run(-want.count - 1, want.offsets[:-1], total, entries)                     # negative
        run(want.count, want.offsets[:-1] + total - 7, total, entries)              # offsets outside
        run(want.count, want.offsets[:-1] - 11, total, entries)                     # negative offsets
        run(want.count, want.offsets[:-1], total - 37, entries)                     # total cut short
    # with total == 0 nothing is launched and nothing is written
    run(want.count, want.offsets[:-1], 0, 0)


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_python_methods_batch_shapes_multiplane_and_a_second_stream(device, cases):
    import planes_sim
    v, f, o, nr, want = cases["icosphere1280"]
    r = make(v, f, device)
    a, c = r.planes_any(T(o[0], device), T(nr[0], device)), r.planes_count(T(o[0], device), T(nr[0], device))
    assert a.shape == () and a.dtype == torch.bool and c.shape == () and c.dtype == torch.int32
    assert bool(a) == bool(want[False].any[0]) and int(c) == int(want[False].count[0])
    assert int(r.planes_count(T(o[0], device), T(nr[0], device), cut=True)) == int(want[True].count[0])

    def flat(o_, n_, shape, cut):
        a, c = r.planes_any(o_, n_), r.planes_count(o_, n_, cut=cut)
        off, tri = r.faces_on_planes(o_, n_, cut=cut)
        assert tuple(a.shape) == shape and tuple(c.shape) == shape and a.dtype == torch.bool and c.dtype == torch.int32
        assert off.dtype == torch.int64 and tri.dtype == torch.int32
        return planes_sim.Result(None, host(c).reshape(-1), host(off), host(tri), None), host(a).reshape(-1)
    for cut in (False, True):
        res, any_ = flat(T(o[:35].reshape(5, 7, 3), device), T(nr[:35].reshape(5, 7, 3), device), (5, 7), cut)
        PC.assert_same(res, planes_sim.brute(v, f, o[:35], nr[:35], cut=cut), f"[5, 7, 3], cut={cut}")
        assert np.array_equal(any_, want[False].any[:35])
    # one normal for many origins, one origin for many normals, numpy and float64 inputs, non-contiguous slices
    up = np.float32([0.0, 0.25, 1.0])
    res, _ = flat(T(o[:35].reshape(5, 7, 3), device), T(up, device), (5, 7), True)
    PC.assert_same(res, planes_sim.brute(v, f, o[:35], np.tile(up, (35, 1)), cut=True), "normals [3] against origins [5, 7, 3]")
    res, _ = flat(T(o[3], device), T(nr[:9], device), (9,), False)
    PC.assert_same(res, planes_sim.brute(v, f, np.tile(o[3], (9, 1)), nr[:9]), "origins [3] against normals [9, 3]")
    res, _ = flat(o[:50].astype(np.float64), T(nr[:50], device), (50,), True)
    PC.assert_same(res, planes_sim.brute(v, f, o[:50], nr[:50], cut=True), "numpy float64 origins, GPU normals")
    wide = torch.zeros((200, 8), dtype=torch.float32, device=device)
    wide[:, 1:4] = T(o[:200], device)
    wide[:, 4:7] = T(nr[:200], device)
    res, _ = flat(wide[::2, 1:4], wide[::2, 4:7], (100,), True)
    PC.assert_same(res, planes_sim.brute(v, f, o[:200:2], nr[:200:2], cut=True), "non-contiguous slices")
    # empty batches
    e = torch.zeros((0, 3), dtype=torch.float32, device=device)
    assert r.planes_any(e, e).shape == (0,) and r.planes_count(e, e).shape == (0,)
    off, tri, seg = r.section_segments(e, e)
    assert host(off).tolist() == [0] and tri.shape == (0,) and tuple(seg.shape) == (0, 2, 3)
    # section_segments: the cut faces, their segments, and faces_on_planes(cut=True) has the same tri_idx; one count launch, one fill
    before = dict(CALLS)
    off, tri, seg = r.section_segments(T(o, device), T(nr, device))
    assert CALLS["planes_native"] == before["planes_native"] + 1 and CALLS["planes_fill_native"] == before["planes_fill_native"] + 1
    PC.assert_same(planes_sim.Result(None, None, host(off), host(tri), host(seg)), want[True], "section_segments")
    off2, tri2 = r.faces_on_planes(T(o, device), T(nr, device), cut=True)
    assert torch.equal(off, off2) and torch.equal(tri, tri2)
    # section_multiplane: plane k at float32(origin + heights[k] * normal), evaluated in float64
    origin, normal = np.float64([0.01, -0.02, 0.03]), np.float64([0.3, -0.2, 1.1])
    heights = np.linspace(-1.2, 1.2, 41)
    mo = np.float32(origin[None, :] + heights[:, None] * normal[None, :])
    off, tri, seg = r.section_multiplane(origin, normal, heights)
    PC.assert_same(planes_sim.Result(None, None, host(off), host(tri), host(seg)),
                   planes_sim.brute(v, f, mo, np.tile(np.float32(normal), (41, 1)), cut=True), "section_multiplane")
    assert int(off[-1]) > 1000 and (np.diff(host(off)) == 0).sum() >= 2
    off32, tri32, _ = r.section_multiplane(T(np.float32(origin), device), T(np.float32(normal), device), T(np.float32(heights), device))
    mo32 = np.float32(np.float32(origin).astype(np.float64)[None, :] + np.float32(heights).astype(np.float64)[:, None] * np.float32(normal).astype(np.float64)[None, :])
    assert np.array_equal(host(tri32), planes_sim.brute(v, f, mo32, np.tile(np.float32(normal), (41, 1)), cut=True).faces)
    # a second stream
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        off, tri, seg = r.section_segments(T(o, device), T(nr, device))
    side.synchronize()
    PC.assert_same(planes_sim.Result(None, None, host(off), host(tri), host(seg)), want[True], "section_segments on a second stream")
    # refusals
    calls = [lambda: r.planes_any(torch.from_numpy(o[:4]), T(nr[:4], device)), lambda: r.planes_count(T(o[:4], device), torch.from_numpy(nr[:4])),
             lambda: r.faces_on_planes(T(o[:4, :2], device), T(nr[:4], device)), lambda: r.section_segments(T(o[:4], device), T(nr[:3], device)),
             lambda: r.section_multiplane(origin[:2], normal, heights), lambda: r.section_multiplane(origin, normal, heights.reshape(1, -1))]
    for call in calls:
        with pytest.raises(ValueError):
            call()


def test_lifecycle_refit_and_update(device):
    import planes_sim
    import workloads as W
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)
    o, nr = PC.hashed_planes(v2, 150, seed=3)
    r = make(v, f, device)
    PC.assert_same(native(r, o, nr, device, cut=True), planes_sim.brute(v, f, o, nr, cut=True), "built")
    r.refit(T(v2, device))
    PC.assert_same(native(r, o, nr, device, cut=True, frontier_entries=1), planes_sim.brute(v2, f, o, nr, cut=True), "after a refit")
    v3, f3 = PC.mesh("cube16")
    r.update_raw(T(v3, device), T(f3, device))
    PC.assert_same(native(r, o, nr, device, cut=False), planes_sim.brute(v3, f3, o, nr, cut=False), "update_raw to another mesh")


def test_the_c_client_runs_every_entry(device):
    from test_planes_cpu import build_planes_client
    p = subprocess.run([build_planes_client()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PLANES C CLIENT OK" in p.stdout
