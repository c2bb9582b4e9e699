"""RaySceneIntersector.intersects_count / intersects_all / segments_count / segments_all (libtriro_scene_cross.so:
k_scene_cross<>, k_scene_cross_rows) against the host brute force.

The oracle of every comparison is tests/host_sim/scene_cross_sim.brute: cross_sim.brute -- the per-triangle predicate of
csrc/tr_range.h over every triangle -- per instance on the rays of scene_sim.transform, the rows ordered by numpy.lexsort on
(ray, t, instance, face), on the same float32 inputs; itself pinned to the scene's any / closest brute force, to the crossing
query at the identity and to integer arithmetic by tests/test_scene_cross_cpu.py.  Comparisons are bit for bit (count, offsets,
instance, face, t, front, loc, uv, ray).  Every native call of the bindings comes back through a wrapper that runs
poison.assert_written on its outputs (the autouse fixture `checked_native`); the row arrays of the direct calls (fill) carry
poisoned guard rows on both sides of the `total` rows, checked after every call; captured calls are checked after each
replay."""
import ctypes as C

import numpy as np
import pytest
import torch

import cross_cases as CC
import poison
import range_cases as RC
import scene_cases as SC
import scene_cross_cases as XC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("scene_cross_count_native", "scene_cross_fill_native")
CALLS = {name: 0 for name in NATIVES}
GUARD = 1024
ROWS = dict(instance=((), torch.int32), faces=((), torch.int32), t=((), torch.float32), front=((), torch.bool), loc=((3,), torch.float32),
            uv=((2,), torch.float32), ray=((), torch.int64), slot=((), torch.int32))
OPTIONAL = ("front", "loc", "uv", "ray")


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


def make_scene(meshes, mesh_of, M):
    from triro.ray import RaySceneIntersector
    return RaySceneIntersector(meshes, mesh_of, M)


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


@pytest.fixture(scope="module")
def member_handles(device):
    """one RayMeshIntersector per member of scene_cases.members(), built once"""
    return [make(v, f, device) for v, f in SC.members()]


def host(x):
    return None if x is None else x.cpu().numpy()


def bound(x, n, device):
    return None if x is None else T(np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (n,))), device)


def guarded_fill(scene, ot, dt, lt, ht, count, offsets, total, stack_entries=0, leave_out=(), ray_base=0, expect_full=True):
    """tr_scene_cross_fill itself into row arrays with GUARD poisoned rows on either side of the `total` rows; the optional
    outputs named in leave_out are passed as NULL (and d_slot with them when no row is to be evaluated).  After the call every
    guard row still holds its poison and (expect_full) every row inside was written.  -> {name: tensor of the total rows}"""
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
        hops._check(hops.get_scene_cross_module().tr_scene_cross_fill(
            scene._handle, C.byref(hops.make_rays(ot, dt)), None if lt is None else lt.data_ptr(), None if ht is None else ht.data_ptr(),
            count.data_ptr(), offsets.data_ptr(), total, ptr("instance"), ptr("faces"), ptr("t"), ptr("front"), ptr("loc"), ptr("uv"), ptr("ray"),
            ray_base, ptr("slot"), int(stack_entries), hops._stream_ptr(dev)))
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


def result(count, offsets, rows):
    import scene_cross_sim
    front = rows["front"]
    return scene_cross_sim.Result(host(count).reshape(-1), host(offsets), host(rows["instance"]), host(rows["faces"]), host(rows["t"]),
                                  None if front is None else host(front), host(rows["loc"]), host(rows["uv"]), host(rows["ray"]))


def native(scene, o, d, lo, hi, device, stack_entries=0, leave_out=(), ray_base=0):
    """the count entry through its binding, then the fill into guarded rows -> a scene_cross_sim.Result of numpy arrays"""
    import triro.backend.ops as hops
    n = len(o)
    ot, dt = T(np.ascontiguousarray(o, np.float32).reshape(-1, 3), device), T(np.ascontiguousarray(d, np.float32).reshape(-1, 3), device)
    lt, ht = bound(lo, n, device), bound(hi, n, device)
    count = hops.scene_cross_count_native(scene._handle, scene.device.index, ot, dt, lt, ht, stack_entries)
    assert count.dtype == torch.int32 and count.shape == (n,)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    offsets[1:] = torch.cumsum(count, 0)
    total = int(offsets[-1])
    rows = guarded_fill(scene, ot, dt, lt, ht, count, offsets[:n].contiguous(), total, stack_entries, leave_out, ray_base)
    return result(count, offsets, rows)


def check(scene, want, o, d, lo, hi, device, what, **kw):
    got = native(scene, o, d, lo, hi, device, **kw)
    XC.assert_same(got, want, what)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.scenes()))
def test_scenes_at_every_stack_limit(device, member_handles, name):
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    for kind in ("none", "hash", "exact"):
        lo, hi = XC.bounds_of(name, kind)
        want = XC.brute_of(name, kind)
        for entries in (1, 2, 0):
            got = check(scene, want, s["o"], s["d"], lo, hi, device, f"{name}, bounds {kind}, stack_entries {entries}", stack_entries=entries)
        if kind == "hash":      # hostile rays and bounds (`bad` is about the scene's own bounds): count 0 and no rows
            assert not got.count[s["bad"]].any() and not np.isin(got.ray, np.flatnonzero(s["bad"])).any() and not np.isnan(got.t).any()


def test_the_fixtures_are_what_the_comparisons_need():
    XC.check_fixture_conditions()


def test_the_binding_of_the_whole_query_is_the_count_the_scan_and_the_fill(device, member_handles):
    import scene_cross_sim
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    want = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], s["o"], s["d"], s["lo"], s["hi"], ray_base=11)
    before = dict(CALLS)
    res = hops.scene_cross_all_native(scene._handle, scene.device.index, T(s["o"], device), T(s["d"], device), T(s["lo"], device), T(s["hi"], device),
                                      True, True, True, True, 11)
    assert CALLS["scene_cross_count_native"] == before["scene_cross_count_native"] + 1
    assert CALLS["scene_cross_fill_native"] == before["scene_cross_fill_native"] + 1
    torch.cuda.synchronize()
    poison.assert_written(res[0], what="scene_cross_all_native offsets")
    assert [x.dtype for x in res] == [torch.int64, torch.int32, torch.int32, torch.float32, torch.bool, torch.float32, torch.float32, torch.int64]
    XC.assert_same(scene_cross_sim.Result(want.count, *(host(x) for x in res)), want, "scene_cross_all_native")


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129])
def test_tails_of_the_lane_and_block_indexing(device, member_handles, n):
    import scene_cross_sim
    s = SC.scenes()["three"]
    full = XC.brute_of("three", "hash")
    start = int(np.flatnonzero(XC.instances_per_ray(full) >= 2)[0])      # (begin where a ray crosses two instances)
    start = min(start, len(s["o"]) - 129)
    o, d, lo, hi = (x[start:start + n] for x in (s["o"], s["d"], s["lo"], s["hi"]))
    want = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], o, d, lo, hi)
    if n >= 63:
        assert len(want.t) > 5 and (want.count == 0).any()
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    got = check(scene, want, o, d, lo, hi, device, f"{n} rays")
    total = int(want.offsets[-1])
    assert got.count.shape == (n,) and got.offsets.shape == (n + 1,) and got.instance.shape == (total,) and got.faces.shape == (total,)
    assert got.t.shape == (total,) and got.front.shape == (total,) and got.loc.shape == (total, 3) and got.uv.shape == (total, 2) and got.ray.shape == (total,)
    # each optional output left out in turn, then all of them (no slot scratch either)
    for leave_out in [(k,) for k in OPTIONAL] + [OPTIONAL, ("front", "loc", "uv")]:
        g = check(scene, want, o, d, lo, hi, device, f"{n} rays, without {leave_out}", leave_out=leave_out)
        assert all(getattr(g, k) is None for k in leave_out) and all(getattr(g, k) is not None for k in OPTIONAL if k not in leave_out)
    # one bound alone, and none
    M = SC.members()
    check(scene, scene_cross_sim.brute(M, s["mesh_of"], s["M"], o, d, None, hi), o, d, None, hi, device, f"{n} rays, tmax alone")
    check(scene, scene_cross_sim.brute(M, s["mesh_of"], s["M"], o, d, lo, None), o, d, lo, None, device, f"{n} rays, tmin alone")
    check(scene, scene_cross_sim.brute(M, s["mesh_of"], s["M"], o, d, ray_base=1 << 40), o, d, None, None, device, f"{n} rays, default bounds",
          ray_base=1 << 40)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_strided_rays_with_a_broadcast_origin(device, member_handles):
    import scene_cross_sim
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    H, Wd = 37, 53
    n = H * Wd
    d = RC.icosphere()[3][:n]
    lo, hi = RC.hash_bounds(n, 91, 3.5)
    origin = np.array([0.2, -0.1, 0.3], np.float32)
    wide = torch.zeros((H, Wd, 5), dtype=torch.float32, device=device)
    wide[..., 1:4] = T(d.reshape(H, Wd, 3), device)
    dirs = wide[..., 1:4]
    origins = T(origin, device).expand(H, Wd, 3)
    assert not dirs.is_contiguous() and origins.stride() == (0, 0, 1)
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    want = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], np.tile(origin, (n, 1)), d, lo, hi)
    assert (want.count > 0).sum() > 100 and len(set(want.instance.tolist())) == 3

    def run(ot, dt, lt, ht, want, what):
        count = hops.scene_cross_count_native(scene._handle, scene.device.index, ot, dt, lt, ht)
        assert count.shape == ot.shape[:-1]
        offsets = T(want.offsets, device)
        rows = guarded_fill(scene, ot, dt, lt, ht, count.reshape(-1), offsets[:n].contiguous(), int(want.offsets[-1]))
        XC.assert_same(result(count, offsets, rows), want, what)
    run(origins, dirs, T(lo, device), T(hi, device), want, "[H, W, 3] view, broadcast origin")
    # rows of a transposed tensor: the general stride path for both
    ot = T(np.tile(origin, (n, 1)).reshape(H, Wd, 3), device).transpose(0, 1)
    dtr = T(d.reshape(H, Wd, 3), device).transpose(0, 1)
    tr = lambda x: np.ascontiguousarray(x.reshape(H, Wd, *x.shape[1:]).swapaxes(0, 1)).reshape(n, *x.shape[1:])      # noqa: E731
    want_t = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], np.tile(origin, (n, 1)), tr(d), tr(lo), tr(hi))
    run(ot, dtr, T(tr(lo), device), T(tr(hi), device), want_t, "transposed rays")


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_a_wave_whose_lanes_split_between_instances(device, member_handles):
    """three members in a row, 10 apart; even lanes start around the first with tmax below 4, odd lanes around the third: no ray
    can reach another instance than its own.  Then the instances listed in reverse order: the same rows after renumbering."""
    import scene_cross_sim
    rng = np.random.default_rng(3)
    M = np.array([SC.placement(SC.general(rng, 0.9), [-10, 0, 0]), SC.placement(np.eye(3), [0, 0, 0]), SC.placement(SC.general(rng, 0.9), [10, 0, 0])])
    mesh_of = np.array([SC.ICO, SC.SHELLS, SC.ICO], np.int32)
    n = 4096
    o, d = W.hash_rays(n, 17, [-1.2] * 3, [1.2] * 3)
    o[0::2, 0] -= 10
    o[1::2, 0] += 10
    lo, hi = RC.hash_bounds(n, 19, 4.0)
    want = scene_cross_sim.brute(SC.members(), mesh_of, M, o, d, lo, hi)
    ray = want.ray
    assert set(want.instance[ray % 2 == 0].tolist()) == {0} and set(want.instance[ray % 2 == 1].tolist()) == {2}
    assert (want.count[0::2] > 0).sum() > 100 and (want.count[1::2] > 0).sum() > 100 and (want.count == 0).sum() > 200 and want.count.max() >= 2
    for entries in (0, 1):
        check(make_scene(member_handles, mesh_of, M), want, o, d, lo, hi, device, f"split lanes, stack_entries {entries}", stack_entries=entries)
        got = native(make_scene(member_handles, mesh_of[::-1].copy(), M[::-1].copy()), o, d, lo, hi, device, stack_entries=entries)
        XC.assert_same(XC.renumbered(got, 3), want, f"split lanes, reversed listing renumbered, stack_entries {entries}")


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_long_interleaved_lists_in_one_wave(device):
    import scene_cross_sim
    q = XC.quad_scene()
    want = scene_cross_sim.brute(q["members"], q["mesh_of"], q["M"], q["o"], q["d"])
    XC.check_quad_scene(want, "quads, brute force")
    scene = make_scene([make(*q["members"][0], device)], q["mesh_of"], q["M"])
    for entries in (0, 1):
        got = check(scene, want, q["o"], q["d"], None, None, device, f"quads placed three times, stack_entries {entries}", stack_entries=entries)
        XC.check_quad_scene(got, f"quads on the GPU, stack_entries {entries}")


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_fill_with_counts_of_a_narrower_interval_stays_inside_its_rows(device, member_handles):
    """the caller's error: count / offsets computed for a narrower interval (and a total cut short) handed to a fill on the
    wider one.  Wrong rows are allowed; a write outside the rows of those counts is not: the guard rows stay poisoned, and
    what is written at a ray's rows are crossings of the wider interval of that ray, ordered, with their own outputs."""
    import scene_cross_sim
    name = "three"
    s = SC.scenes()[name]
    wide = XC.brute_of(name, "hash")
    with np.errstate(invalid="ignore"):      # (the hostile bounds: Inf - Inf)
        lo2, hi2 = CC.narrower(s["lo"], s["hi"])
    small = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], s["o"], s["d"], lo2, hi2)
    assert (wide.count >= small.count).all() and wide.offsets[-1] > 1.5 * small.offsets[-1] > 100
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    ot, dt, lt, ht = T(s["o"], device), T(s["d"], device), T(s["lo"], device), T(s["hi"], device)
    count, offsets = T(small.count, device), T(small.offsets[:-1].copy(), device)
    key = (wide.ray * 8 + wide.instance) * 4096 + wide.faces
    order = np.argsort(key)
    for total in (int(small.offsets[-1]), int(small.offsets[-1]) - 37):
        for entries in (0, 1):
            rows = guarded_fill(scene, ot, dt, lt, ht, count, offsets, total, entries)
            inst, face, t, ray = host(rows["instance"]), host(rows["faces"]), host(rows["t"]), host(rows["ray"])
            mine = np.repeat(np.arange(len(s["o"])), small.count)[:total]
            assert np.array_equal(ray, mine)
            mykey = (mine * 8 + inst) * 4096 + face
            at = np.minimum(np.searchsorted(key[order], mykey), len(key) - 1)
            assert np.array_equal(key[order][at], mykey), "a row is no crossing of its ray on the wider interval"
            at = order[at]
            for k, got in (("t", t), ("front", host(rows["front"])), ("loc", host(rows["loc"])), ("uv", host(rows["uv"]))):
                assert np.array_equal(RC.bits(got), RC.bits(getattr(wide, k)[at])), k
            same_ray = mine[1:] == mine[:-1]
            after = (t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & ((inst[1:] > inst[:-1]) | ((inst[1:] == inst[:-1]) & (face[1:] > face[:-1]))))
            assert after[same_ray].all()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "odd", "many65"])
def test_count_is_any_and_the_first_row_is_closest_on_the_same_handle(device, member_handles, name):
    import triro.backend.ops as hops
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    ot, dt, lt, ht = T(s["o"], device), T(s["d"], device), T(s["lo"], device), T(s["hi"], device)
    h, dev = scene._handle, scene.device.index
    for a, b in ((None, None), (lt, ht)):
        offsets, inst, face, t, front, loc, uv, _ = hops.scene_cross_all_native(h, dev, ot, dt, a, b, True, True, True)
        count = offsets[1:] - offsets[:-1]
        assert torch.equal(count > 0, hops.scene_any_native(h, dev, ot, dt, a, b))
        chit, cfront, cinst, ctri, ct, cloc, cuv = hops.scene_closest_native(h, dev, ot, dt, a, b)
        assert torch.equal(count > 0, chit) and int(chit.sum()) > 100
        first = offsets[:-1][chit]
        assert torch.equal(inst[first], cinst[chit]) and torch.equal(face[first], ctri[chit]) and torch.equal(front[first], cfront[chit])
        for mine, theirs in ((t, ct), (loc, cloc), (uv, cuv)):
            assert torch.equal(mine[first].view(torch.int32), theirs[chit].view(torch.int32))


@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI])
def test_one_instance_at_the_identity_is_the_crossing_query_of_the_member(device, member_handles, member):
    import triro.backend.ops as hops
    mk = (RC.icosphere, RC.shells5, RC.icosphere)[member]
    o, d, lo, hi = mk()[2:6]
    ho, hd, hlo, hhi, _ = RC.hostile_rays(o, d, lo, hi)
    o, d, lo, hi = (np.concatenate(x) for x in ((o[:6000], ho), (d[:6000], hd), (lo[:6000], hlo), (hi[:6000], hhi)))
    keep = ~(np.signbit(o) & (o == 0)).any(1) & ~(np.signbit(d) & (d == 0)).any(1)      # rays without a negative-zero component
    o, d, lo, hi = o[keep], d[keep], lo[keep], hi[keep]
    scene = make_scene(member_handles, [member], np.eye(3, 4, dtype=np.float32)[None])
    ot, dt, lt, ht = T(o, device), T(d, device), T(lo, device), T(hi, device)
    for a, b in ((None, None), (lt, ht)):
        mine = hops.scene_cross_all_native(scene._handle, scene.device.index, ot, dt, a, b, True, True, True, True, 3)
        theirs = hops.cross_all_native(member_handles[member].as_wrapper, ot, dt, a, b, True, True, True, True, 3)
        assert int(theirs[0][-1]) > (20 if member == SC.TRI else 500) and not mine[1].any()
        for x, y in zip(mine[:1] + mine[2:], theirs):
            assert x.shape == y.shape and torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int64 if x.element_size() == 8 else torch.int32),
                                                      y.view(torch.uint8) if y.dtype == torch.bool else y.view(torch.int64 if y.element_size() == 8 else torch.int32))


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_exact_transforms_against_the_integer_reference(device):
    import scene_cross_sim
    L = SC.lattice_scene()
    meshes = [make(v, f, device) for v, f in L["members"]]
    scene = make_scene(meshes, L["mesh_of"], L["M"])
    want = scene_cross_sim.brute(L["members"], L["mesh_of"], L["M"], L["o"], L["d"])
    for entries in (0, 1):
        got = check(scene, want, L["o"], L["d"], None, None, device, f"lattice scene, stack_entries {entries}", stack_entries=entries)
    full, pairs = XC.check_lattice(got, "lattice scene on the GPU")
    assert full > 7000 and pairs > 1000


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_set_transforms_refit_and_update_raw(device):
    import scene_cross_sim
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.2)).astype(np.float32)
    tv, tf = SC.members()[SC.TRI]
    a, b = make(v, f, device), make(tv, tf, device)
    mem = [(v, f), (tv, tf)]
    mesh_of = np.array([0, 1, 0], np.int32)
    rng = np.random.default_rng(11)
    M1 = np.array([SC.placement(np.eye(3), [-1.2, 0, 0]), SC.placement(np.eye(3) * 1.5, [0, 0.2, 0]), SC.placement(SC.general(rng), [1.2, 0.3, 0])])
    n = 3000
    o, d = W.hash_rays(n, 23, [-2.5, -1.5, -1.5], [2.5, 1.5, 1.5])
    lo, hi = RC.hash_bounds(n, 25, 4.0)
    brute = lambda mem, M: scene_cross_sim.brute(mem, mesh_of, M, o, d, lo, hi)      # noqa: E731
    scene = make_scene([a, b], mesh_of, M1)
    built = (a.generation, b.generation)
    first = brute(mem, M1)
    assert (XC.instances_per_ray(first) >= 2).sum() > 20
    check(scene, first, o, d, lo, hi, device, "built")
    # an object moves: twelve floats and a commit, no member is rebuilt
    M2 = M1.copy()
    M2[2] = SC.placement(SC.rotation([0, 0, 1], 0.8) @ M1[2][:, :3].astype(np.float64), [0.6, -0.4, 0.5])
    scene.set_transforms(M2)
    want = brute(mem, M2)
    assert not np.array_equal(want.count, first.count)
    check(scene, want, o, d, lo, hi, device, "after set_transforms")
    assert (a.generation, b.generation) == built and scene.info()["commits"] == 2
    # a refit keeps the member's arrays: the scene stays valid and shows the moved geometry
    a.refit(T(v2, device))
    mem[0] = (v2, f)
    want = brute(mem, M2)
    check(scene, want, o, d, lo, hi, device, "after a refit of a member, no commit")
    check(scene, want, o, d, lo, hi, device, "after a refit, one stack entry", stack_entries=1)
    assert scene.info()["commits"] == 2
    # update_raw to another triangle count moves them: stale until committed
    v3, f3 = W.icosphere(3)
    a.update_raw(T(v3, device), T(f3, device))
    ot, dt = T(o, device), T(d, device)
    for call in (lambda: scene.intersects_count(ot, dt), lambda: scene.intersects_all(ot, dt), lambda: scene.segments_count(ot, T(o + d, device)),
                 lambda: scene.segments_all(ot, T(o + d, device))):
        with pytest.raises(ValueError, match="scene is stale: commit it again"):
            call()
    scene.commit()
    mem[0] = (v3, f3)
    check(scene, brute(mem, M2), o, d, lo, hi, device, "update_raw of a member, then commit")


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_the_first_calls_on_a_fresh_scene_can_be_captured(device, member_handles):
    import scene_cross_sim
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    n = 1000
    o1, d1 = W.hash_rays(n, 29, [-1.5] * 3, [1.5] * 3)
    o2, d2 = W.hash_rays(n, 31, [-1.5] * 3, [1.5] * 3)
    b1, b2 = RC.hash_bounds(n, 33, 3.0), RC.hash_bounds(n, 35, 3.0)
    steps = ((o1, d1, b1), (o2, d2, b2))
    wants = [scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], o, d, lo, hi, ray_base=5) for o, d, (lo, hi) in steps]
    rows = max(int(w.offsets[-1]) for w in wants) + 64
    # the count, captured as the very first call on a fresh scene
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    h, dev = scene._handle, scene.device.index
    ot, dt, lt, ht = T(o1, device), T(d1, device), T(b1[0], device), T(b1[1], device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the call neither allocates nor synchronises
        count = hops.scene_cross_count_native(h, dev, ot, dt, lt, ht)
    # the fill with known counts, captured as the very first call on another fresh scene
    scene2 = make_scene(member_handles, s["mesh_of"], s["M"])
    count_in = torch.zeros(n, dtype=torch.int32, device=device)
    offsets_in = torch.zeros(n, dtype=torch.int64, device=device)
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=side):
        outs = hops.scene_cross_fill_native(scene2._handle, dev, ot, dt, lt, ht, count_in, offsets_in, rows, True, True, True, True, 5)
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
        poison.assert_written(count, *(x[:total] for x in outs), what=f"graph replay {step}")
        for name, x in zip(("instance", "face", "t", "front", "loc", "uv", "ray"), outs):
            assert poison.stale_mask(x[total:]).all(), f"graph replay {step}: {name} rows beyond the total were written"
        got = scene_cross_sim.Result(host(count), want.offsets, *(host(x[:total]) for x in outs))
        XC.assert_same(got, want, f"graph replay {step}")


# ---- 11 -----------------------------------------------------------------------------------------------------------------
def test_python_methods_shapes_bounds_segments_and_errors(device, member_handles):
    import scene_cross_sim
    from triro.ray import RaySceneIntersector
    s = SC.scenes()["three"]
    mem, mesh_of, M = SC.members(), s["mesh_of"], s["M"]
    o, d, lo, hi = s["o"], s["d"], s["lo"], s["hi"]
    scene = RaySceneIntersector(member_handles, mesh_of, M)
    brute = lambda *a, **kw: scene_cross_sim.brute(mem, mesh_of, M, *a, **kw)      # noqa: E731
    n = 35

    def as_result(count, out):
        """the tuple of intersects_all(front, loc, uv) -> a Result"""
        offsets, inst, tri, t, front, loc, uv = out
        assert [x.dtype for x in out] == [torch.int64, torch.int32, torch.int32, torch.float32, torch.bool, torch.float32, torch.float32]
        assert int(offsets[-1]) == len(inst) == len(tri) == len(t) == len(front) == len(loc) == len(uv) and loc.shape[1:] == (3,) and uv.shape[1:] == (2,)
        return scene_cross_sim.Result(host(count).reshape(-1), host(offsets), host(inst), host(tri), host(t), host(front), host(loc), host(uv), None)
    every = dict(return_front=True, return_locations=True, return_uv=True)
    # [3]: a single ray, scalar bounds
    i = int(np.flatnonzero(XC.brute_of("three", "none").count >= 2)[0])
    w1 = brute(o[i:i + 1], d[i:i + 1], 0.0, 50.0)
    assert w1.count[0] >= 2
    c = scene.intersects_count(T(o[i], device), T(d[i], device), 0.0, 50.0)
    assert c.shape == () and c.dtype == torch.int32
    XC.assert_same(as_result(c, scene.intersects_all(T(o[i], device), T(d[i], device), 0.0, 50.0, **every)), w1, "[3] with scalar bounds")
    # [5, 7, 3] with tensor bounds of the batch shape; the optional parts in the order front, loc, uv
    ot, dt = T(o[:n].reshape(5, 7, 3), device), T(d[:n].reshape(5, 7, 3), device)
    lt, ht = T(lo[:n].reshape(5, 7), device), T(hi[:n].reshape(5, 7), device)
    wn = brute(o[:n], d[:n], lo[:n], hi[:n])
    c = scene.intersects_count(ot, dt, lt, ht)
    assert c.shape == (5, 7)
    XC.assert_same(as_result(c, scene.intersects_all(ot, dt, lt, ht, **every)), wn, "[5, 7, 3]")
    plain = scene.intersects_all(ot, dt, lt, ht)
    assert len(plain) == 4 and np.array_equal(host(plain[1]), wn.instance) and np.array_equal(host(plain[2]), wn.faces)
    assert np.array_equal(RC.bits(host(plain[3])), RC.bits(wn.t))
    for kw, k, shape in ((dict(return_front=True), "front", ()), (dict(return_locations=True), "loc", (3,)), (dict(return_uv=True), "uv", (2,))):
        out = scene.intersects_all(ot, dt, lt, ht, **kw)
        assert len(out) == 5 and out[4].shape == (len(wn.faces),) + shape and np.array_equal(RC.bits(host(out[4])), RC.bits(getattr(wn, k)))
    out = scene.intersects_all(ot, dt, lt, ht, return_uv=True, return_front=True)
    assert len(out) == 6 and out[4].dtype == torch.bool and out[5].shape[1:] == (2,)
    # default bounds, one bound alone
    wd = brute(o[:n], d[:n])
    XC.assert_same(as_result(scene.intersects_count(ot, dt), scene.intersects_all(ot, dt, **every)), wd, "default bounds")
    wb = brute(o[:n], d[:n], None, 0.75)
    XC.assert_same(as_result(scene.intersects_count(ot, dt, tmax=0.75), scene.intersects_all(ot, dt, None, torch.tensor(0.75), **every)), wb, "tmax alone")
    # segments: the float32 difference and the range [0, 1]; t is the fraction along the segment
    m = 1500
    p0, p1 = o[:m], (o[:m] + d[:m] * hi[:m, None]).astype(np.float32)
    so, sd, slo, shi = RC.segment_rays(p0, p1)
    ws = brute(so, sd, slo, shi)
    assert (ws.count > 1).sum() > 50 and (ws.count == 0).sum() > 200
    sc = scene.segments_count(T(p0, device), T(p1, device))
    got = as_result(sc, scene.segments_all(T(p0, device), T(p1, device), **every))
    XC.assert_same(got, ws, "segments")
    assert ((got.t >= 0) & (got.t <= 1)).all() and len(scene.segments_all(T(p0, device), T(p1, device))) == 4
    sc = scene.segments_count(T(p0[:24].reshape(2, 3, 4, 3), device), T(p1[:24].reshape(2, 3, 4, 3), device))
    assert sc.shape == (2, 3, 4) and np.array_equal(host(sc).reshape(-1), ws.count[:24])
    # an empty batch; a scene without a mesh
    e = torch.zeros((0, 3), dtype=torch.float32, device=device)
    assert scene.intersects_count(e, e).shape == (0,) and scene.segments_count(e, e).shape == (0,)
    out = scene.intersects_all(e, e, **every)
    assert out[0].shape == (1,) and int(out[0][0]) == 0 and all(len(x) == 0 for x in out[1:]) and out[5].shape == (0, 3)
    nothing = RaySceneIntersector([], [], np.zeros((0, 3, 4), np.float32))
    assert not nothing.intersects_count(ot, dt).any() and int(nothing.intersects_all(ot, dt)[0][-1]) == 0
    # one count launch, one fill
    before = dict(CALLS)
    scene.intersects_all(ot, dt, lt, ht)
    assert CALLS["scene_cross_count_native"] == before["scene_cross_count_native"] + 1
    assert CALLS["scene_cross_fill_native"] == before["scene_cross_fill_native"] + 1
    # errors: CPU tensors, shapes, bounds that do not broadcast
    for call in (lambda: scene.intersects_count(torch.from_numpy(o[:4]), torch.from_numpy(d[:4])),
                 lambda: scene.intersects_all(torch.from_numpy(o[:4]), T(d[:4], device)),
                 lambda: scene.segments_count(torch.from_numpy(o[:4]), T(d[:4], device)),
                 lambda: scene.segments_all(T(o[:4], device), torch.from_numpy(d[:4])),
                 lambda: scene.intersects_count(T(o[:4, :2], device), T(d[:4, :2], device)),
                 lambda: scene.intersects_all(T(o[:4], device), T(d[:5], device)),
                 lambda: scene.segments_all(T(o[:4], device), T(o[:5], device)),
                 lambda: scene.intersects_count(ot, dt, tmin=T(lo[:6], device)),
                 lambda: scene.intersects_all(ot, dt, tmax=T(hi[:6], device))):
        with pytest.raises(ValueError):
            call()
