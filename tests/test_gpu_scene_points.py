"""RaySceneIntersector.contains_points / contains_count / containing_instances (libtriro_scene_points.so: k_scene_points<>)
against the host brute force.

The oracle of every comparison is tests/host_sim/scene_points_sim.brute: the counts of cross_sim.brute -- the per-triangle
predicate of csrc/tr_range.h over every triangle -- per instance on the rays of scene_sim.transform for +d and -d, then the
parity in numpy, on the same float32 inputs; itself pinned to the scene's crossing rows, to the crossing counts at the identity
and to integer parity by tests/test_scene_points_cpu.py.  Comparisons are bit for bit (any, count, offsets, instance).  Every
native call of the bindings comes back through a wrapper that runs poison.assert_written on its outputs (the autouse fixture
`checked_native`); the list of the direct calls (fill) carries poisoned guard rows on both sides of the `total` rows, checked
after every call; captured calls are checked after each replay."""
import numpy as np
import pytest
import torch

import nearest_cases as NC
import poison
import scene_cases as SC
import scene_points_cases as PC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("scene_points_any_native", "scene_points_count_native", "scene_points_fill_native")
CALLS = {name: 0 for name in NATIVES}
GUARD = 1024


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
                poison.assert_written(res, what=name)
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


def guarded_fill(scene, pt, dt, count, offsets, total, stack_entries=0, expect_full=True):
    """tr_scene_points_fill itself into a list with GUARD poisoned rows on either side of the `total` rows.  After the call
    every guard row still holds its poison and (expect_full) every row inside was written.  -> the tensor of the total rows"""
    import triro.backend.ops as hops
    dev = pt.device
    buf = poison.poisoned((GUARD + total + GUARD,), torch.int32, dev)
    with torch.cuda.device(dev):
        hops._check(hops.get_scene_points_module().tr_scene_points_fill(
            scene._handle, pt.data_ptr(), pt.shape[0], dt.data_ptr(), count.data_ptr(), offsets.data_ptr(), total, buf[GUARD:].data_ptr(),
            int(stack_entries), hops._stream_ptr(dev)))
    torch.cuda.synchronize()
    stale = poison.stale_mask(buf)
    assert stale[:GUARD].all() and stale[GUARD + total:].all(), f"a guard row was written (total {total}, stack_entries {stack_entries})"
    if expect_full:
        assert not stale[GUARD:GUARD + total].any(), "a row inside was not written"
    return buf[GUARD:GUARD + total]


def native(scene, p, d, device, stack_entries=0):
    """the any and the count entry through their bindings, then the fill into guarded rows -> a scene_points_sim.Result"""
    import scene_points_sim
    import triro.backend.ops as hops
    pt, dt = T(np.ascontiguousarray(p, np.float32).reshape(-1, 3), device), T(np.ascontiguousarray(d, np.float32).reshape(3), device)
    n = len(pt)
    h, dev = scene._handle, scene.device.index
    any_ = hops.scene_points_any_native(h, dev, pt, dt, stack_entries)
    count = hops.scene_points_count_native(h, dev, pt, dt, stack_entries)
    assert any_.dtype == torch.bool and any_.shape == (n,) and count.dtype == torch.int32 and count.shape == (n,)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    offsets[1:] = torch.cumsum(count, 0)
    total = int(offsets[-1])
    inst = guarded_fill(scene, pt, dt, count, offsets[:n].contiguous(), total, stack_entries)
    return scene_points_sim.Result(host(any_), host(count), host(offsets), host(inst))


def check(scene, want, p, d, device, what, **kw):
    got = native(scene, p, d, device, **kw)
    PC.assert_same(got, want, what)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.scenes()))
def test_scenes_at_every_stack_limit(device, member_handles, name):
    """every scene, the `none` scene among them: the three kernels against the brute force at stack limits 1, 2 and all"""
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    p = PC.points_of(name)
    want = PC.brute_of(name)
    for entries in (1, 2, 0):
        got = check(scene, want, p, PC.DEFAULT, device, f"{name}, stack_entries {entries}", stack_entries=entries)
    bad = ~PC.valid_points(p)
    assert bad.sum() >= 50 and not got.any[bad].any() and not got.count[bad].any()
    check(scene, PC.brute_of(name, "other"), p, PC.OTHER, device, f"{name}, another direction")
    # the same instances listed in reverse: the same rows after renumbering
    r = SC.reversed_scene(s)
    got = native(make_scene(member_handles, r["mesh_of"], r["M"]), p, PC.DEFAULT, device, stack_entries=1)
    PC.assert_same(PC.renumbered(got, len(s["mesh_of"])), want, f"{name}, reversed listing renumbered")
    # a direction that is not finite: every point is inside nothing, and every output is still written
    for d in ([np.nan, 0, 1], [0, np.inf, 1]):
        got = native(scene, p[:300], np.float32(d), device)
        assert not got.any.any() and not got.count.any() and len(got.instance) == 0


def test_the_fixtures_are_what_the_comparisons_need():
    PC.check_fixture_conditions()


def test_the_binding_of_the_list_is_the_count_the_scan_and_the_fill(device, member_handles):
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    want = PC.brute_of("three")
    before = dict(CALLS)
    offsets, inst = hops.scene_points_list_native(scene._handle, scene.device.index, T(PC.points_of("three"), device), T(PC.DEFAULT, device))
    assert CALLS["scene_points_count_native"] == before["scene_points_count_native"] + 1
    assert CALLS["scene_points_fill_native"] == before["scene_points_fill_native"] + 1 and CALLS["scene_points_any_native"] == before["scene_points_any_native"]
    torch.cuda.synchronize()
    poison.assert_written(offsets, inst, what="scene_points_list_native")
    assert offsets.dtype == torch.int64 and inst.dtype == torch.int32
    assert np.array_equal(host(offsets), want.offsets) and np.array_equal(host(inst), want.instance)


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, member_handles, n):
    import scene_points_sim
    s = SC.scenes()["three"]
    full = PC.brute_of("three")
    base = PC.points_of("three")
    start = int(np.flatnonzero(full.count >= 2)[0])      # (begin where a point is inside two instances)
    start = min(start, len(base) - 129)
    p = base[start:start + n] if n <= 129 else np.concatenate([base, base[::-1]])[:n]
    assert len(p) == n
    want = scene_points_sim.brute(SC.members(), s["mesh_of"], s["M"], p, PC.DEFAULT)
    if n >= 63:
        assert len(want.instance) > 5 and (want.count == 0).any() and (want.count >= 2).any()
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    got = check(scene, want, p, PC.DEFAULT, device, f"{n} points")
    assert got.any.shape == (n,) and got.count.shape == (n,) and got.offsets.shape == (n + 1,) and got.instance.shape == (int(want.offsets[-1]),)
    check(scene, want, p, PC.DEFAULT, device, f"{n} points, one stack entry", stack_entries=1)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_waves_inside_different_instances_and_inside_nothing(device, member_handles):
    """scene_points_cases.split_waves(): a wave whose lanes are inside different instances (the ANY early exit finishes them
    at different instances), a wave in which no lane's ray crosses anything and one in which every first count is even
    and some are not zero (the second pass is skipped by the whole wave), a wave inside the middle instance alone, then hashed
    points around all three; and the reversed listing"""
    mesh_of, M, p, want = PC.split_waves()
    for entries in (0, 1):
        check(make_scene(member_handles, mesh_of, M), want, p, PC.DEFAULT, device, f"split lanes, stack_entries {entries}", stack_entries=entries)
        rev = native(make_scene(member_handles, mesh_of[::-1].copy(), M[::-1].copy()), p, PC.DEFAULT, device, stack_entries=entries)
        PC.assert_same(PC.renumbered(rev, 3), want, f"split lanes, reversed listing renumbered, stack_entries {entries}")


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_whole_waves_and_whole_blocks_of_invalid_points(device, member_handles):
    import scene_points_sim
    s = SC.scenes()["three"]
    base = PC.points_of("three")[:1024].copy()
    p = base.copy()
    p[64:128] = PC.hostile_points(base[64:128])            # a whole wave
    p[256:512] = PC.hostile_points(base[256:512])          # two whole blocks
    p[700:703] = PC.hostile_points(base[700:703])          # single lanes
    p[896:1024] = np.float32(np.nan)                       # the last block: every component of every point
    want = scene_points_sim.brute(SC.members(), s["mesh_of"], s["M"], p, PC.DEFAULT)
    bad = ~PC.valid_points(p)
    assert bad[64:128].all() and bad[256:512].all() and bad[896:].all() and not want.count[bad].any() and (want.count[~bad] > 0).sum() > 100
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    for entries in (0, 1):
        check(scene, want, p, PC.DEFAULT, device, f"invalid waves and blocks, stack_entries {entries}", stack_entries=entries)
    allbad = PC.hostile_points(base[:300])
    got = native(scene, allbad, PC.DEFAULT, device)
    assert not got.any.any() and not got.count.any() and len(got.instance) == 0


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_exact_transforms_against_integer_parity(device):
    import scene_points_sim
    L = SC.lattice_scene()
    P = PC.lattice_points()
    meshes = [make(v, f, device) for v, f in L["members"]]
    scene = make_scene(meshes, L["mesh_of"], L["M"])
    got = {}
    for j, d in enumerate(PC.LATTICE_DIRECTIONS):
        want = scene_points_sim.brute(L["members"], L["mesh_of"], L["M"], P["p"], d)
        for entries in (0, 1):
            got[j] = check(scene, want, P["p"], d, device, f"lattice scene, direction {d}, stack_entries {entries}", stack_entries=entries)
    PC.check_lattice(lambda j: got[j], "lattice scene on the GPU")


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_fill_with_counts_of_another_direction_stays_inside_its_rows(device, member_handles):
    """the caller's error: count / offsets computed for another direction (and a total cut short) handed to a fill.  Wrong
    rows are allowed; a write outside the rows of those counts is not: the guard rows stay poisoned, what is written at a
    point's rows are the first instances that hold it, ascending, and rows it has no instance for stay untouched."""
    q = PC.open_scene()      # (open members: on closed ones the counts of two directions are the same)
    mine, theirs, p = q["mine"], q["theirs"], q["p"]
    scene = make_scene([make(v, f, device) for v, f in q["members"]], q["mesh_of"], q["M"])
    check(scene, mine, p, PC.DEFAULT, device, "open scene")
    check(scene, theirs, p, PC.OTHER, device, "open scene, the other direction", stack_entries=1)
    pt, dt = T(p, device), T(PC.DEFAULT, device)
    count, offsets = T(theirs.count, device), T(theirs.offsets[:-1].copy(), device)
    for total in (int(theirs.offsets[-1]), int(theirs.offsets[-1]) - 37):
        for entries in (0, 1):
            buf = guarded_fill(scene, pt, dt, count, offsets, total, entries, expect_full=False)
            PC.check_misdirected_rows(host(buf), mine, theirs, total, ~host(poison.stale_mask(buf)), f"total {total}, stack_entries {entries}")
    # a negative count, an offset beyond the list and one below it: those points write nothing, the others what they did
    c2, o2 = theirs.count.copy(), theirs.offsets[:-1].copy()
    held = np.flatnonzero((mine.count > 0) & (theirs.count > 0))[:3]
    c2[held[0]], o2[held[1]], o2[held[2]] = -5, int(theirs.offsets[-1]) + 10, -3
    total = int(theirs.offsets[-1])
    buf = guarded_fill(scene, pt, dt, T(c2, device), T(o2, device), total, 0, expect_full=False)
    stale = host(poison.stale_mask(buf))
    for i in held:
        assert stale[int(theirs.offsets[i]):int(theirs.offsets[i + 1])].all(), f"point {i} wrote rows it was not given"


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "odd", "many65"])
def test_the_list_is_the_odd_odd_instances_of_the_crossing_rows_on_the_same_handle(device, member_handles, name):
    import triro.backend.ops as hops
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    p = PC.points_of(name)
    n, ninst = len(p), len(s["mesh_of"])
    pt, dt = T(p, device), T(PC.DEFAULT, device)
    h, dev = scene._handle, scene.device.index
    offsets, inst = hops.scene_points_list_native(h, dev, pt, dt)
    count = hops.scene_points_count_native(h, dev, pt, dt)
    assert torch.equal(hops.scene_points_any_native(h, dev, pt, dt), count > 0) and torch.equal(offsets[1:] - offsets[:-1], count.long())
    odd = []
    for sign in (1.0, -1.0):
        dirs = (sign * dt).expand(n, 3).contiguous()
        xo, xi = hops.scene_cross_all_native(h, dev, pt, dirs)[:2]
        per = torch.zeros((n, ninst), dtype=torch.int64, device=device)
        ray = torch.repeat_interleave(torch.arange(n, device=device), xo[1:] - xo[:-1])
        per.index_put_((ray, xi.long()), torch.ones_like(ray), accumulate=True)
        odd.append(per % 2 == 1)
    held = odd[0] & odd[1]
    assert int(held.sum()) > 500
    where = held.nonzero()
    assert torch.equal(where[:, 1].int(), inst) and torch.equal(held.sum(1).int(), count)


@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI])
def test_one_instance_at_the_identity_is_the_parity_of_the_members_crossing_counts(device, member_handles, member):
    import triro.backend.ops as hops
    v = SC.members()[member][0]
    lo, hi = v.min(0), v.max(0)
    p = NC.hash_points(6000, 77, lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo))
    p = np.concatenate([p, PC.hostile_points(p[:60])])
    p = p[~(np.signbit(p) & (p == 0)).any(1)]      # points without a negative-zero component (the direction has none)
    n = len(p)
    mesh = member_handles[member]
    scene = make_scene(member_handles, [member], np.eye(3, 4, dtype=np.float32)[None])
    pt, dt = T(p, device), T(PC.DEFAULT, device)
    cp = hops.cross_count_native(mesh.as_wrapper, pt, dt.expand(n, 3).contiguous())
    cm = hops.cross_count_native(mesh.as_wrapper, pt, (-dt).expand(n, 3).contiguous())
    inside = (cp % 2 == 1) & (cm % 2 == 1)
    assert member == SC.TRI or int(inside.sum()) > 1000
    h, dev = scene._handle, scene.device.index
    assert torch.equal(hops.scene_points_any_native(h, dev, pt, dt), inside)
    assert torch.equal(hops.scene_points_count_native(h, dev, pt, dt), inside.int())
    offsets, inst = hops.scene_points_list_native(h, dev, pt, dt)
    assert torch.equal(offsets[1:] - offsets[:-1], inside.long()) and not inst.any()
    # the member's own contains_points (libtriro_points.so: the same parity rule on the counts of tr_intersects_count, after
    # a box test that only turns down points outside the mesh's box)
    blo, bhi = (t.reshape(3) for t in mesh.mesh_aabb)
    theirs = hops.contains_points_native(mesh.as_wrapper, pt, dt, blo, bhi)[0]
    assert torch.equal(scene.contains_points(pt), theirs)
    if member == SC.ICO:      # closed: no point is unresolved, the public method has no retry to make
        assert torch.equal(scene.contains_points(pt), mesh.contains_points(pt))


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_set_transforms_refit_and_update_raw(device):
    import scene_points_sim
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.2)).astype(np.float32)
    tv, tf = SC.members()[SC.TRI]
    a, b = make(v, f, device), make(tv, tf, device)
    mem = [(v, f), (tv, tf)]
    mesh_of = np.array([0, 1, 0], np.int32)
    rng = np.random.default_rng(11)
    M1 = np.array([SC.placement(np.eye(3), [-0.3, 0, 0]), SC.placement(np.eye(3) * 1.5, [0, 0.2, 0]), SC.placement(SC.general(rng), [0.3, 0.3, 0])])
    p = NC.hash_points(3000, 23, [-2.0, -1.5, -1.5], [2.0, 1.5, 1.5])
    brute = lambda mem, M: scene_points_sim.brute(mem, mesh_of, M, p, PC.DEFAULT)      # noqa: E731
    scene = make_scene([a, b], mesh_of, M1)
    built = (a.generation, b.generation)
    first = brute(mem, M1)
    assert (first.count >= 2).sum() > 20 and (first.count == 0).sum() > 500
    check(scene, first, p, PC.DEFAULT, device, "built")
    # an object moves: twelve floats and a commit, no member is rebuilt
    M2 = M1.copy()
    M2[2] = SC.placement(SC.rotation([0, 0, 1], 0.8) @ M1[2][:, :3].astype(np.float64), [0.3, -0.4, 0.5])
    scene.set_transforms(M2)
    want = brute(mem, M2)
    assert not np.array_equal(want.count, first.count)
    check(scene, want, p, PC.DEFAULT, device, "after set_transforms")
    assert (a.generation, b.generation) == built and scene.info()["commits"] == 2
    # a refit keeps the member's arrays: the scene stays valid and shows the moved geometry
    a.refit(T(v2, device))
    mem[0] = (v2, f)
    want2 = brute(mem, M2)
    assert not np.array_equal(want2.count, want.count)
    check(scene, want2, p, PC.DEFAULT, device, "after a refit of a member, no commit")
    check(scene, want2, p, PC.DEFAULT, device, "after a refit, one stack entry", stack_entries=1)
    assert scene.info()["commits"] == 2
    # update_raw to another triangle count moves them: stale until committed
    v3, f3 = W.icosphere(3)
    a.update_raw(T(v3, device), T(f3, device))
    pt = T(p, device)
    for call in (lambda: scene.contains_points(pt), lambda: scene.contains_count(pt), lambda: scene.containing_instances(pt)):
        with pytest.raises(ValueError, match="scene is stale: commit it again"):
            call()
    scene.commit()
    mem[0] = (v3, f3)
    check(scene, brute(mem, M2), p, PC.DEFAULT, device, "update_raw of a member, then commit")


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_the_first_calls_on_a_fresh_scene_can_be_captured_in_one_graph(device, member_handles):
    """any, count and the fill (with counts handed in) as the very first calls on a fresh scene, captured on ONE stream, then
    replayed across new points and a set_transforms (the committed table keeps its place: twelve floats per instance move)"""
    import scene_points_sim
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    n = 1000
    p1 = NC.hash_points(n, 29, [-1.5] * 3, [1.5] * 3)
    p2 = NC.hash_points(n, 31, [-1.5] * 3, [1.5] * 3)
    M2 = s["M"].copy()
    M2[0] = SC.placement(SC.rotation([1, 0, 0], 0.5) * 0.8, [-0.2, 0.1, 0.3])
    steps = ((p1, s["M"]), (p2, s["M"]), (p2, M2), (p1, M2))
    wants = [scene_points_sim.brute(SC.members(), s["mesh_of"], M, p, PC.DEFAULT) for p, M in steps]
    assert not np.array_equal(wants[1].count, wants[2].count)
    rows = max(int(w.offsets[-1]) for w in wants) + 64
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    h, dev = scene._handle, scene.device.index
    pt, dt = T(p1, device), T(PC.DEFAULT, device)
    count_in = torch.zeros(n, dtype=torch.int32, device=device)
    offsets_in = torch.zeros(n, dtype=torch.int64, device=device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the calls neither allocate nor synchronise
        any_ = hops.scene_points_any_native(h, dev, pt, dt)
        count = hops.scene_points_count_native(h, dev, pt, dt)
        inst = hops.scene_points_fill_native(h, dev, pt, dt, count_in, offsets_in, rows)
    for step, ((p, M), want) in enumerate(zip(steps, wants)):
        pt.copy_(T(p, device))
        if step == 2:
            scene.set_transforms(M)
        count_in.copy_(T(want.count, device))
        offsets_in.copy_(T(want.offsets[:-1].copy(), device))
        graph.replay()
        torch.cuda.synchronize()
        total = int(want.offsets[-1])
        assert 0 < total <= rows - 64
        poison.assert_written(any_, count, inst[:total], what=f"graph replay {step}")
        assert poison.stale_mask(inst[total:]).all(), f"graph replay {step}: rows beyond the total were written"
        PC.assert_same(scene_points_sim.Result(host(any_), host(count), want.offsets, host(inst[:total])), want, f"graph replay {step}")


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_python_methods_shapes_directions_and_errors(device, member_handles):
    import scene_points_sim
    from triro.ray import RaySceneIntersector
    s = SC.scenes()["three"]
    mem, mesh_of, M = SC.members(), s["mesh_of"], s["M"]
    p = PC.points_of("three")
    full = PC.brute_of("three")
    scene = RaySceneIntersector(member_handles, mesh_of, M)
    # [3]: a single point
    i = int(np.flatnonzero(full.count >= 2)[0])
    a, c = scene.contains_points(T(p[i], device)), scene.contains_count(T(p[i], device))
    assert a.shape == () and a.dtype == torch.bool and bool(a) and c.shape == () and c.dtype == torch.int32 and int(c) == full.count[i]
    offsets, inst = scene.containing_instances(T(p[i], device))
    assert offsets.tolist() == [0, int(full.count[i])] and np.array_equal(host(inst), PC.rows_of(full, i))
    # [5, 7, 3], without a direction and with one: a tensor, a list, an array
    n = 35
    j = max(0, i - 10)
    q = p[j:j + n]
    pt = T(q.reshape(5, 7, 3), device)
    for direction, d in ((None, PC.DEFAULT), (T(PC.OTHER, device), PC.OTHER), (PC.OTHER.tolist(), PC.OTHER), (PC.OTHER.astype(np.float64), PC.OTHER),
                         (torch.from_numpy(PC.OTHER), PC.OTHER)):
        want = scene_points_sim.brute(mem, mesh_of, M, q, d)
        assert want.any.any() and not want.any.all()
        a, c = scene.contains_points(pt, direction), scene.contains_count(pt, check_direction=direction)
        assert a.shape == (5, 7) and c.shape == (5, 7) and a.dtype == torch.bool and c.dtype == torch.int32
        offsets, inst = scene.containing_instances(pt, direction)
        assert offsets.dtype == torch.int64 and inst.dtype == torch.int32 and offsets.shape == (n + 1,)
        PC.assert_same(scene_points_sim.Result(host(a).reshape(-1), host(c).reshape(-1), host(offsets), host(inst)), want, f"[5, 7, 3], direction {direction}")
    # points that are no float32 GPU tensor are converted as the box queries convert theirs
    want = scene_points_sim.brute(mem, mesh_of, M, q, PC.DEFAULT)
    assert np.array_equal(host(scene.contains_count(q)), want.count) and np.array_equal(host(scene.contains_count(T(q.astype(np.float64), device))), want.count)
    # an empty batch; a scene without a mesh
    e = torch.zeros((0, 3), dtype=torch.float32, device=device)
    assert scene.contains_points(e).shape == (0,) and scene.contains_count(e).shape == (0,)
    offsets, inst = scene.containing_instances(e)
    assert offsets.shape == (1,) and int(offsets[0]) == 0 and inst.shape == (0,)
    nothing = RaySceneIntersector([], [], np.zeros((0, 3, 4), np.float32))
    assert not nothing.contains_points(pt).any() and not nothing.contains_count(pt).any() and int(nothing.containing_instances(pt)[0][-1]) == 0
    # one launch for any and for count; one count launch and one fill for the list
    before = dict(CALLS)
    scene.contains_points(pt)
    scene.contains_count(pt)
    assert CALLS["scene_points_any_native"] == before["scene_points_any_native"] + 1 and CALLS["scene_points_count_native"] == before["scene_points_count_native"] + 1
    scene.containing_instances(pt)
    assert CALLS["scene_points_count_native"] == before["scene_points_count_native"] + 2 and CALLS["scene_points_fill_native"] == before["scene_points_fill_native"] + 1
    # errors: CPU tensors, shapes, directions that are not three numbers
    for call in (lambda: scene.contains_points(torch.from_numpy(q)), lambda: scene.contains_count(T(q[:, :2], device)),
                 lambda: scene.containing_instances(torch.from_numpy(q)), lambda: scene.contains_points(pt, [1.0, 2.0]),
                 lambda: scene.contains_count(pt, T(np.float32([1, 2, 3, 4]), device)), lambda: scene.containing_instances(pt, 1.0)):
        with pytest.raises(ValueError):
            call()
