"""RaySceneIntersector.triangles_any / triangles_count / faces_meeting_triangles / mesh_collides / mesh_contacts /
colliding_instances (libtriro_scene_tris.so: k_scene_tris<>, k_scene_tris_rows) against the host brute force.

The oracle of every comparison is tests/host_sim/scene_tris_sim.brute: the placed copies baked into one float32 mesh by
scene_sim.points (the scene's fmaf chain), then tris_sim.brute -- the predicate of csrc/tr_tris.h over every triangle -- on it,
on the same float32 inputs; itself pinned to the identity placement and to the integer reference on exact placements by
tests/test_scene_tris_cpu.py.  Comparisons are element for element (any, count, offsets, instance, face).  Direct calls of the
C entries write between poisoned guard rows, checked after every call; calls through the binding come back through a wrapper
that runs poison.assert_written on their outputs; captured calls are checked after each replay."""
import numpy as np
import pytest
import torch

import poison
import scene_cases as SC
import scene_nearest_cases as NN
import scene_tris_cases as ST
import tris_cases as TC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

GUARD = 256
CALLS = {"scene_tris_native": 0, "scene_tris_fill_native": 0}
F32 = np.float32


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


def make_scene(meshes, mesh_of, M):
    from triro.ray import RaySceneIntersector
    return RaySceneIntersector(meshes, mesh_of, M)


def host(x):
    return None if x is None else x.cpu().numpy()


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every call of the binding: counted, and -- outside a graph capture -- all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    originals = {name: getattr(hops, name) for name in CALLS}

    def wrap(name):
        def call(*args, **kwargs):
            res = originals[name](*args, **kwargs)
            CALLS[name] += 1
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
                poison.assert_written(*(res if isinstance(res, tuple) else (res,)), what=name)
            return res
        return call
    for name in CALLS:
        setattr(hops, name, wrap(name))
    try:
        yield
    finally:
        for name, fn in originals.items():
            setattr(hops, name, fn)


@pytest.fixture(scope="module")
def handles(device):
    """member set -> one RayMeshIntersector per member, built once"""
    return {"scene_cases": [make(v, f, device) for v, f in SC.members()],
            "overflow": [make(v, f, device) for v, f in NN.overflow_scene()["members"]],
            "small": [make(v, f, device) for v, f in ST.small_members()]}


def guarded(n, dtype, device):
    return poison.poisoned((GUARD + n + GUARD,), dtype, device)


def inside(buf, n, what, written=True):
    """the n rows between the guards, on the host, after checking that the guards kept their poison and -- where `written`
    -- that every row inside lost it"""
    stale = poison.stale_mask(buf).reshape(len(buf), -1)
    assert stale[:GUARD].all() and stale[GUARD + n:].all(), f"{what}: a guard row was written"
    if written:
        assert not stale[GUARD:GUARD + n].any(), f"{what}: a row inside was not written"
    return host(buf[GUARD:GUARD + n])


def native(scene, tri, device, stack_entries=0):
    """tr_scene_tris_any, _count and _fill themselves, every output between GUARD poisoned rows on either side
    -> scene_tris_sim.Result on the host"""
    import scene_tris_sim as S
    import triro.backend.ops as hops
    lib = hops.get_scene_tris_module()
    tt = T(np.ascontiguousarray(tri, F32).reshape(-1, 3, 3), device)
    n = len(tt)
    ptr = tt.data_ptr() if n else None
    any_, count = guarded(n, torch.uint8, device), guarded(n, torch.int32, device)
    stream = hops._stream_ptr(tt.device)
    what = f"{n} triangles, stack_entries {stack_entries}"
    with torch.cuda.device(device):
        hops._check(lib.tr_scene_tris_any(scene._handle, ptr, n, any_[GUARD:].data_ptr(), int(stack_entries), stream))
        hops._check(lib.tr_scene_tris_count(scene._handle, ptr, n, count[GUARD:].data_ptr(), int(stack_entries), stream))
    torch.cuda.synchronize()
    a, c = inside(any_, n, "any: " + what), inside(count, n, "count: " + what)
    assert set(np.unique(a).tolist()) <= {0, 1}
    off = np.zeros(n + 1, np.int64)
    np.cumsum(c, out=off[1:])
    total = int(off[-1])
    inst, face = guarded(total, torch.int32, device), guarded(total, torch.int32, device)
    ct, ot = T(c, device), T(off[:-1], device)
    with torch.cuda.device(device):
        hops._check(lib.tr_scene_tris_fill(scene._handle, ptr, n, ct.data_ptr() if n else None, ot.data_ptr() if n else None, total,
                                           inst[GUARD:].data_ptr(), face[GUARD:].data_ptr(), int(stack_entries), stream))
    torch.cuda.synchronize()
    return S.Result(a != 0, c, off, inside(inst, total, "instance: " + what), inside(face, total, "face: " + what))


def check(scene, want, tri, device, what, **kw):
    got = native(scene, tri, device, **kw)
    ST.assert_same(got, want, what)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ST.names())
def test_scenes_at_every_stack_limit(device, handles, name):
    """every scene -- the empty one, 1 to 65 instances, members from one triangle to the deep tree, the hostile placements of
    `odd` and `overflow` -- at stack limits 1, 2, 3 and 32 (all): the kernels against the brute force"""
    members, mesh_of, M = ST.scene_of(name)
    scene = make_scene(handles[ST.member_set(name)], mesh_of, M)
    tri, want = ST.queries_of(name), ST.brute_of(name)
    for entries in (1, 2, 3, 32, 0):
        got = check(scene, want, tri, device, f"{name}, stack_entries {entries}", stack_entries=entries)
    ST.check_identities(got, name)
    bad = ~np.isfinite(tri).all(axis=(1, 2))
    assert bad.sum() >= 27 and not got.any[bad].any() and not got.count[bad].any()


def test_the_fixtures_are_what_the_comparisons_need():
    ST.check_fixture_conditions()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_tails_of_the_lane_and_block_indexing(device, handles):
    """n = 0, 1, 63, 64, 65, 127, 128, 129 and 257 queries: the answer of a query does not depend on its neighbours, so every
    count is a slice of one brute force"""
    import scene_tris_sim as S
    name = "small5"
    members, mesh_of, M = ST.scene_of(name)
    scene = make_scene(handles["small"], mesh_of, M)
    base, full = ST.queries_of(name), ST.brute_of(name)
    assert len(base) >= 257 and full.any[:257].sum() > 60
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 257):
        c = full.count[:n]
        off = np.zeros(n + 1, np.int64)
        np.cumsum(c, out=off[1:])
        want = S.Result(full.any[:n], c, off, full.instance[:off[-1]], full.face[:off[-1]])
        for entries in (0, 1):
            got = check(scene, want, base[:n], device, f"{n} triangles, stack_entries {entries}", stack_entries=entries)
        assert got.any.shape == (n,) and got.count.shape == (n,)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_a_wave_whose_lanes_meet_different_instances(device, handles):
    """scene_tris_cases.split_wave(): lane i meets instance i mod 3 only; the long triangles have pairs in instance 0 and
    overflow a stack of one entry in instance 1 -- the count keeps instance 0's pairs exactly once"""
    import scene_tris_sim as S
    from sim import SimBVH
    mesh_of, M, tri, want = ST.split_wave()
    B = [SimBVH(v, f) for v, f in ST.small_members()]
    _, lost = S.walk(B, mesh_of, M, tri, 1, want_lost=True)
    assert lost[192:].any()
    scene = make_scene(handles["small"], mesh_of, M)
    for entries in (0, 1, 2):
        got = check(scene, want, tri, device, f"split wave, stack_entries {entries}", stack_entries=entries)
    for i in np.flatnonzero(lost[192:]) + 192:
        rows = got.instance[got.offsets[i]:got.offsets[i + 1]]
        assert (rows == 0).sum() == (want.instance[want.offsets[i]:want.offsets[i + 1]] == 0).sum() > 0
    # the same instances listed in reverse
    rev = native(make_scene(handles["small"], mesh_of[::-1].copy(), M[::-1].copy()), tri, device, stack_entries=1)
    ST.assert_same(ST.renumbered(rev, np.arange(3)[::-1]), want, "split wave, reversed listing renumbered")


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_row_limits(device, handles):
    """a total smaller than the sum of the counts, and counts from a different batch: no write beyond `total` or beyond
    count[i] rows of a query (poisoned guard rows and poisoned rows of other queries intact), and what is written are pairs
    of the query, ascending"""
    import triro.backend.ops as hops
    lib = hops.get_scene_tris_module()
    name = "small5"
    members, mesh_of, M = ST.scene_of(name)
    scene = make_scene(handles["small"], mesh_of, M)
    tri, want = ST.queries_of(name), ST.brute_of(name)
    n, total = len(tri), int(want.offsets[-1])
    tt = T(tri, device)
    stream = hops._stream_ptr(tt.device)
    pairs = [set(zip(want.instance[want.offsets[i]:want.offsets[i + 1]].tolist(), want.face[want.offsets[i]:want.offsets[i + 1]].tolist()))
             for i in range(n)]

    def fill(count, off, rows, entries):
        inst, face = guarded(rows, torch.int32, device), guarded(rows, torch.int32, device)
        ct, ot = T(np.ascontiguousarray(count, np.int32), device), T(np.ascontiguousarray(off, np.int64), device)
        with torch.cuda.device(device):
            hops._check(lib.tr_scene_tris_fill(scene._handle, tt.data_ptr(), n, ct.data_ptr(), ot.data_ptr(), rows, inst[GUARD:].data_ptr(),
                                               face[GUARD:].data_ptr(), entries, stream))
        torch.cuda.synchronize()
        stale = host(poison.stale_mask(inst[GUARD:GUARD + rows]) | poison.stale_mask(face[GUARD:GUARD + rows]))
        return inside(inst, rows, "instance", written=False), inside(face, rows, "face", written=False), stale

    # (a) the total cut short
    cut = total - total // 3
    for entries in (0, 1):
        inst, face, stale = fill(want.count, want.offsets[:-1], cut, entries)
        whole = want.offsets[1:] <= cut
        assert whole.sum() > 50 and (~whole).sum() > 20
        assert not stale.any()
        assert np.array_equal(inst[:want.offsets[1:][whole].max()], want.instance[:want.offsets[1:][whole].max()])
        for i in np.flatnonzero(~whole & (want.offsets[:-1] < cut)):      # the query the cut goes through: its rows are pairs of it
            rows = list(zip(inst[want.offsets[i]:cut].tolist(), face[want.offsets[i]:cut].tolist()))
            assert set(rows) <= pairs[i] and rows == sorted(set(rows))
    # (b) counts of a different batch: the queries rolled by seven against the counts and offsets as they were
    other = np.roll(np.arange(n), 7)
    tt = T(tri[other], device)
    for entries in (0, 1):
        inst, face, stale = fill(want.count, want.offsets[:-1], total, entries)
        seen_short = seen_long = 0
        for i in range(n):
            lo, hi = want.offsets[i], want.offsets[i + 1]
            mine = pairs[other[i]]
            rows = [r for r, s in zip(zip(inst[lo:hi].tolist(), face[lo:hi].tolist()), stale[lo:hi]) if not s]
            assert set(rows) <= mine and len(rows) == len(set(rows)) == min(hi - lo, len(mine)), f"query {i}: {len(rows)} rows of {hi - lo}, {len(mine)} pairs"
            seen_short += len(mine) < hi - lo
            seen_long += len(mine) > hi - lo
            # rows remain a permutation of what was there: written rows and poisoned rows, nothing invented
            assert stale[lo:hi].sum() == (hi - lo) - len(rows)
        assert seen_short > 10 and seen_long > 10


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "odd", "small8"])
def test_the_baked_identity_on_the_same_gpu(device, handles, name):
    """tr_tris_any / _count / _fill on a handle built from the baked mesh, on the same GPU: the scene's answers, with
    (instance, face) mapped to the baked index by the instance offsets"""
    import scene_tris_sim as S
    import triro.backend.ops as hops
    members, mesh_of, M = ST.scene_of(name)
    scene = make_scene(handles[ST.member_set(name)], mesh_of, M)
    bv, bf, inst_of, tri_of = S.bake(members, mesh_of, M)
    baked = make(bv, bf, device)
    tt = T(ST.queries_of(name), device)
    h, dev = scene._handle, scene.device.index
    assert torch.equal(hops.scene_tris_native(h, dev, tt, "any"), hops.tris_native(baked.as_wrapper, tt, "any"))
    assert torch.equal(hops.scene_tris_native(h, dev, tt, "count"), hops.tris_native(baked.as_wrapper, tt, "count"))
    off, inst, face = hops.scene_faces_meeting_triangles_native(h, dev, tt)
    boff, bface = hops.faces_meeting_triangles_native(baked.as_wrapper, tt)
    assert torch.equal(off, boff) and int(off[-1]) > 500
    assert np.array_equal(host(inst), inst_of[host(bface)]) and np.array_equal(host(face), tri_of[host(bface)])
    ST.assert_same((host(hops.scene_tris_native(h, dev, tt, "any")), host(hops.scene_tris_native(h, dev, tt, "count")), host(off), host(inst),
                    host(face)), ST.brute_of(name), name)


@pytest.mark.parametrize("member", [ST.ONE, ST.TWO, ST.CUBE, ST.ICO80, ST.DEEP])
def test_one_instance_at_the_identity_is_the_triangle_query_of_the_member(device, handles, member):
    import triro.backend.ops as hops
    v, f = ST.small_members()[member]
    tri = np.concatenate([q for _, q in TC.query_sets(v, f)])
    tt = T(np.concatenate([tri, TC.hostile_triangles(tri[:40])[0]]), device)
    mesh = handles["small"][member]
    scene = make_scene(handles["small"], [member], np.eye(3, 4, dtype=F32)[None])
    h, dev = scene._handle, scene.device.index
    for query in ("any", "count"):
        assert torch.equal(hops.scene_tris_native(h, dev, tt, query), hops.tris_native(mesh.as_wrapper, tt, query))
    off, inst, face = hops.scene_faces_meeting_triangles_native(h, dev, tt)
    moff, mface = hops.faces_meeting_triangles_native(mesh.as_wrapper, tt)
    assert torch.equal(off, moff) and torch.equal(face, mface) and bool((inst == 0).all()) and int(off[-1]) > 0


def test_exact_placements_against_the_integer_reference(device):
    E = ST.exact_scene()
    scene = make_scene([make(v, f, device) for v, f in E["members"]], E["mesh_of"], E["M"])
    for entries in (0, 1):
        stats = ST.check_exact(native(scene, E["tri"], device, stack_entries=entries), f"exact scene, stack_entries {entries}")
    print("pairs %d, meeting %d, of which only touching %d, coplanar and meeting %d" % stats)


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_set_transforms_refit_and_update_raw(device):
    import scene_tris_sim as S
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * F32(1.2)).astype(F32)
    tv, tf = SC.members()[SC.TRI]
    a, b = make(v, f, device), make(tv, tf, device)
    mem = [(v, f), (tv, tf)]
    mesh_of = np.array([0, 1, 0], np.int32)
    rng = np.random.default_rng(11)
    M1 = np.array([SC.placement(np.eye(3), [-0.3, 0, 0]), SC.placement(np.eye(3) * 1.5, [0, 0.2, 0]), SC.placement(SC.general(rng), [0.3, 0.3, 0])])
    tri = TC.hashed_triangles(900, [-2.0, -1.5, -1.5], [2.0, 1.5, 1.5], 2.0, seed=23)
    brute = lambda mem, M: S.brute(mem, mesh_of, M, tri)      # noqa: E731
    scene = make_scene([a, b], mesh_of, M1)
    built = (a.generation, b.generation)
    first = brute(mem, M1)
    assert all((first.instance == k).sum() > 20 for k in range(3))
    check(scene, first, tri, device, "built")
    # an object moves: twelve floats and a commit, no member is rebuilt
    M2 = M1.copy()
    M2[2] = SC.placement(SC.rotation([0, 0, 1], 0.8) @ M1[2][:, :3].astype(np.float64), [0.3, -0.4, 0.5])
    scene.set_transforms(M2)
    want = brute(mem, M2)
    assert not np.array_equal(want.count, first.count)
    check(scene, want, tri, device, "after set_transforms")
    assert (a.generation, b.generation) == built and scene.info()["commits"] == 2
    # a refit keeps the member's arrays: the scene stays valid and shows the moved geometry
    a.refit(T(v2, device))
    mem[0] = (v2, f)
    want2 = brute(mem, M2)
    assert not np.array_equal(want2.count, want.count)
    check(scene, want2, tri, device, "after a refit of a member, no commit")
    check(scene, want2, tri, device, "after a refit, one stack entry", stack_entries=1)
    assert scene.info()["commits"] == 2
    # update_raw to another triangle count moves them: stale until committed
    v3, f3 = W.icosphere(3)
    a.update_raw(T(v3, device), T(f3, device))
    tt = T(tri, device)
    for call in (lambda: scene.triangles_any(tt), lambda: scene.triangles_count(tt), lambda: scene.faces_meeting_triangles(tt),
                 lambda: scene.mesh_collides(tv, tf), lambda: scene.mesh_contacts(tv, tf), lambda: scene.colliding_instances(tv, tf)):
        with pytest.raises(ValueError, match="scene is stale: commit it again"):
            call()
    scene.commit()
    mem[0] = (v3, f3)
    check(scene, brute(mem, M2), tri, device, "update_raw of a member, then commit")


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_the_first_call_on_a_fresh_scene_can_be_captured_in_one_graph(device, handles):
    """any, count and a fill (on counts and offsets computed beforehand for a row budget) as the very first calls on a fresh
    scene, captured on ONE stream, then replayed across new triangles and a set_transforms"""
    import scene_tris_sim as S
    import triro.backend.ops as hops
    name = "small5"
    members, mesh_of, M = ST.scene_of(name)
    n = 300
    t1 = ST.queries_of(name)[:n].copy()
    t2 = np.roll(t1, 31, axis=0)
    M2 = M.copy()
    M2[1] = SC.placement(SC.rotation([1, 0, 0], 0.5) * 0.8, [0.3, 0.1, -0.1])
    steps = ((t1, M), (t2, M), (t2, M2), (t1, M2))
    wants = [S.brute(members, mesh_of, Mk, t) for t, Mk in steps]
    assert not np.array_equal(wants[1].count, wants[2].count)
    scene = make_scene(handles["small"], mesh_of, M)
    h, dev = scene._handle, scene.device.index
    tt = T(t1, device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the calls neither allocate nor synchronise
        any_ = hops.scene_tris_native(h, dev, tt, "any")
        count = hops.scene_tris_native(h, dev, tt, "count")
    for step, ((t, Mk), want) in enumerate(zip(steps, wants)):
        tt.copy_(T(t, device))
        if step == 2:
            scene.set_transforms(Mk)
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(any_, count, what=f"graph replay {step}")
        assert np.array_equal(host(any_), want.any) and np.array_equal(host(count), want.count), f"graph replay {step}"
    # the fill, captured as the first call on another fresh scene, replays to the same bits
    scene2 = make_scene(handles["small"], mesh_of, M2)
    want = wants[3]
    ct, ot = T(want.count, device), T(want.offsets[:-1], device)
    total = int(want.offsets[-1])
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=side):
        inst, face = hops.scene_tris_fill_native(scene2._handle, dev, tt, ct, ot, total)
    for step in range(2):
        graph2.replay()
        torch.cuda.synchronize()
        poison.assert_written(inst, face, what=f"fill replay {step}")
        assert np.array_equal(host(inst), want.instance) and np.array_equal(host(face), want.face), f"fill replay {step}"
        inst.fill_(-5); face.fill_(-5)


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_python_methods_shapes_chunks_and_errors(device, handles):
    import scene_tris_sim as S
    from triro.ray import RaySceneIntersector
    name = "small5"
    members, mesh_of, M = ST.scene_of(name)
    tri, full = ST.queries_of(name), ST.brute_of(name)
    scene = RaySceneIntersector(handles["small"], mesh_of, M)
    # [3, 3]: a single triangle; [5, 7, 3, 3]
    k = int(np.flatnonzero(full.count > 1)[0])
    a, c = scene.triangles_any(T(tri[k], device)), scene.triangles_count(T(tri[k], device))
    assert a.shape == () and c.shape == () and a.dtype == torch.bool and c.dtype == torch.int32 and bool(a) and int(c) == full.count[k]
    q = tri[:35]
    qt = T(q.reshape(5, 7, 3, 3), device)
    a, c = scene.triangles_any(qt), scene.triangles_count(qt)
    assert a.shape == (5, 7) and c.shape == (5, 7)
    assert np.array_equal(host(a).reshape(-1), full.any[:35]) and np.array_equal(host(c).reshape(-1), full.count[:35])
    off, inst, face = scene.faces_meeting_triangles(qt)
    assert off.dtype == torch.int64 and inst.dtype == face.dtype == torch.int32 and off.shape == (36,)
    end = full.offsets[35]
    assert np.array_equal(host(off), full.offsets[:36]) and np.array_equal(host(inst), full.instance[:end]) and np.array_equal(host(face), full.face[:end])
    # a numpy array and float64 are converted as the mesh class converts its
    assert np.array_equal(host(scene.triangles_count(q)), full.count[:35])
    assert np.array_equal(host(scene.triangles_count(T(q.astype(np.float64), device))), full.count[:35])
    # an empty batch; a scene without a mesh
    e = torch.zeros((0, 3, 3), dtype=torch.float32, device=device)
    assert scene.triangles_any(e).shape == (0,) and scene.triangles_count(e).shape == (0,)
    off, inst, face = scene.faces_meeting_triangles(e)
    assert host(off).tolist() == [0] and inst.shape == face.shape == (0,)
    nothing = RaySceneIntersector([], [], np.zeros((0, 3, 4), F32))
    assert not bool(nothing.triangles_any(qt).any()) and int(nothing.triangles_count(qt).sum()) == 0
    assert nothing.mesh_contacts(*ST.small_members()[ST.CUBE]).shape == (0, 3) and not nothing.mesh_collides(*ST.small_members()[ST.CUBE])
    # mesh against scene: the icosphere, moved into the scene, as the other mesh
    ov, of = ST.small_members()[ST.ICO80]
    ov = (ov * F32(0.8) + F32([0.5, 0.1, -0.2])).astype(F32)
    want = S.brute(members, mesh_of, M, ov[of])
    rows = np.stack([np.repeat(np.arange(len(of)), want.count), want.instance, want.face], 1).astype(np.int64)
    assert len(rows) > 40 and len(np.unique(want.instance)) >= 2
    whole = scene.mesh_contacts(T(ov, device), T(of, device))
    assert whole.dtype == torch.int64 and np.array_equal(host(whole), rows)
    for chunk in (1, 7, len(of)):
        assert torch.equal(scene.mesh_contacts(ov, of, chunk=chunk), whole), chunk
    assert scene.mesh_collides(ov, of) and scene.mesh_collides(ov, of, chunk=1) and scene.mesh_collides(T(ov, device), T(of, device), chunk=7)
    hit = scene.colliding_instances(ov, of, chunk=7)
    assert hit.dtype == torch.int64 and np.array_equal(host(hit), np.unique(want.instance)) and torch.equal(hit, scene.colliding_instances(ov, of))
    far = (ov + F32([50, 0, 0])).astype(F32)
    assert not scene.mesh_collides(far, of) and scene.mesh_contacts(far, of).shape == (0, 3) and scene.colliding_instances(far, of).shape == (0,)
    # mesh_collides stops at the first chunk that says yes
    first = int(np.flatnonzero(want.count > 0)[0])
    before = CALLS["scene_tris_native"]
    assert scene.mesh_collides(ov, of, chunk=1)
    assert CALLS["scene_tris_native"] == before + first + 1
    # errors: CPU tensors, shapes, another device's kind of argument
    for call in (lambda: scene.triangles_any(torch.from_numpy(q)), lambda: scene.triangles_count(T(q[:, :2], device)),
                 lambda: scene.faces_meeting_triangles(T(q.reshape(-1, 9), device)), lambda: scene.mesh_collides(ov[:, :2], of),
                 lambda: scene.mesh_contacts(ov, of[:, :2]), lambda: scene.mesh_contacts(ov, of + len(ov)), lambda: scene.mesh_collides(ov, of, chunk=0),
                 lambda: scene.colliding_instances(ov, of, chunk=-1)):
        with pytest.raises(ValueError):
            call()
    import triro.backend.ops as hops
    with pytest.raises(ValueError, match="scene lives on"):
        hops.scene_tris_native(scene._handle, scene.device.index + 1, qt.reshape(-1, 3, 3), "any")
    with pytest.raises(ValueError, match="query must be"):
        hops.scene_tris_native(scene._handle, scene.device.index, qt.reshape(-1, 3, 3), "list")
    with pytest.raises(ValueError):
        hops.scene_tris_fill_native(scene._handle, scene.device.index, qt.reshape(-1, 3, 3), T(full.count[:35], device), T(full.offsets[:35], device), -1)
