"""RaySceneIntersector.closest_point / signed_distance (libtriro_scene_nearest.so: k_scene_closest_point) against the host
brute force.

The oracle of every comparison is tests/host_sim/scene_nearest_sim.brute: the placed copies baked into one float32 mesh by
scene_sim.points (the scene's fmaf chain), then the brute forces of nearest_sim / within_sim -- the per-triangle function of
csrc/tr_nearest.h over every triangle -- on it, on the same float32 inputs; itself pinned to the identity placement, to an
independent float64 evaluation and to the integer-baked lattice mesh by tests/test_scene_nearest_cpu.py.  Comparisons are bit
for bit (closest, distance, instance, tri).  Direct calls of the C entry write between poisoned guard rows, checked after every
call; calls through the binding come back through a wrapper that runs poison.assert_written on its outputs; captured calls
are checked after each replay."""
import numpy as np
import pytest
import torch

import nearest_cases as NC
import poison
import scene_cases as SC
import scene_nearest_cases as NN
import scene_points_cases as PC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

GUARD = 256
CALLS = {"scene_closest_point_native": 0}
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
    original = hops.scene_closest_point_native

    def call(*args, **kwargs):
        res = original(*args, **kwargs)
        CALLS["scene_closest_point_native"] += 1
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize()
            poison.assert_written(*res, what="scene_closest_point_native")
        return res
    hops.scene_closest_point_native = call
    try:
        yield
    finally:
        hops.scene_closest_point_native = original


@pytest.fixture(scope="module")
def member_handles(device):
    """one RayMeshIntersector per member of scene_cases.members(), built once"""
    return [make(v, f, device) for v, f in SC.members()]


def native(scene, p, md, device, stack_entries=0, outputs=NN.KEYS):
    """tr_scene_closest_point itself, every output between GUARD poisoned rows on either side.  md: None (NULL and +Inf), a
    number (NULL and the scalar) or an array [n] (per point).  outputs: the optional ones (closest, distance) not named are
    passed as NULL.  After the call every guard row still holds its poison and every row inside was written.
    -> (closest or None, distance or None, instance, tri) on the host"""
    import triro.backend.ops as hops
    pt = T(np.ascontiguousarray(p, F32).reshape(-1, 3), device)
    n = len(pt)
    rt, r = None, float("inf")
    if md is not None and np.ndim(md) == 0:
        r = float(md)
    elif md is not None:
        rt = T(np.ascontiguousarray(md, F32), device)
        assert rt.shape == (n,)
    bufs = {"closest": poison.poisoned((GUARD + n + GUARD, 3), torch.float32, device) if "closest" in outputs else None,
            "distance": poison.poisoned((GUARD + n + GUARD,), torch.float32, device) if "distance" in outputs else None,
            "instance": poison.poisoned((GUARD + n + GUARD,), torch.int32, device),
            "tri": poison.poisoned((GUARD + n + GUARD,), torch.int32, device)}
    ptr = lambda k: None if bufs[k] is None else bufs[k][GUARD:].data_ptr()      # noqa: E731
    with torch.cuda.device(device):
        hops._check(hops.get_scene_nearest_module().tr_scene_closest_point(
            scene._handle, pt.data_ptr() if n else None, n, None if rt is None else rt.data_ptr(), r, ptr("closest"), ptr("distance"),
            ptr("instance"), ptr("tri"), int(stack_entries), hops._stream_ptr(pt.device)))
    torch.cuda.synchronize()
    out = []
    for k in NN.KEYS:
        b = bufs[k]
        if b is None:
            out.append(None)
            continue
        stale = poison.stale_mask(b).reshape(len(b), -1)
        assert stale[:GUARD].all() and stale[GUARD + n:].all(), f"{k}: a guard row was written ({n} points, stack_entries {stack_entries})"
        assert not stale[GUARD:GUARD + n].any(), f"{k}: a row inside was not written"
        out.append(host(b[GUARD:GUARD + n]))
    return tuple(out)


def check(scene, want, p, md, device, what, **kw):
    got = native(scene, p, md, device, **kw)
    NN.assert_same(got, want, what)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.scenes()))
def test_scenes_at_every_stack_limit(device, member_handles, name):
    """every scene, the `none` scene among them: the kernel against the brute force at stack limits 0 (all), 1 and 2, unbounded
    and under the three per-point max_distance arrays; each optional output left out in turn; a scalar max_distance"""
    import scene_nearest_sim as S
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    p = NN.points_of(name)
    for entries in (0, 1, 2):
        got = check(scene, NN.brute_of(name), p, None, device, f"{name}, stack_entries {entries}", stack_entries=entries)
    bad = ~NN.valid_points(p)
    assert bad.sum() >= 30 and (got[2][bad] == -1).all() and (got[3][bad] == -1).all() and np.isinf(got[1][bad]).all() and np.isnan(got[0][bad]).all()
    for kind in ("hash", "exact", "below"):
        for entries in (0, 1):
            check(scene, NN.brute_of(name, kind), p, NN.max_distance_of(name, kind), device, f"{name}, max_distance {kind}, stack_entries {entries}",
                  stack_entries=entries)
    for outputs in (("closest",), ("distance",), ()):
        got = check(scene, NN.brute_of(name, "hash"), p, NN.max_distance_of(name, "hash"), device, f"{name}, outputs {outputs}", stack_entries=2,
                    outputs=outputs)
        assert (got[0] is None) == ("closest" not in outputs) and (got[1] is None) == ("distance" not in outputs)
    # one max_distance for every point: the scalar argument against the same value per point
    finite = NN.brute_of(name).distance[np.isfinite(NN.brute_of(name).distance)]
    radius = F32(np.median(finite)) if len(finite) else F32(1)
    want = S.brute(SC.members(), s["mesh_of"], s["M"], p, radius)
    assert name == "none" or ((want.instance >= 0).sum() > 100 and (want.instance < 0).sum() > 100)
    check(scene, want, p, radius, device, f"{name}, scalar max_distance")
    check(scene, want, p, np.full(len(p), radius, F32), device, f"{name}, the same max_distance per point", stack_entries=1)
    for radius in (np.nan, -1.0):
        got = native(scene, p[:300], radius, device)
        assert (got[2] == -1).all() and (got[3] == -1).all() and np.isinf(got[1]).all() and np.isnan(got[0]).all()
    # the same instances listed in reverse: the same answer after renumbering, away from exact ties between instances (where
    # the instance listed first wins in either listing, at the same distance)
    r = SC.reversed_scene(s)
    got = native(make_scene(member_handles, r["mesh_of"], r["M"]), p, None, device, stack_entries=1)
    keep = ~NN.cross_instance_ties(name)
    back = NN.renumbered(S.Result(*got), len(s["mesh_of"]))
    NN.assert_same([x[keep] for x in back], [x[keep] for x in NN.brute_of(name)], f"{name}, reversed listing renumbered")
    assert np.array_equal(NN.bits(got[1]), NN.bits(NN.brute_of(name).distance))


def test_the_fixtures_are_what_the_comparisons_need():
    NN.check_fixture_conditions()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_tails_of_the_lane_and_block_indexing(device, member_handles):
    """point counts 0 ... 129 and 4133: the answer of a point does not depend on its neighbours, so every count is a slice of
    one brute force"""
    s = SC.scenes()["three"]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    base, full = NN.points_of("three"), NN.brute_of("three")
    md, bounded = NN.max_distance_of("three", "hash"), NN.brute_of("three", "hash")
    start = len(base) - 60 - 100      # (the last hashed and placed points, then hostile ones: every count above 100 ends in invalid points)
    assert len(set(full.instance[start:start + 129].tolist())) >= 3
    for n in range(130):
        sl = slice(start, start + n)
        got = check(scene, [x[sl] for x in full], base[sl], None, device, f"{n} points")
        assert got[0].shape == (n, 3) and got[1].shape == (n,) and got[2].shape == (n,) and got[3].shape == (n,)
        check(scene, [x[sl] for x in bounded], base[sl], md[sl], device, f"{n} points, max_distance per point, one stack entry", stack_entries=1)
    n = 4133
    idx = np.arange(n) % len(base)
    check(scene, [x[idx] for x in full], base[idx], None, device, f"{n} points")
    check(scene, [x[idx] for x in bounded], base[idx], md[idx], device, f"{n} points, max_distance per point", stack_entries=1)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_a_wave_whose_lanes_have_their_winners_in_different_instances(device, member_handles):
    """scene_nearest_cases.split_waves(): a wave whose even lanes win in the first and odd lanes in the third instance, a wave
    and a whole block of invalid points, lanes that win in the three instances in turn, then hashed points; and the reversed
    listing"""
    import scene_nearest_sim as S
    mesh_of, M, p, want = NN.split_waves()
    for entries in (0, 1):
        check(make_scene(member_handles, mesh_of, M), want, p, None, device, f"split lanes, stack_entries {entries}", stack_entries=entries)
        rev = native(make_scene(member_handles, mesh_of[::-1].copy(), M[::-1].copy()), p, None, device, stack_entries=entries)
        NN.assert_same(NN.renumbered(S.Result(*rev), 3), want, f"split lanes, reversed listing renumbered, stack_entries {entries}")


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_whole_waves_and_whole_blocks_of_invalid_points(device, member_handles):
    import scene_nearest_sim as S
    s = SC.scenes()["three"]
    base = NN.points_of("three")[:1024].copy()
    p = base.copy()
    p[64:128] = PC.hostile_points(base[64:128])            # a whole wave
    p[256:512] = PC.hostile_points(base[256:512])          # two whole blocks
    p[700:703] = PC.hostile_points(base[700:703])          # single lanes
    p[896:1024] = F32(np.nan)                              # the last block: every component of every point
    bad = ~NN.valid_points(p)
    p[64:128][~bad[64:128]] = F32(np.inf)                  # (3e38 is finite: these waves are to be invalid in every lane)
    p[256:512][~bad[256:512]] = F32(-np.inf)
    bad = ~NN.valid_points(p)
    md = np.full(len(p), np.inf, F32)
    md[128:192] = F32(np.nan)                              # a wave that is invalid through its max_distance alone
    md[192:256] = F32(-2.0)
    want = S.brute(SC.members(), s["mesh_of"], s["M"], p, md)
    assert bad[64:128].all() and bad[256:512].all() and bad[896:].all() and (want.instance[bad] == -1).all() and (want.instance[128:256] == -1).all()
    assert (want.instance >= 0).sum() > 300
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    for entries in (0, 1):
        check(scene, want, p, md, device, f"invalid waves and blocks, stack_entries {entries}", stack_entries=entries)
    allbad = np.full((300, 3), np.nan, F32)
    got = native(scene, allbad, None, device)
    assert (got[2] == -1).all() and (got[3] == -1).all() and np.isinf(got[1]).all() and np.isnan(got[0]).all()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_a_placement_that_overflows(device):
    q = NN.overflow_scene()
    scene = make_scene([make(v, f, device) for v, f in q["members"]], q["mesh_of"], q["M"])
    for entries in (0, 1, 2):
        got = check(scene, q["want"], q["p"], None, device, f"overflowing placement, stack_entries {entries}", stack_entries=entries)
    assert not np.isnan(got[1]).any() and not np.isnan(got[0][got[2] >= 0]).any()


def test_exact_placements_against_the_integer_baked_mesh(device):
    L = NN.lattice()
    scene = make_scene([make(v.astype(F32), f.astype(np.int32), device) for v, f in L["members"]], L["mesh_of"], L["M"])
    for entries in (0, 1):
        check(scene, L["want"], L["p"], None, device, f"lattice scene, stack_entries {entries}", stack_entries=entries)


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "odd", "many65"])
def test_the_baked_identity_on_the_same_gpu(device, member_handles, name):
    """tr_closest_point and tr_within_closest on a handle built from the baked mesh, on the same GPU: closest, distance and
    the triangle (mapped by the instance offsets) are the scene's, bit for bit"""
    import scene_nearest_sim as S
    import triro.backend.ops as hops
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    bv, bf, inst_of, tri_of = S.bake(SC.members(), s["mesh_of"], s["M"])
    baked = make(bv, bf, device)
    p = NN.points_of(name)
    pt = T(p, device)
    h, dev = scene._handle, scene.device.index
    inst_of, tri_of = T(inst_of, device), T(tri_of, device)

    def mapped(tri):
        hit = tri >= 0
        safe = tri.clamp(min=0).long()
        return torch.where(hit, inst_of[safe], torch.full_like(tri, -1)), torch.where(hit, tri_of[safe], torch.full_like(tri, -1))

    c, d, i, t = hops.scene_closest_point_native(h, dev, pt)
    bc, bd, bt = hops.closest_point_native(baked.as_wrapper, pt)
    bi, bt = mapped(bt)
    NN.assert_same((host(c), host(d), host(i), host(t)), (host(bc), host(bd), host(bi), host(bt)), f"{name}: the scene against tr_closest_point on the baked handle")
    assert int((i >= 0).sum()) > 1000
    for kind in ("hash", "exact"):
        md = T(NN.max_distance_of(name, kind), device)
        c, d, i, t = hops.scene_closest_point_native(h, dev, pt, md)
        bc, bd, bt = hops.within_closest_native(baked.as_wrapper, pt, md)
        bi, bt = mapped(bt)
        NN.assert_same((host(c), host(d), host(i), host(t)), (host(bc), host(bd), host(bi), host(bt)), f"{name}, {kind}: the scene against tr_within_closest on the baked handle")
        assert int((i >= 0).sum()) > 300 and int((i < 0).sum()) > 300


@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI, SC.INACTIVE])
def test_one_instance_at_the_identity_is_closest_point_of_the_member(device, member_handles, member):
    import triro.backend.ops as hops
    v = SC.members()[member][0]
    assert not (np.signbit(v) & (v == 0)).any()
    fin = v[np.isfinite(v).all(1)]
    lo, hi = (fin.min(0), fin.max(0)) if len(fin) else (-np.ones(3), np.ones(3))
    p = NC.hash_points(6000, 77, lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo))
    p = np.concatenate([p, fin[::7], PC.hostile_points(p[:60])])
    pt = T(p, device)
    mesh = member_handles[member]
    scene = make_scene(member_handles, [member], np.eye(3, 4, dtype=F32)[None])
    c, d, i, t = hops.scene_closest_point_native(scene._handle, scene.device.index, pt)
    mc, md, mt = hops.closest_point_native(mesh.as_wrapper, pt)
    NN.assert_same((host(c), host(d), host(i), host(t)), (host(mc), host(md), host(torch.where(mt >= 0, 0, -1).int()), host(mt)), f"member {member} at the identity")
    assert member == SC.INACTIVE or int((i == 0).sum()) > 6000


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_set_transforms_refit_and_update_raw(device):
    import scene_nearest_sim as S
    v, f = W.icosphere(2)
    v = W.displaced(v, seed=4, amplitude=0.05)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * F32(1.2)).astype(F32)
    tv, tf = SC.members()[SC.TRI]
    a, b = make(v, f, device), make(tv, tf, device)
    mem = [(v, f), (tv, tf)]
    mesh_of = np.array([0, 1, 0], np.int32)
    rng = np.random.default_rng(11)
    M1 = np.array([SC.placement(np.eye(3), [-0.3, 0, 0]), SC.placement(np.eye(3) * 1.5, [0, 0.2, 0]), SC.placement(SC.general(rng), [0.3, 0.3, 0])])
    p = NC.hash_points(3000, 23, [-2.0, -1.5, -1.5], [2.0, 1.5, 1.5])
    brute = lambda mem, M: S.brute(mem, mesh_of, M, p)      # noqa: E731
    scene = make_scene([a, b], mesh_of, M1)
    built = (a.generation, b.generation)
    first = brute(mem, M1)
    assert all((first.instance == k).sum() > 50 for k in range(3))
    check(scene, first, p, None, device, "built")
    # an object moves: twelve floats and a commit, no member is rebuilt
    M2 = M1.copy()
    M2[2] = SC.placement(SC.rotation([0, 0, 1], 0.8) @ M1[2][:, :3].astype(np.float64), [0.3, -0.4, 0.5])
    scene.set_transforms(M2)
    want = brute(mem, M2)
    assert not np.array_equal(want.instance, first.instance)
    check(scene, want, p, None, device, "after set_transforms")
    assert (a.generation, b.generation) == built and scene.info()["commits"] == 2
    # a refit keeps the member's arrays: the scene stays valid and shows the moved geometry
    a.refit(T(v2, device))
    mem[0] = (v2, f)
    want2 = brute(mem, M2)
    assert not np.array_equal(NN.bits(want2.distance), NN.bits(want.distance))
    check(scene, want2, p, None, device, "after a refit of a member, no commit")
    check(scene, want2, p, None, device, "after a refit, one stack entry", stack_entries=1)
    assert scene.info()["commits"] == 2
    # update_raw to another triangle count moves them: stale until committed
    v3, f3 = W.icosphere(3)
    a.update_raw(T(v3, device), T(f3, device))
    pt = T(p, device)
    for call in (lambda: scene.closest_point(pt), lambda: scene.closest_point(pt, 0.5), lambda: scene.signed_distance(pt)):
        with pytest.raises(ValueError, match="scene is stale: commit it again"):
            call()
    scene.commit()
    mem[0] = (v3, f3)
    check(scene, brute(mem, M2), p, None, device, "update_raw of a member, then commit")


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_the_first_call_on_a_fresh_scene_can_be_captured_in_one_graph(device, member_handles):
    """the unbounded and the per-point bounded query as the very first calls on a fresh scene, captured on ONE stream, then
    replayed across new points and a set_transforms (the committed table keeps its place: twelve floats per instance move)"""
    import scene_nearest_sim as S
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    n = 1000
    p1 = NC.hash_points(n, 29, [-1.5] * 3, [1.5] * 3)
    p2 = NC.hash_points(n, 31, [-1.5] * 3, [1.5] * 3)
    M2 = s["M"].copy()
    M2[0] = SC.placement(SC.rotation([1, 0, 0], 0.5) * 0.8, [-0.2, 0.1, 0.3])
    radii = (NC.hash_points(n, 37, [0.0] * 3, [0.4] * 3)[:, 0]).astype(F32)
    steps = ((p1, s["M"]), (p2, s["M"]), (p2, M2), (p1, M2))
    wants = [(S.brute(SC.members(), s["mesh_of"], M, p), S.brute(SC.members(), s["mesh_of"], M, p, radii)) for p, M in steps]
    assert not np.array_equal(wants[1][0].instance, wants[2][0].instance)
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    h, dev = scene._handle, scene.device.index
    pt, rt = T(p1, device), T(radii, device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the call neither allocates nor synchronises
        free = hops.scene_closest_point_native(h, dev, pt)
        bounded = hops.scene_closest_point_native(h, dev, pt, rt)
    for step, ((p, M), (want, want_b)) in enumerate(zip(steps, wants)):
        pt.copy_(T(p, device))
        if step == 2:
            scene.set_transforms(M)
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(*free, *bounded, what=f"graph replay {step}")
        NN.assert_same([host(x) for x in free], want, f"graph replay {step}")
        NN.assert_same([host(x) for x in bounded], want_b, f"graph replay {step}, bounded")
        assert (want_b.instance >= 0).sum() > 100 and (want_b.instance < 0).sum() > 100


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_python_methods_shapes_max_distance_and_errors(device, member_handles):
    import scene_nearest_sim as S
    from triro.ray import RaySceneIntersector
    s = SC.scenes()["three"]
    mem, mesh_of, M = SC.members(), s["mesh_of"], s["M"]
    p = NN.points_of("three")
    full = NN.brute_of("three")
    scene = RaySceneIntersector(member_handles, mesh_of, M)
    # [3]: a single point
    c, d, i, t = scene.closest_point(T(p[5], device))
    assert c.shape == (3,) and d.shape == () and i.shape == () and t.shape == () and c.dtype == d.dtype == torch.float32 and i.dtype == t.dtype == torch.int32
    NN.assert_same([host(x).reshape((1,) + tuple(x.shape)) for x in (c, d, i, t)], [x[5:6] for x in full], "a single point")
    # [5, 7, 3]: unbounded, a scalar, a tensor that broadcasts, a list
    n = 35
    q = p[100:100 + n]
    pt = T(q.reshape(5, 7, 3), device)
    row = (np.arange(7, dtype=F32) * F32(0.05)).astype(F32)
    for md, per_point in ((None, None), (0.2, np.full(n, 0.2, F32)), (T(row, device), np.tile(row, 5)), (row.tolist(), np.tile(row, 5)),
                          (torch.from_numpy(row.reshape(1, 7)), np.tile(row, 5))):
        want = S.brute(mem, mesh_of, M, q, per_point)
        c, d, i, t = scene.closest_point(pt, md)
        assert c.shape == (5, 7, 3) and d.shape == (5, 7) and i.shape == (5, 7) and t.shape == (5, 7)
        NN.assert_same((host(c).reshape(-1, 3), host(d).reshape(-1), host(i).reshape(-1), host(t).reshape(-1)), want, f"[5, 7, 3], max_distance {md}")
    assert (want.instance >= 0).any() and (want.instance < 0).any()
    # points that are no float32 GPU tensor are converted as the mesh class converts its
    want = S.brute(mem, mesh_of, M, q)
    NN.assert_same([host(x) for x in scene.closest_point(q)], want, "a numpy array")
    NN.assert_same([host(x) for x in scene.closest_point(T(q.astype(np.float64), device))], want, "float64 points")
    # an empty batch; a scene without a mesh
    e = torch.zeros((0, 3), dtype=torch.float32, device=device)
    c, d, i, t = scene.closest_point(e)
    assert c.shape == (0, 3) and d.shape == (0,) and i.shape == (0,) and t.shape == (0,) and scene.signed_distance(e).shape == (0,)
    nothing = RaySceneIntersector([], [], np.zeros((0, 3, 4), F32))
    c, d, i, t = nothing.closest_point(pt)
    assert bool(torch.isnan(c).all()) and bool(torch.isinf(d).all()) and bool((i == -1).all()) and bool((t == -1).all())
    # one launch per call
    before = CALLS["scene_closest_point_native"]
    scene.closest_point(pt)
    scene.closest_point(pt, 0.3)
    assert CALLS["scene_closest_point_native"] == before + 2
    # errors: CPU tensors, shapes, a max_distance that does not broadcast or lives elsewhere
    for call in (lambda: scene.closest_point(torch.from_numpy(q)), lambda: scene.closest_point(T(q[:, :2], device)),
                 lambda: scene.closest_point(pt, T(np.ones(4, F32), device)), lambda: scene.signed_distance(torch.from_numpy(q)),
                 lambda: scene.signed_distance(pt, [1.0, 2.0])):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("name", ["three", "odd"])
def test_signed_distance_is_the_distance_with_the_sign_of_contains_points(device, member_handles, name):
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    p = NN.points_of(name)
    ok = NN.valid_points(p) & (np.abs(np.nan_to_num(p)) < 1e38).all(1)
    pt = T(p[ok].reshape(-1, 2, 3) if ok.sum() % 2 == 0 else p[ok][:-1].reshape(-1, 2, 3), device)
    for direction in (None, PC.OTHER.tolist()):
        sd = scene.signed_distance(pt, direction)
        d = scene.closest_point(pt)[1]
        inside = scene.contains_points(pt, direction)
        assert sd.shape == pt.shape[:-1] and sd.dtype == torch.float32
        assert torch.equal(sd, torch.where(inside, d, -d))
        assert int(inside.sum()) > 100 and int((~inside).sum()) > 100 and bool((sd[inside] >= 0).all()) and bool((sd[~inside] <= 0).all())
    want = NN.brute_of(name).distance[ok][:pt.shape[0] * 2]
    assert np.array_equal(NN.bits(np.abs(host(sd)).reshape(-1)), NN.bits(want))
