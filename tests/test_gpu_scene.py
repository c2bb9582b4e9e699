"""Instanced scenes (libtriro_scene.so, k_scene_query<any | closest>) against the host brute force.

The oracle of every comparison is tests/host_sim/scene_sim.brute: the per-triangle predicate of csrc/tr_range.h on the ray of
each instance's frame (csrc/tr_scene.h), over every triangle of every instance, reduced by (t, instance, face) -- itself
pinned to a second computation in numpy, to the range query at the identity and to the integer-arithmetic reference by
tests/test_scene_cpu.py.  Comparisons are bit for bit, +Inf included.  Every native call of this module comes back through a
wrapper that runs poison.assert_written on everything it returns (the autouse fixture `checked_native`); the captured calls
are checked after each replay."""
import numpy as np
import pytest
import torch

import poison
import range_cases as RC
import scene_cases as SC
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu


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
    """every native call: -- outside a graph capture -- all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    originals = {name: getattr(hops, name) for name in ("scene_any_native", "scene_closest_native")}

    def wrap(name):
        def call(*args, **kwargs):
            res = originals[name](*args, **kwargs)
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


@pytest.fixture(scope="module")
def member_handles(device):
    """one RayMeshIntersector per member of scene_cases.members(), built once"""
    return [make(v, f, device) for v, f in SC.members()]


def bound(x, n, device):
    return None if x is None else T(np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (n,))), device)


def as_dict(any_, closest):
    out = {}
    if any_ is not None:
        out["any"] = any_.cpu().numpy().reshape(-1)
    if closest is not None:
        for k, x in zip(("hit", "front", "instance", "tri", "t", "loc", "uv"), closest):
            out[k] = None if x is None else x.cpu().numpy()
    return out


def native(scene, o, d, lo, hi, device, **kw):
    """both queries on dense rays: the dict of scene_sim"""
    import triro.backend.ops as hops
    n = len(o)
    ot, dt, lt, ht = T(o, device), T(d, device), bound(lo, n, device), bound(hi, n, device)
    h, dev = scene._handle, scene.device.index
    return as_dict(hops.scene_any_native(h, dev, ot, dt, lt, ht, **kw), hops.scene_closest_native(h, dev, ot, dt, lt, ht, **kw))


def check(scene, want, o, d, lo, hi, device, what, **kw):
    got = native(scene, o, d, lo, hi, device, **kw)
    RC.assert_same_bits(got, want, what, keys=SC.KEYS)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.scenes()))
def test_scenes_at_every_stack_limit(device, member_handles, name):
    s = SC.scenes()[name]
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    info = scene.info()
    assert info["num_instances"] == len(s["mesh_of"]) and info["num_members"] == len(member_handles) and info["commits"] == 1
    for kind in ("none", "hash", "exact"):
        lo, hi, want = SC.brute_of(name, kind)
        for entries in (1, 2, 0):
            got = check(scene, want, s["o"], s["d"], lo, hi, device, f"{name}, bounds {kind}, stack_entries {entries}", stack_entries=entries)
    lo, hi, want = SC.brute_of(name, "hash")
    got = check(scene, want, s["o"], s["d"], lo, hi, device, f"{name}, once more")
    RC.check_miss_rule(got, s["bad"], name)
    assert (got["instance"][s["bad"]] == -1).all()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4133])
def test_tails_of_the_lane_and_block_indexing(device, member_handles, n):
    import ctypes as C
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    lo, hi, want = SC.brute_of("three", "hash")
    assert len(s["o"]) < 4133
    reps = -(-4133 // len(s["o"]))
    o, d, lo, hi = (np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:n] for x in (s["o"], s["d"], lo, hi))
    want = {k: np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:n] for k, x in want.items()}
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    got = check(scene, want, o, d, lo, hi, device, f"{n} rays")
    assert got["any"].shape == (n,) and got["loc"].shape == (n, 3) and got["uv"].shape == (n, 2) and got["t"].shape == (n,) and got["instance"].shape == (n,)
    # tr_scene_closest itself, each optional output left out in turn, then all of them
    ot, dt, lt, ht = T(o, device), T(d, device), bound(lo, n, device), bound(hi, n, device)
    spec = dict(instance=((n,), torch.int32), tri=((n,), torch.int32), t=((n,), torch.float32), hit=((n,), torch.bool), front=((n,), torch.bool),
                loc=((n, 3), torch.float32), uv=((n, 2), torch.float32))
    ptr = lambda x: None if x is None else x.data_ptr()      # noqa: E731
    for leave_out in (("instance",), ("t",), ("hit",), ("front",), ("loc",), ("uv",), ("instance", "t", "hit", "front", "loc", "uv")):
        outs = {k: None if k in leave_out else hops._new_output(sh, dt_, ot.device) for k, (sh, dt_) in spec.items()}
        with torch.cuda.device(ot.device):
            hops._check(hops.get_scene_module().tr_scene_closest(
                scene._handle, C.byref(hops.make_rays(ot, dt)), ptr(lt), ptr(ht), *(ptr(outs[k]) for k in ("instance", "tri", "t", "hit", "front", "loc", "uv")),
                0, torch.cuda.current_stream(ot.device).cuda_stream))
        torch.cuda.synchronize()
        poison.assert_written(*outs.values(), what=f"tr_scene_closest without {leave_out}")
        RC.assert_same_bits({k: None if x is None else x.cpu().numpy() for k, x in outs.items()}, want, f"{n} rays, no {leave_out}", keys=SC.KEYS_CLOSEST)
    hit, front, inst, tri, t, loc, uv = hops.scene_closest_native(scene._handle, scene.device.index, ot, dt, lt, ht, want_t=False, want_dense=False)
    assert hit is None and front is None and loc is None and uv is None and t is None
    assert np.array_equal(tri.cpu().numpy(), want["tri"]) and np.array_equal(inst.cpu().numpy(), want["instance"])


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_strided_rays_with_a_broadcast_origin(device, member_handles):
    import scene_sim
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
    want = scene_sim.brute(SC.members(), s["mesh_of"], s["M"], np.tile(origin, (n, 1)), d, lo, hi)
    assert want["hit"].sum() > 100 and len(set(want["instance"].tolist())) >= 3
    lt, ht = T(lo, device), T(hi, device)
    h, dev = scene._handle, scene.device.index
    a = hops.scene_any_native(h, dev, origins, dirs, lt, ht)
    c = hops.scene_closest_native(h, dev, origins, dirs, lt, ht)
    assert a.shape == (H, Wd) and c[2].shape == (H, Wd) and c[5].shape == (H, Wd, 3) and c[6].shape == (H, Wd, 2) and c[4].shape == (H, Wd)
    RC.assert_same_bits(as_dict(a, c), want, "[H, W, 3] view, broadcast origin", keys=SC.KEYS)
    # rows of a transposed tensor: the general stride path for both
    ot = T(np.tile(origin, (n, 1)).reshape(H, Wd, 3), device).transpose(0, 1)
    dtr = T(d.reshape(H, Wd, 3), device).transpose(0, 1)
    want_t = {k: np.ascontiguousarray(x.reshape(H, Wd, *x.shape[1:]).swapaxes(0, 1)).reshape(n, *x.shape[1:]) for k, x in want.items() if k in SC.KEYS}
    lt2 = T(np.ascontiguousarray(lo.reshape(H, Wd).T).reshape(-1), device)
    ht2 = T(np.ascontiguousarray(hi.reshape(H, Wd).T).reshape(-1), device)
    RC.assert_same_bits(as_dict(hops.scene_any_native(h, dev, ot, dtr, lt2, ht2), hops.scene_closest_native(h, dev, ot, dtr, lt2, ht2)),
                        want_t, "transposed rays", keys=SC.KEYS)


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_a_wave_whose_lanes_split_between_instances(device, member_handles):
    """three spheres in a row, 10 apart; even lanes start around the first with tmax below 4, odd lanes around the third: no ray can
    reach another sphere than its own.  Then the instances listed in reverse order: the same bits after renumbering."""
    import scene_sim
    rng = np.random.default_rng(3)
    M = np.array([SC.placement(SC.general(rng, 0.9), [-10, 0, 0]), SC.placement(np.eye(3), [0, 0, 0]), SC.placement(SC.general(rng, 0.9), [10, 0, 0])])
    mesh_of = np.array([SC.ICO, SC.SHELLS, SC.ICO], np.int32)
    n = 4096
    o, d = W.hash_rays(n, 17, [-1.2] * 3, [1.2] * 3)
    o[0::2, 0] -= 10
    o[1::2, 0] += 10
    lo, hi = RC.hash_bounds(n, 19, 4.0)
    want = scene_sim.brute(SC.members(), mesh_of, M, o, d, lo, hi)
    hit = want["hit"]
    assert set(want["instance"][0::2].tolist()) == {-1, 0} and set(want["instance"][1::2].tolist()) == {-1, 2}
    assert hit[0::2].sum() > 100 and hit[1::2].sum() > 100 and (~hit).sum() > 200
    for entries in (0, 1):
        check(make_scene(member_handles, mesh_of, M), want, o, d, lo, hi, device, f"split lanes, stack_entries {entries}", stack_entries=entries)
        got = native(make_scene(member_handles, mesh_of[::-1].copy(), M[::-1].copy()), o, d, lo, hi, device, stack_entries=entries)
        got["instance"] = np.where(got["hit"], 2 - got["instance"], -1).astype(np.int32)
        RC.assert_same_bits(got, want, f"split lanes, reversed listing renumbered, stack_entries {entries}", keys=SC.KEYS)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_exact_transforms_against_the_integer_reference(device):
    import scene_sim
    L = SC.lattice_scene()
    meshes = [make(v, f, device) for v, f in L["members"]]
    scene = make_scene(meshes, L["mesh_of"], L["M"])
    want = scene_sim.brute(L["members"], L["mesh_of"], L["M"], L["o"], L["d"])
    for entries in (0, 1):
        got = check(scene, want, L["o"], L["d"], None, None, device, f"lattice scene, stack_entries {entries}", stack_entries=entries)
        ties, other, mask = SC.check_against_ideal(L, got, f"lattice scene on the GPU, stack_entries {entries}")
        assert ties > 2000


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_lifecycle_set_transforms_refit_and_update_raw(device):
    import scene_sim
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
    scene = make_scene([a, b], mesh_of, M1)
    built = (a.generation, b.generation)
    check(scene, scene_sim.brute(mem, mesh_of, M1, o, d, lo, hi), o, d, lo, hi, device, "built")
    # an object moves: twelve floats and a commit, no member is rebuilt
    M2 = M1.copy()
    M2[2] = SC.placement(SC.rotation([0, 0, 1], 0.8) @ M1[2][:, :3].astype(np.float64), [0.6, -0.4, 0.5])
    scene.set_transforms(T(np.concatenate([M2, np.tile(np.float32([0, 0, 0, 1]), (3, 1, 1))], 1), device))      # [n, 4, 4], a tensor on the GPU
    want = scene_sim.brute(mem, mesh_of, M2, o, d, lo, hi)
    assert (want["instance"] != scene_sim.brute(mem, mesh_of, M1, o, d, lo, hi)["instance"]).sum() > 20
    check(scene, want, o, d, lo, hi, device, "after set_transforms")
    assert (a.generation, b.generation) == built and scene.info()["commits"] == 2
    # a refit keeps the member's arrays: the scene stays valid and shows the moved geometry
    a.refit(T(v2, device))
    mem[0] = (v2, f)
    want = scene_sim.brute(mem, mesh_of, M2, o, d, lo, hi)
    check(scene, want, o, d, lo, hi, device, "after a refit of a member, no commit")
    check(scene, want, o, d, lo, hi, device, "after a refit, one stack entry", stack_entries=1)
    assert scene.info()["commits"] == 2
    # update_raw to another triangle count moves them: stale until committed
    v3, f3 = W.icosphere(3)
    a.update_raw(T(v3, device), T(f3, device))
    for call in (lambda: scene.intersects_any(T(o, device), T(d, device)), lambda: scene.intersects_closest(T(o, device), T(d, device)),
                 lambda: scene.segments_any(T(o, device), T(o + d, device))):
        with pytest.raises(ValueError, match="scene is stale: commit it again"):
            call()
    scene.commit()
    mem[0] = (v3, f3)
    check(scene, scene_sim.brute(mem, mesh_of, M2, o, d, lo, hi), o, d, lo, hi, device, "update_raw of a member, then commit")
    # an update_raw that keeps the triangle count rebuilds inside the same arrays: no commit needed
    a.update_raw(T((v3 * np.float32(0.8)).astype(np.float32), device), T(f3, device))
    mem[0] = ((v3 * np.float32(0.8)).astype(np.float32), f3)
    check(scene, scene_sim.brute(mem, mesh_of, M2, o, d, lo, hi), o, d, lo, hi, device, "update_raw with the same triangle count")


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_the_first_call_on_a_fresh_scene_can_be_captured(device, member_handles):
    import scene_sim
    import triro.backend.ops as hops
    s = SC.scenes()["three"]
    n = 1000
    o1, d1 = W.hash_rays(n, 29, [-1.5] * 3, [1.5] * 3)
    o2, d2 = W.hash_rays(n, 31, [-1.5] * 3, [1.5] * 3)
    b1, b2 = RC.hash_bounds(n, 33, 3.0), RC.hash_bounds(n, 35, 3.0)
    scene = make_scene(member_handles, s["mesh_of"], s["M"])
    ot, dt, lt, ht = T(o1, device), T(d1, device), T(b1[0], device), T(b1[1], device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # no warm-up: the calls neither allocate nor synchronise
        out_any = hops.scene_any_native(scene._handle, scene.device.index, ot, dt, lt, ht)
        out_closest = hops.scene_closest_native(scene._handle, scene.device.index, ot, dt, lt, ht)
    for step, (o, d, (lo, hi)) in enumerate(((o1, d1, b1), (o2, d2, b2))):
        for src, dst in ((o, ot), (d, dt), (lo, lt), (hi, ht)):
            dst.copy_(T(src, device))
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(out_any, *out_closest, what=f"graph replay {step}")
        RC.assert_same_bits(as_dict(out_any, out_closest), scene_sim.brute(SC.members(), s["mesh_of"], s["M"], o, d, lo, hi), f"graph replay {step}",
                            keys=SC.KEYS)


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_python_api_shapes_transforms_segments_and_errors(device, member_handles):
    import scene_sim
    from triro.ray import RaySceneIntersector
    s = SC.scenes()["three"]
    mem, mesh_of, M = SC.members(), s["mesh_of"], s["M"]
    o, d, lo, hi = s["o"], s["d"], s["lo"], s["hi"]
    M44 = np.concatenate([M, np.tile(np.float32([0, 0, 0, 1]), (len(M), 1, 1))], 1)
    scene = RaySceneIntersector(member_handles, mesh_of.tolist(), M44)              # [n, 4, 4] numpy, a list of indices
    scene34 = RaySceneIntersector(member_handles, torch.from_numpy(mesh_of), torch.from_numpy(M))      # [n, 3, 4] tensors
    n = 35
    # [3]: a single ray, scalar bounds
    w1 = scene_sim.brute(mem, mesh_of, M, o[:1], d[:1], 0.25, 2.5)
    a = scene.intersects_any(T(o[0], device), T(d[0], device), 0.25, 2.5)
    c = scene.intersects_closest(T(o[0], device), T(d[0], device), 0.25, 2.5)
    assert a.shape == () and a.dtype == torch.bool and c[5].shape == (3,) and c[6].shape == (2,) and c[4].shape == () and c[2].shape == ()
    assert [x.dtype for x in c] == [torch.bool, torch.bool, torch.int32, torch.int32, torch.float32, torch.float32, torch.float32]
    RC.assert_same_bits(as_dict(a, c), w1, "[3] with scalar bounds", keys=SC.KEYS)
    # [5, 7, 3] with tensor bounds of the batch shape, on both scenes
    ot, dt = T(o[:n].reshape(5, 7, 3), device), T(d[:n].reshape(5, 7, 3), device)
    wn = scene_sim.brute(mem, mesh_of, M, o[:n], d[:n], lo[:n], hi[:n])
    for sc in (scene, scene34):
        a = sc.intersects_any(ot, dt, T(lo[:n].reshape(5, 7), device), T(hi[:n].reshape(5, 7), device))
        c = sc.intersects_closest(ot, dt, T(lo[:n].reshape(5, 7), device), T(hi[:n].reshape(5, 7), device))
        assert a.shape == (5, 7) and c[0].shape == (5, 7) and c[2].shape == (5, 7) and c[5].shape == (5, 7, 3) and c[6].shape == (5, 7, 2)
        RC.assert_same_bits(as_dict(a, c), wn, "[5, 7, 3]", keys=SC.KEYS)
    # default bounds, one bound alone
    wd = scene_sim.brute(mem, mesh_of, M, o[:n], d[:n])
    RC.assert_same_bits(as_dict(scene.intersects_any(ot, dt), scene.intersects_closest(ot, dt)), wd, "default bounds", keys=SC.KEYS)
    wb = scene_sim.brute(mem, mesh_of, M, o[:n], d[:n], None, 0.75)
    RC.assert_same_bits(as_dict(scene.intersects_any(ot, dt, tmax=0.75), scene.intersects_closest(ot, dt, None, torch.tensor(0.75))), wb, "tmax alone", keys=SC.KEYS)
    # segments: the float32 difference and the range [0, 1]
    m = 1500
    p0, p1 = o[:m], (o[:m] + d[:m] * hi[:m, None]).astype(np.float32)
    so, sd, slo, shi = RC.segment_rays(p0, p1)
    ws = scene_sim.brute(mem, mesh_of, M, so, sd, slo, shi)
    assert ws["hit"].sum() > 200 and (~ws["hit"]).sum() > 200
    a, c = scene.segments_any(T(p0, device), T(p1, device)), scene.segments_closest(T(p0, device), T(p1, device))
    RC.assert_same_bits(as_dict(a, c), ws, "segments", keys=SC.KEYS)
    assert ((c[4][c[0]] >= 0) & (c[4][c[0]] <= 1)).all()
    a = scene.segments_any(T(p0[:24].reshape(2, 3, 4, 3), device), T(p1[:24].reshape(2, 3, 4, 3), device))
    assert a.shape == (2, 3, 4) and np.array_equal(a.cpu().numpy().reshape(-1), ws["any"][:24])
    # errors
    bad = M44.copy()
    bad[1, 3, 2] = 0.5
    with pytest.raises(ValueError, match="last row"):
        RaySceneIntersector(member_handles, mesh_of, bad)
    with pytest.raises(ValueError, match="last row"):
        scene.set_transforms(bad)
    with pytest.raises(ValueError):
        RaySceneIntersector(member_handles, mesh_of, M[:, :2, :])
    with pytest.raises(ValueError):
        scene.set_transforms(M[:2])
    with pytest.raises(ValueError, match="outside"):
        RaySceneIntersector(member_handles, [0, len(member_handles), 1], M)
    with pytest.raises(ValueError, match="outside"):
        RaySceneIntersector(member_handles, [0, -1, 1], M)
    with pytest.raises(ValueError):
        RaySceneIntersector(member_handles + [object()], mesh_of, M)
    with pytest.raises(ValueError):
        scene.intersects_any(torch.from_numpy(o[:4]), torch.from_numpy(d[:4]))
    with pytest.raises(ValueError):
        scene.intersects_closest(T(o[:4, :2], device), T(d[:4, :2], device))
    with pytest.raises(ValueError):
        scene.intersects_any(T(o[:4], device), T(d[:5], device))
    with pytest.raises(ValueError):
        scene.intersects_any(ot, dt, tmin=T(lo[:6], device))
    with pytest.raises(ValueError):
        scene.segments_closest(T(o[:4], device), T(o[:5], device))
    # a refused set_transforms leaves the placements the native scene has; no mesh at all is a scene in which every ray misses
    assert np.array_equal(scene.transforms, M.reshape(-1, 12)) and scene.info()["commits"] == 1
    nothing = RaySceneIntersector([], [], np.zeros((0, 3, 4), np.float32))
    assert nothing.info()["num_members"] == 0 and not nothing.intersects_any(ot, dt).any()
    c = nothing.intersects_closest(ot, dt)
    assert (c[2] == -1).all() and (c[3] == -1).all() and torch.isposinf(c[4]).all() and not c[0].any()
    # the scene after all the refusals is the scene before
    RC.assert_same_bits(as_dict(scene.intersects_any(ot, dt), scene.intersects_closest(ot, dt)), wd, "after the refusals", keys=SC.KEYS)


def test_a_member_on_another_device_is_refused(device, member_handles):
    """needs two GPUs: on a box with one this test SKIPS, and what then runs of the refusal is the C entry's, against stand-in
    handles, in tests/test_scene_cpu.py::test_invalid_arguments_are_refused_without_a_device"""
    import ctypes as C
    import triro.backend.ops as hops
    from triro.ray import RaySceneIntersector
    if torch.cuda.device_count() < 2:
        pytest.skip("a member on another device needs a second GPU")
    s = SC.scenes()["three"]
    v, f = SC.members()[SC.TRI]
    far = make(v, f, torch.device("cuda:1"))
    with pytest.raises(ValueError, match="one device"):
        RaySceneIntersector(member_handles + [far], s["mesh_of"], s["M"])
    # the C entry itself, past the Python check
    scene = RaySceneIntersector(member_handles, s["mesh_of"], s["M"])
    with pytest.raises(ValueError, match="lives on device 1"):
        hops.scene_commit(scene._handle, [m.as_wrapper._inner for m in member_handles] + [far.as_wrapper._inner], s["mesh_of"],
                          s["M"].reshape(-1, 12), scene.device.index)
    assert scene.info()["commits"] == 1 and C.sizeof(C.c_void_p) == 8
