"""The float top of the stealing closest / first / any launch on the grid nodes (csrc/kernels_direct.inc: the table loop in
front of the uniform top of wave_traverse_steal; csrc/tr_bvh.h: tr_top_rec, tr_top_test; csrc/bvh_build.hip: k_emit,
k_update_boxes, tr_top_upload):
every case against the oracle bit for bit, and against the same launch with the handle's table switched off (float_top = 0:
tr_bvh_set_float_top, no table is passed: the parent's loop) on every output, byte for byte.  tests/test_float_top_cpu.py
holds the loop to the uniform top trip by trip on the host; here the kernels run it.

What the loop and its table can get wrong, and the smallest shape that reaches it:
  * trees shallower than the table (1, 2, 20, 320 triangles), one around the table's depth (chosen from bvh_info), deeper
    ones (icosphere(5) under 64 x 64 and 128 x 128 pixels: the hand-over to the generic loop below the table);
  * a leaf child of the root (one large triangle beside a dense cluster): absent slots;
  * all eight octants (cameras on the diagonals), tiles that straddle octants (a camera on an axis: the failed entry test),
    axis-parallel rays of both signs and directions with -0.0 components (which octant is a zero's?);
  * partial waves (64, 65, 127 rays), the give-away thresholds steal = 2, 4, 5, 64 and the default;
  * the other instantiations: the deep tree of tests/hostile_rays.py (64-bit trail), and compact = 0 (64-bit addressing: the
    stealing launch then walks the exact nodes, a kernel without the loop, which must not notice the table);
  * the table's life: build, refit, a captured graph replayed after the refit, update_raw to another size, save / load --
    after each the downloaded table is the host function (tr_top_build_slot) of the downloaded grid nodes, byte for byte.

That the stealing launch really walks the table is shown by overwriting the root's record with planes no ray can meet
(tr_bvh_poke_top): every hit is lost with the table and none without it.  The instrumented launch (trace_stats) never
steals, so it does not run this loop and its counters cannot show that the loop ran; they are compared between
float_top = 1 and 0 all the same (the switch must not change that launch)."""
import contextlib

import numpy as np
import pytest

import float_top_sim as F
import poison
import workloads as W
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import PRUNING, T, check_query, run_query
from test_gpu_plain_stack import _expect_stealing_grid_launch, _expected

pytestmark = pytest.mark.gpu


def _image(w, h, distance=2.5, vfov=40.0):
    o, d = W.pinhole_grid(w, h, vfov_deg=vfov, distance=distance)
    return (np.ascontiguousarray(np.broadcast_to(o, d.shape), np.float32).reshape(-1, 3),
            np.ascontiguousarray(d, np.float32).reshape(-1, 3))


def _camera(at, w=64, h=64, vfov=40.0):
    """a pinhole image of the origin seen from `at`"""
    at = np.asarray(at, np.float64)
    fwd = -at / np.linalg.norm(at)
    up0 = np.float64([0, 1, 0]) if abs(fwd[1]) < 0.9 else np.float64([1, 0, 0])
    right = np.cross(fwd, up0); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    t = np.tan(np.radians(vfov) / 2)
    ys, xs = np.meshgrid((np.arange(h) + 0.5) / h * 2 - 1, (np.arange(w) + 0.5) / w * 2 - 1, indexing="ij")
    d = fwd[None, None] + (xs * t * w / h)[..., None] * right + (-ys * t)[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = np.ascontiguousarray(d.reshape(-1, 3), np.float32)
    return np.ascontiguousarray(np.broadcast_to(at.astype(np.float32), d.shape)), d


def _bytes(got):
    got = got if isinstance(got, (tuple, list)) else (got,)
    return [g.cpu().numpy().tobytes() for g in got]


def _levels(r):
    top = r.as_wrapper.download_top()
    return 0 if top is None else int(np.log2(top.shape[1] + 1))


def assert_table(r, what):
    """the handle's table is the host function of its grid nodes, byte for byte"""
    qn, _ = r.as_wrapper.download_qnodes()
    top = r.as_wrapper.download_top()
    if len(qn) == 0:
        assert top is None, f"{what}: a table without a hierarchy"
        return
    want = F.table(qn, int(np.log2(top.shape[1] + 1)))
    assert top.shape == want.shape and top.tobytes() == want.tobytes(), f"{what}: the table is not tr_top_build_slot of the grid nodes"


@contextlib.contextmanager
def no_table(r):
    """launches on `r` are handed no table (tr_bvh_set_float_top(0)): the parent's loop walks the top"""
    r.as_wrapper.set_float_top(False)
    try:
        yield
    finally:
        r.as_wrapper.set_float_top(True)


def both(r, query, ot, dt, exp, what, stealing=True):
    """float_top = 1 against the oracle, then float_top = 0 against it and against float_top = 1 byte for byte"""
    got = run_query(r, query, ot, dt)
    check_query(query, got, exp, what + ", float_top = 1")
    if stealing:
        _expect_stealing_grid_launch(r, query, what)
    one = _bytes(got)
    with no_table(r):
        got0 = run_query(r, query, ot, dt)
        check_query(query, got0, exp, what + ", float_top = 0")
        if stealing:
            _expect_stealing_grid_launch(r, query, what + ", float_top = 0")
        assert _bytes(got0) == one, f"{what}: float_top = 0 and 1 differ"


def _make(v, f, device):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


def _leaf_at_the_top():
    """one large triangle beside a dense cluster: a child of the root is a leaf"""
    v, f = W.icosphere(3)
    big = np.float32([[6, -3, -3], [6, 3, -3], [6, 0, 4]])
    return np.concatenate([v, big]).astype(np.float32), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)


def _mesh(name):
    if name == "1 triangle":
        v, f = W.two_triangles()
        return v[:3].copy(), f[:1].copy()
    if name == "2 triangles":
        return W.two_triangles()
    if name == "20 triangles":
        return W.icosphere(0)
    if name == "leaf at the top":
        return _leaf_at_the_top()
    return W.icosphere(int(name.split()[-1]))


# ---- trees shallower than, around and deeper than the table ----------------------------------------------------------------
@pytest.mark.parametrize("query", PRUNING)
@pytest.mark.parametrize("mesh,px", [("1 triangle", 32), ("2 triangles", 32), ("20 triangles", 32), ("icosphere 2", 64),
                                     ("icosphere 5", 64), ("icosphere 5", 128), ("leaf at the top", 64)])
def test_against_the_oracle_and_against_float_top_0(device, mesh, px, query):
    v, f = _mesh(mesh)
    o, d = _image(px, px, distance=3.0 if "triangle" in mesh and mesh[0] in "12" else 2.5)
    if mesh == "leaf at the top":
        o2, d2 = _camera([9.0, 0.5, 0.5], 32, 32, vfov=60.0)      # a second camera that sees the large triangle past the cluster
        o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    exp = _expected(f"float top {mesh} {px}", v, f, o, d)
    r = _make(v, f, device)
    info = r.bvh_info()
    assert_table(r, mesh)
    if mesh == "leaf at the top":
        assert (r.as_wrapper.download_qnodes()[0][0, 6:8].view(np.int32) < 0).sum() == 1, "no leaf child at the root"
        assert exp["closest"][2].max() == len(f) - 1, "no ray sees the large triangle"
    if mesh == "icosphere 5":
        assert info["depth"] > _levels(r), "the tree is not deeper than the table"
    if mesh in ("2 triangles", "20 triangles", "icosphere 2"):
        assert info["depth"] < _levels(r), "the tree is not shallower than the table"
    both(r, query, T(o, device), T(d, device), exp, f"{mesh}, {px} x {px}, {query}", stealing=len(f) >= 2)


@pytest.mark.parametrize("query", PRUNING)
def test_a_tree_around_the_tables_depth(device, query):
    """the smallest icosphere whose hierarchy is at least as deep as the table, and the one before it"""
    levels, seen = None, []
    for sub in range(1, 6):
        v, f = W.icosphere(sub)
        r = _make(v, f, device)
        levels = _levels(r)
        seen.append((sub, r.bvh_info()["depth"]))
        if r.bvh_info()["depth"] >= levels:
            break
    assert seen[-1][1] >= levels > seen[-2][1], f"no icosphere around {levels} levels: {seen}"
    for sub, _ in seen[-2:]:
        v, f = W.icosphere(sub)
        o, d = _image(64, 64)
        r = _make(v, f, device)
        assert_table(r, f"icosphere {sub}")
        both(r, query, T(o, device), T(d, device), _expected(f"float top icosphere {sub} 64", v, f, o, d), f"icosphere {sub}, {query}")


@pytest.mark.parametrize("sub", [2, 5])
def test_the_table_of_a_tree_in_karras_numbering(device, sub):
    """node_layout = 0: k_emit writes nodes and table without layout positions"""
    v, f = W.icosphere(sub)
    o, d = _image(64, 64)
    with options(node_layout=0):
        r = _make(v, f, device)
    assert_table(r, f"icosphere {sub}, node_layout = 0")
    both(r, "closest", T(o, device), T(d, device), _expected(f"float top icosphere {sub} 64", v, f, o, d), f"icosphere {sub}, node_layout = 0")


# ---- octants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("query", PRUNING)
def test_all_octants_and_tiles_that_straddle_them(device, query):
    """eight cameras on the diagonals (every wave in one octant, each octant's table), one on an axis (tiles of mixed
    octants fail the entry test and take the phase)"""
    v, f = W.icosphere(4)
    r = _make(v, f, device)
    cams = [(sx * 1.5, sy * 1.5, sz * 1.5) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)] + [(2.5, 0.0, 0.0)]
    for at in cams:
        o, d = _camera(at)
        if 0.0 not in at:
            assert (np.sign(d) == -np.sign(np.float32(at))).all(), "a diagonal camera with rays of another octant"
        both(r, query, T(o, device), T(d, device), _expected(f"float top camera {at}", v, f, o, d), f"camera at {at}, {query}")


@pytest.mark.parametrize("query", PRUNING)
def test_axis_parallel_rays_and_negative_zeros(device, query):
    v, f = W.icosphere(4)
    r = _make(v, f, device)
    g = (np.arange(64, dtype=np.float32) + np.float32(0.5)) / np.float32(32) - np.float32(1)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    k = np.arange(64 * 64).reshape(8, 8, 8, 8).transpose(0, 2, 1, 3).reshape(-1)      # 8 x 8 tiles: a wave sees one patch
    xy = xy[k]
    for axis in range(3):
        for sign in (1.0, -1.0):
            for zeros in (0.0, -0.0):
                d = np.full((len(xy), 3), zeros, np.float32)
                d[:, axis] = -sign
                o = np.zeros((len(xy), 3), np.float32)
                o[:, axis] = 3.0 * sign
                o[:, [a for a in range(3) if a != axis]] = xy
                what = f"rays along axis {axis}, from {sign:+.0f}, other components {zeros!r}"
                both(r, query, T(o, device), T(d, device), _expected("float top " + what, v, f, o, d), f"{what}, {query}")


# ---- partial waves, thresholds, the other instantiations -------------------------------------------------------------------
@pytest.mark.parametrize("query", PRUNING)
@pytest.mark.parametrize("n", [64, 65, 127])
def test_partial_waves(device, n, query):
    v, f = W.icosphere(5)
    o, d = _image(64, 64)
    s = 64 * 30 + 20                      # a stretch of the image that crosses the silhouette
    o, d = o[s:s + n], d[s:s + n]
    both(_make(v, f, device), query, T(o, device), T(d, device), _expected(f"float top {n} rays", v, f, o, d), f"{n} rays, {query}")


@pytest.mark.parametrize("query", PRUNING)
@pytest.mark.parametrize("steal", [2, 4, 5, 64, 1])
def test_give_away_thresholds(device, steal, query):
    v, f = W.icosphere(5)
    o, d = _image(64, 64)
    exp = _expected("float top icosphere 5 64", v, f, o, d)
    ot, dt = T(o, device), T(d, device)
    with options(steal=steal):
        r = _make(v, f, device)
        got = run_query(r, query, ot, dt)
        check_query(query, got, exp, f"steal = {steal}, {query}")
        _expect_stealing_grid_launch(r, query, f"steal = {steal}, {query}")
    with options(steal=steal), no_table(r):
        got0 = run_query(r, query, ot, dt)
        check_query(query, got0, exp, f"steal = {steal}, {query}, float_top = 0")
    assert _bytes(got0) == _bytes(got), f"steal = {steal}, {query}: float_top = 0 and 1 differ"


@pytest.mark.parametrize("query", PRUNING)
def test_generic_addressing(device, query):
    """compact = 0: the stealing launch in 64-bit addressing walks the exact nodes and has no loop to hand the table to"""
    v, f = W.icosphere(5)
    o, d = _image(64, 64)
    exp = _expected("float top icosphere 5 64", v, f, o, d)
    ot, dt = T(o, device), T(d, device)
    r = _make(v, f, device)
    out = {}
    for ft in (1, 0):
        with options(compact=0):
            r.as_wrapper.set_float_top(bool(ft))
            out[ft] = run_query(r, query, ot, dt)
            check_query(query, out[ft], exp, f"compact = 0, float_top = {ft}, {query}")
            li = r.as_wrapper.last_launch()
            assert (li["shape"], li["grid_nodes"], li["addressing"]) == (1, 0, 0), li
    assert _bytes(out[0]) == _bytes(out[1])


@pytest.mark.parametrize("query", PRUNING)
def test_the_deep_tree(device, query):
    import hostile_rays as H
    v, f, o, d, _, alone = H.scene("deep", 4096)
    r = _make(v, f, device)
    assert r.bvh_info()["depth"] > 32
    assert_table(r, "deep tree")
    both(r, query, T(o, device), T(d, device), alone, f"deep tree, {query}")
    assert r.as_wrapper.last_launch()["addressing"] == 2


def test_the_instrumented_launch_is_the_same_with_and_without_the_option(device):
    import triro.backend.ops as hops
    v, f = W.icosphere(5)
    o, d = _image(64, 64)
    r = _make(v, f, device)
    ot, dt = T(o, device), T(d, device)
    for query in PRUNING:
        one = hops.trace_stats(r.as_wrapper, ot, dt, query)
        with no_table(r):
            zero = hops.trace_stats(r.as_wrapper, ot, dt, query)
        assert one == zero and one["node_visits"] > 0, (query, one, zero)


# ---- the launch reads the table --------------------------------------------------------------------------------------------
# planes no ray of the image can meet: the x slab collapsed onto the box's minimum, the y slab onto its maximum, the z slab onto
# the middle -- a ray would have to pass through the one point (min x, max y, mid z), which lies outside the camera's view
NO_BOX = np.float32([0, 65535, 0, 65535, 32768, 32768] * 2)


@pytest.mark.parametrize("query", PRUNING)
def test_the_stealing_launch_walks_the_table(device, query):
    """With the root's record made unmeetable every wave that walks the table loses all its hits, while the same handle
    without its table (the generic loop on the grid nodes) answers as before: the launch reads the table, and the switch is
    what takes it away.  A camera on a diagonal: every wave in one octant, so every wave enters the loop."""
    v, f = W.icosphere(4)
    o, d = _camera((1.5, 1.5, 1.5))
    exp = _expected("float top camera (1.5, 1.5, 1.5)", v, f, o, d)
    assert exp["closest"][0].sum() > 1000
    r = _make(v, f, device)
    ot, dt = T(o, device), T(d, device)
    both(r, query, ot, dt, exp, f"before the poke, {query}")
    r.as_wrapper.poke_top(0, NO_BOX)
    got = run_query(r, query, ot, dt)
    _expect_stealing_grid_launch(r, query, f"poked root, {query}")
    hits = {"closest": lambda g: g[0], "first": lambda g: g >= 0, "any": lambda g: g}[query](got)
    assert int(hits.sum()) == 0, f"{query}: {int(hits.sum())} rays still hit: the launch did not walk the table"
    with no_table(r):
        check_query(query, run_query(r, query, ot, dt), exp, f"poked root, float_top = 0, {query}")
    r.refit(T(v, device))      # writes the table anew
    assert_table(r, "after the refit that follows the poke")
    both(r, query, ot, dt, exp, f"after the refit, {query}")


# ---- the table's life ------------------------------------------------------------------------------------------------------
def _moved(v):
    w = v.copy()
    w[:, 2] *= (np.float32(1.0) + np.float32(0.35) * w[:, 0])
    w[:, 1] += np.float32(0.2) * w[:, 0] * w[:, 0]
    return w.astype(np.float32)


def _arena_bytes(nf):
    """the arena of `nf` triangles: nodes | links | tris | grid nodes, each from a multiple of 256 bytes on"""
    nn, off = max(nf - 1, 1), 0
    for size in (64 * nn, 8 * nn, 48 * nf, 32 * nn):
        off = (off + 255) // 256 * 256 + size
    return (off + 255) // 256 * 256


def test_the_table_follows_the_handle_through_its_life(device, tmp_path):
    import torch
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(4)
    v2 = _moved(v)
    o, d = _image(64, 64, distance=3.0)
    ot, dt = T(o, device), T(d, device)
    exp1, exp2 = _expected("float top life 1", v, f, o, d), _expected("float top life 2", v2, f, o, d)
    assert not np.array_equal(exp1["closest"][3], exp2["closest"][3])
    r = _make(v, f, device)
    assert_table(r, "after the build")
    before = r.as_wrapper.download_top()
    both(r, "closest", ot, dt, exp1, "after the build")
    # a launch captured now must find the refitted table where it found this one
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        check_query("closest", run_query(r, "closest", ot, dt), exp1, "eager on the side stream")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run_query(r, "closest", ot, dt)
    graph.replay()
    torch.cuda.synchronize()
    poison.assert_written(*out, what="replay before the refit")
    check_query("closest", out, exp1, "replay before the refit")
    r.refit(T(v2, device))
    assert_table(r, "after the refit")
    assert r.as_wrapper.download_top().tobytes() != before.tobytes(), "the refit left the table as it was"
    both(r, "closest", ot, dt, exp2, "after the refit")
    graph.replay()
    torch.cuda.synchronize()
    check_query("closest", out, exp2, "replay after the refit")
    # save / load: the table is not in the blob
    blob = r.as_wrapper.serialize()
    assert len(blob) == 80 + _arena_bytes(len(f)), "the serialised size changed"
    path = str(tmp_path / "life.npz")
    r.save(path)
    loaded = RayMeshIntersector.load(path, device)
    assert_table(loaded, "after the load")
    both(loaded, "closest", ot, dt, exp2, "after the load")
    # a rebuild to a mesh of another size (a larger arena), then to one without a hierarchy, then back
    v3, f3 = W.icosphere(5)
    r.update_raw(T(v3, device), T(f3, device))
    assert_table(r, "after update_raw to a larger mesh")
    both(r, "closest", ot, dt, _expected("float top life 3", v3, f3, o, d), "after update_raw to a larger mesh")
    v1, f1 = _mesh("1 triangle")
    r.update_raw(T(v1, device), T(f1, device))
    assert_table(r, "after update_raw to one triangle")
    both(r, "closest", ot, dt, _expected("float top life 4", v1, f1, o, d), "after update_raw to one triangle", stealing=False)
    r.update_raw(T(v, device), T(f, device))
    assert_table(r, "after update_raw back")
    both(r, "closest", ot, dt, exp1, "after update_raw back")
