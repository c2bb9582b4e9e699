"""The GPU builder and refit (csrc/bvh_build.hip), checked structurally at every size edge.

Query answers cannot judge a builder: a hierarchy whose boxes are too large, whose sort is not stable or whose nodes lie
in another order still answers every ray.  Every case here therefore downloads the arrays the builder wrote and
  (i)   holds them to the numpy references of tests/bvh_checks.py (check_structure: triangle order of a stable sort,
        records, leaf boxes bit for bit, check_tree's topology / nesting / grid nodes, height, bounds, frame),
  (ii)  compares all five arrays, depth and key mode with the host construction (tests/host_sim) byte for byte,
  (iii) compares closest-hit and count answers on a few thousand rays with the oracle bit for bit, so that no case passes
        on arrays alone.
tests/test_builder_reference.py shows, without a GPU, that references and host construction agree on every input used
here and that check_structure rejects a tree that is wrong by one float spacing or one exchanged pair of records.

Edges of bvh_build.hip and the test that crosses each:
  nf == 1, nf == 2; one wave / one block of k_karras, k_emit, k_gather; the radix sort's tile of 1024 keys and workgroup
  of 4096 keys; the grid cap of k_tri_bounds (262 144 triangles); the second trip of k_rs_scan's tile loop
  (1 048 577)                                                   test_size_ladder
  stability of the scatter across tiles and workgroups          test_equal_keys_keep_their_input_order
  degenerate and extreme frames                                 test_degenerate_frames
  refit-round guess too small, heights 64 and 65                test_height_boundaries
  rebuild into a used handle, build_cache on and off            test_rebuild_into_a_used_handle
  node_layout = 0 (k_emit without positions)                    test_node_layout_0
  refit: k_regather, k_refit_nodes_round, k_qframe_box,
  k_update_boxes                                                test_refit_structure, test_refit_of_loaded_saved_and_layout_0_handles
  bad face beyond the grid cap of k_tri_bounds                  test_bad_face_beyond_the_grid_cap"""
import numpy as np
import pytest
import torch

import bvh_checks as K
import sim
import workloads as W
from launch_options import options
from oracle.oracle import OracleIntersector
from sim import SimBVH
from test_builder_reference import copies_of_one_triangle, named_mesh, same_tree_under_a_permutation
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)

pytestmark = pytest.mark.gpu

ARRAYS = ("nodes", "links", "tris", "qnodes", "frame")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def make(v, f, dev):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, dev), faces=T(f, dev))


def download(r):
    nodes, links, tris = r.as_wrapper.download()
    qnodes, frame = r.as_wrapper.download_qnodes()
    return nodes, links, tris, qnodes, frame


def host(v, f, layout=1):
    sim.use_node_layout(layout)
    try:
        return SimBVH(v, f)
    finally:
        sim.use_node_layout(1)


def assert_same_arrays(got, want, what):
    for name, g, w in zip(ARRAYS, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        gb, wb = np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)
        assert np.array_equal(gb, wb), f"{what}: {name} differs in {int(np.sum(np.any((gb != wb).reshape(len(g), -1), axis=1)))} rows"


def probe_rays(v, f, n, seed):
    """n rays around the mesh: half with hashed directions, half aimed at triangle centroids (so that tiny triangles
    in a large box are hit, too)"""
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    c, e = (lo + hi) / 2, max(float((hi - lo).max()), 1e-30) * 0.75
    o, d = W.hash_rays(n, seed, (c - e).astype(np.float32), (c + e).astype(np.float32))
    pick = (np.arange(n // 2, dtype=np.int64) * 7919) % len(f)
    cen = ((v[f[pick, 0]] + v[f[pick, 1]]) + v[f[pick, 2]]) * np.float32(1.0 / 3.0)
    d[n // 2:] = (cen - o[n // 2:]).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def assert_answers(r, v, f, dev, what, n=3000, seed=3, R=None):
    """closest and count on probe rays == the oracle, bit for bit"""
    R = R if R is not None else OracleIntersector(v, f, 1)
    o, d = probe_rays(v, f, n, seed)
    ot, dt = T(o, dev), T(d, dev)
    got = r.intersects_closest(ot, dt)
    exp = R.closest_raw(o, d)
    for name, g, e in zip(("hit", "front", "tri", "loc", "uv"), got, exp):
        g = g.cpu().numpy()
        assert g.shape == e.shape and np.array_equal(g, e), f"{what}: closest {name} differs from the oracle"
    assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), R.intersects_count(o, d)), f"{what}: count"
    return R


def assert_all_queries(r, R, o, d, dev, what):
    """any, first, closest, count and location == the oracle, bit for bit"""
    o, d = np.ascontiguousarray(o).reshape(-1, 3), np.ascontiguousarray(d).reshape(-1, 3)
    ot, dt = T(o, dev), T(d, dev)
    exp = R.closest_raw(o, d)
    for name, g, e in zip(("hit", "front", "tri", "loc", "uv"), r.intersects_closest(ot, dt), exp):
        assert np.array_equal(g.cpu().numpy(), e), f"{what}: closest {name}"
    cnt = R.intersects_count(o, d)
    assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), cnt), f"{what}: count"
    assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy(), cnt > 0), f"{what}: any"
    assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy(), exp[2]), f"{what}: first"
    for name, g, e in zip(("loc", "ray", "tri"), r.intersects_location(ot, dt), R.intersects_location(o, d)):
        g = g.cpu().numpy()
        assert g.shape == e.shape and np.array_equal(g, e), f"{what}: location {name}"


def build_and_check(v, f, dev, what, layout=1, rays=3000, key_mode=None, depth=None):
    """(i), (ii), (iii) of the module docstring for one mesh; returns (intersector, host tree, downloaded arrays)"""
    r = make(v, f, dev)
    got, info = download(r), r.bvh_info()
    assert info["num_tris"] == len(f) and info["num_nodes"] == max(len(f) - 1, 0), what
    H = host(v, f, layout)
    K.check_structure(v, f, *got, info, ref_frame=H.frame)
    assert_same_arrays(got, (H.nodes, H.links, H.tris, H.qnodes, H.frame), what + ": GPU vs host construction")
    assert info["depth"] == H.depth and info["key_mode"] == H.key_mode, (what, info["depth"], H.depth, info["key_mode"], H.key_mode)
    if key_mode is not None:
        assert info["key_mode"] == key_mode, what
    if depth is not None:
        assert info["depth"] == depth, what
    assert_answers(r, v, f, dev, what, n=rays)
    return r, H, got


# ---- sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                               262143, 262144, 262145, 1048576, 1049601])
def test_size_ladder(device, n):
    v, f = W.random_soup(n, seed=n)
    r, H, got = build_and_check(v, f, device, f"soup {n}", key_mode=0)
    if n == 1:
        assert len(got[0]) == 0 and len(got[1]) == 0 and len(got[3]) == 0 and r.bvh_info()["depth"] == 0
        assert np.array_equal(got[2], K.tri_records(v, f, [0]))


# ---- equal keys -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["copies1025", "copies4097", "copies10000", "sphere_x4", "soup_x3"])
def test_equal_keys_keep_their_input_order(device, name):
    """a radix sort is stable only if every pass keeps equal digits in order ACROSS tiles (1024 keys) and workgroups
    (4096 keys): runs of equal keys longer than both, and equal keys that start 5000 and 10 000 face ids apart"""
    v, f = copies_of_one_triangle(int(name[6:])) if name.startswith("copies") else named_mesh(name)
    r, H, got = build_and_check(v, f, device, name, key_mode=0)
    order = got[2][:, K.FACE].view(np.int32)
    keys = K.morton_keys(v, f)
    if name.startswith("copies"):
        assert len(np.unique(keys)) == 1 and np.array_equal(order, np.arange(len(f)))
    else:
        reps = 4 if name == "sphere_x4" else 3
        n0 = len(f) // reps
        # every key occurs a multiple of `reps` times; within a run of equal keys the face ids ascend, and the copies
        # of one triangle (ids n0 apart) are all in that run
        same = keys[order][1:] == keys[order][:-1]
        assert np.all(order[1:][same] > order[:-1][same])
        _, counts = np.unique(keys, return_counts=True)
        assert np.all(counts % reps == 0) and len(f) == (20480 if name == "sphere_x4" else 15000)
        assert np.array_equal(keys[:n0], keys[n0:2 * n0])


# ---- frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat", "line", "huge", "tiny", "far"])
def test_degenerate_frames(device, name):
    """an axis of zero extent (two of them), coordinates x 3e12 and x 1e-12 + 1e-9, a small mesh far from the origin:
    keys with a zero extent, frames whose scale is clamped or far below the float spacing of the coordinates"""
    v, f = named_mesh(name)
    build_and_check(v, f, device, name, key_mode=0)


# ---- heights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reps,key_mode,depth", [(5, 0, 64), (8, 1, 36), (4000, 1, None)])
def test_height_boundaries(device, reps, key_mode, depth):
    """deep_tree_mesh(5): 68 triangles, height 64 with plain keys -- kept; the first guess of the refit rounds is
    log2(68) + 10 = 17, so six more batches of eight rounds follow, k_emit runs after each and skips the nodes the layout
    has not reached, and the layout continues on the caller's stream.  deep_tree_mesh(8): height 65 -> rebuilt with
    depth-bounded keys.  deep_tree_mesh(4000): far beyond."""
    v, f = W.deep_tree_mesh(reps)
    r, H, got = build_and_check(v, f, device, f"deep_tree_mesh({reps})", key_mode=key_mode, depth=depth)
    assert r.bvh_info()["depth"] <= 64
    # rays down the pile of identical triangles at the origin: `reps` exact ties
    o = np.tile(np.float32([1e-10, 1e-10, 1.0]), (64, 1))
    d = np.tile(np.float32([0, 0, -1]), (64, 1))
    R = OracleIntersector(v, f, 1)
    cnt = r.intersects_count(T(o, device), T(d, device)).cpu().numpy()
    assert np.array_equal(cnt, R.intersects_count(o, d)) and cnt[0] >= reps
    assert np.array_equal(r.intersects_first(T(o, device), T(d, device)).cpu().numpy(), R.intersects_first(o, d))


# ---- rebuild ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build_cache", [1, 0])
def test_rebuild_into_a_used_handle(device, build_cache):
    """update_raw rebuilds inside the handle: the round guess is the previous height + 1 (30 000-soup -> height-64 tree:
    too small; back to a sphere: far too large), the arena shrinks to one triangle and regrows to 262 145, the cached
    temporaries are reused or (build_cache = 0) allocated per build.  After every step the handle holds, byte for byte,
    what a fresh handle builds from the same mesh."""
    steps = [("soup 30000", W.random_soup(30000, seed=30000)), ("deep_tree_mesh(5)", W.deep_tree_mesh(5)),
             ("icosphere(2)", W.icosphere(2)), ("soup 4097", W.random_soup(4097, seed=4097)),
             ("one triangle", W.random_soup(1, seed=1)), ("soup 262145", W.random_soup(262145, seed=262145))]
    with options(build_cache=build_cache):
        r = None
        for what, (v, f) in steps:
            what = f"build_cache {build_cache}, {what}"
            if r is None:
                r = make(v, f, device)
            else:
                r.update_raw(T(v, device), T(f, device))
            fresh = make(v, f, device)
            got, want = download(r), download(fresh)
            assert_same_arrays(got, want, what + ": used vs fresh handle")
            ir, ifr = r.bvh_info(), fresh.bvh_info()
            for key in ("num_tris", "num_nodes", "depth", "key_mode", "aabb_min", "aabb_max"):
                assert ir[key] == ifr[key], (what, key, ir[key], ifr[key])
            assert r.as_wrapper.replica_hash() == fresh.as_wrapper.replica_hash(), what
            K.check_structure(v, f, *got, ir)
            assert_answers(r, v, f, device, what, n=1000)
            del fresh


# ---- node_layout = 0 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup2", "soup65", "soup4097", "soup30000", "deep5"])
def test_node_layout_0(device, name):
    """Karras numbering: k_emit writes node i at i (pos == nullptr).  Same tree as the default layout under one
    permutation of the node ids; the option is read when the tree is built, not when it is queried."""
    v, f = W.random_soup(int(name[4:]), seed=int(name[4:])) if name.startswith("soup") else named_mesh(name)
    R = OracleIntersector(v, f, 1)
    c = (v.min(0).astype(np.float64) + v.max(0)) / 2
    ext = float((v.max(0) - v.min(0)).max())
    po, pd = W.pinhole_grid(96, 96, distance=2.5 * ext, center=tuple(c))
    ho, hd = probe_rays(v, f, 6000, 17)
    with options(node_layout=0):
        r, H0, got = build_and_check(v, f, device, name + " layout 0", layout=0)
        assert_all_queries(r, R, po, pd, device, name + " layout 0, pinhole")
        assert_all_queries(r, R, ho, hd, device, name + " layout 0, hash rays")
    # the option is back to 1: the old handle still holds (and walks) its Karras-numbered arrays ...
    assert_same_arrays(download(r), got, name + ": layout-0 handle after the option was reset")
    assert_all_queries(r, R, po, pd, device, name + " layout 0 handle under node_layout = 1, pinhole")
    assert_all_queries(r, R, ho, hd, device, name + " layout 0 handle under node_layout = 1, hash rays")
    # ... and a new build is in treelet order again: the same tree, renumbered
    r1 = make(v, f, device)
    n1, l1, t1, q1, f1 = download(r1)
    H1 = host(v, f, 1)
    assert_same_arrays((n1, l1, t1, q1, f1), (H1.nodes, H1.links, H1.tris, H1.qnodes, H1.frame), name + " layout 1 again")
    if len(f) >= 2:
        G0 = SimBVH(arrays=got[:3], qarrays=got[3:])
        G1 = SimBVH(arrays=(n1, l1, t1), qarrays=(q1, f1))
        G0.depth = G1.depth = r1.bvh_info()["depth"]
        same_tree_under_a_permutation(G0, G1)


# ---- refit ------------------------------------------------------------------------------------------------------------------
def deformed(v, f, kind, seed=3):
    if kind == "deform":
        c = v.astype(np.float64).mean(0)
        v2 = W.displaced((v - c).astype(np.float32) + np.float32(1e-3), seed=seed, amplitude=0.2) * np.array([1.0, 0.7, 1.3], np.float32) + c
        # every triangle gets a shift of its own where it has vertices of its own (soups, the copies of one triangle)
        if len(v) == 3 * len(f) and np.array_equal(f.ravel(), np.arange(3 * len(f))):
            shift = np.random.default_rng(seed).normal(size=(len(f), 1, 3)) * 0.05 * float((v.max(0) - v.min(0)).max())
            v2 = (v2.reshape(-1, 3, 3) + shift).reshape(-1, 3)
        return v2.astype(np.float32)
    if kind == "shrink":
        return (v * np.float32(0.01)).astype(np.float32)
    assert kind == "flatten"
    v2 = v.copy()
    v2[:, 2] = np.float32(-0.375)
    return v2


def check_refitted(r, v2, f, order, depth, device, what):
    """the refitted arrays, with numpy: the triangle order of the BUILD, the records and leaf boxes of the NEW vertices,
    internal boxes = unions, grid nodes containing the exact boxes and tight to a cell of the NEW frame (check_tree), bounds
    and frame of a fresh build of the new mesh; closest and count == the oracle of the new mesh"""
    got, info = download(r), r.bvh_info()
    assert info["depth"] == depth, what
    fresh = make(v2, f, device)
    fi = fresh.bvh_info()
    assert info["aabb_min"] == fi["aabb_min"] and info["aabb_max"] == fi["aabb_max"], (what, info, fi)
    fresh_frame = fresh.as_wrapper.download_qnodes()[1]
    assert np.array_equal(got[4].view(np.uint32), fresh_frame.view(np.uint32)), what + ": frame of a fresh build"
    K.check_structure(v2, f, *got, info, ref_frame=SimBVH(v2, f).frame, order=order)
    assert_answers(r, v2, f, device, what, n=2000)
    return got


REFIT_MESHES = {
    "icosphere5": lambda: W.icosphere(5),
    "soup4097": lambda: W.random_soup(4097, seed=4097),
    "copies10000": lambda: copies_of_one_triangle(10000),
    "two_triangles": W.two_triangles,
    "one_triangle": lambda: W.random_soup(1, seed=1),
}


@pytest.mark.parametrize("name", list(REFIT_MESHES))
def test_refit_structure(device, name):
    """build, then refit three times in a row -- deformed (the copies of one triangle move apart), shrunk to 1 % (stale
    large boxes would still answer every ray: only the arrays show them), flattened onto a plane -- and back to the
    original vertices, which must give the arrays of the build again"""
    v, f = REFIT_MESHES[name]()
    r = make(v, f, device)
    built, info = download(r), r.bvh_info()
    order = built[2][:, K.FACE].view(np.int32).copy()
    assert np.array_equal(order, K.expected_order(v, f))
    v2 = v
    for kind in ("deform", "shrink", "flatten"):
        v2 = deformed(v2 if kind != "flatten" else v, f, kind)
        r.refit(T(v2, device))
        check_refitted(r, v2, f, order, info["depth"], device, f"{name} refit {kind}")
    r.refit(T(v, device))
    assert_same_arrays(download(r), built, name + ": refit back to the vertices of the build")
    assert r.bvh_info()["aabb_min"] == info["aabb_min"] and r.bvh_info()["aabb_max"] == info["aabb_max"]


def test_refit_of_loaded_saved_and_layout_0_handles(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(5)
    v2, v3 = deformed(v, f, "deform"), deformed(v, f, "shrink")
    r = make(v, f, device)
    order, depth = K.expected_order(v, f), r.bvh_info()["depth"]
    path = str(tmp_path / "built.npz")
    r.save(path)
    # a handle that came from load(): refit it
    rl = RayMeshIntersector.load(path, device=device)
    assert_same_arrays(download(rl), download(r), "loaded handle")
    rl.refit(T(v2, device))
    after = check_refitted(rl, v2, f, order, depth, device, "refit of a loaded handle")
    r.refit(T(v2, device))
    assert_same_arrays(download(r), after, "refit of the built handle vs refit of the loaded one")
    # save() after a refit, load(): byte-identical arrays, the same bounds, and it refits on
    path2 = str(tmp_path / "refitted.npz")
    r.save(path2)
    r2 = RayMeshIntersector.load(path2, device=device)
    assert_same_arrays(download(r2), after, "save after refit, load")
    for key in ("depth", "key_mode", "aabb_min", "aabb_max"):
        assert r2.bvh_info()[key] == r.bvh_info()[key], key
    assert r2.as_wrapper.replica_hash() == r.as_wrapper.replica_hash()
    assert_answers(r2, v2, f, device, "loaded refitted handle", n=2000)
    r2.refit(T(v3, device))
    check_refitted(r2, v3, f, order, depth, device, "refit of a handle loaded from a refitted one")
    # a Karras-numbered tree refits like any other (the refit kernels follow the child ids of the nodes)
    with options(node_layout=0):
        r0 = make(v, f, device)
    r0.refit(T(v2, device))
    got0 = check_refitted(r0, v2, f, order, depth, device, "refit of a node_layout = 0 tree")
    G0 = SimBVH(arrays=got0[:3], qarrays=got0[3:])
    G1 = SimBVH(arrays=after[:3], qarrays=after[3:])
    G0.depth = G1.depth = depth
    same_tree_under_a_permutation(G0, G1)


# ---- malformed input ------------------------------------------------------------------------------------------------------
def test_bad_face_beyond_the_grid_cap(device):
    """k_tri_bounds runs at most 1024 blocks of 256 threads: face 262 144 is the first one a thread meets on its SECOND
    trip of the grid-stride loop.  The error names the smallest bad face, from build and from refit."""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.random_soup(262145, seed=262145)
    bad = f.copy()
    bad[262144, 0] = len(v) + 5
    bad[200000, 1] = -1
    with pytest.raises(ValueError, match=r"face 200000 has a vertex index outside \[0, 786435\)"):
        RayMeshIntersector(vertices=T(v, device), faces=T(bad, device))
    bad2 = f.copy()
    bad2[262144, 2] = len(v)
    with pytest.raises(ValueError, match=r"face 262144 has a vertex index outside"):
        RayMeshIntersector(vertices=T(v, device), faces=T(bad2, device))
    r = make(v, f, device)
    with pytest.raises(ValueError, match=r"face 200000 has a vertex index outside"):
        r.as_wrapper.refit(T(v, device), T(bad, device))
    # a failed refit drops the hierarchy; the handle rebuilds
    r.update_raw(T(v, device), T(f, device))
    got, info = download(r), r.bvh_info()
    K.check_structure(v, f, *got, info)
    assert_answers(r, v, f, device, "rebuilt after a failed refit", n=1000)


def test_load_that_fails_after_the_arena_exists(device):
    """a blob whose header claims 256 arena bytes fewer than 80 triangles use (the buffer is as long as it was) passes the
    header checks and is refused once the new handle owns an arena on the device: the one load failure that has device
    memory to give back.  The library loads the untouched blob afterwards as if nothing had happened."""
    from triro.ray.ray_optix import OptixAccelStructureWrapper
    v, f = W.icosphere(1)
    r = make(v, f, device)
    built = download(r)
    blob = r.as_wrapper.serialize()
    bad = blob.copy()
    arena_bytes = bad[24:32].view(np.int64)      # magic[8] | num_tris | num_nodes | arena_bytes
    assert arena_bytes[0] == len(blob) - 80
    arena_bytes[0] -= 256
    w = OptixAccelStructureWrapper()
    with pytest.raises(ValueError, match="arena size mismatch"):
        w.deserialize(bad, device)
    fresh = OptixAccelStructureWrapper()
    fresh.deserialize(blob, device)
    loaded = fresh.download() + fresh.download_qnodes()
    assert_same_arrays(loaded, built, "loaded after a failed load")
