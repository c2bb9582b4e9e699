"""Every query, the builder, refit and persistence on meshes with NaN, infinite and far-away vertices
(tests/hostile_meshes.py builds them; tests/test_hostile_meshes_cpu.py checks the same on the oracle and on the host build
of the product headers).

What a gfx950 build and an x86 build of the same headers are most likely to part on, and what these meshes reach: the
fminf / fmaxf chains of k_tri_bounds, k_refit_round and k_refit_nodes_round with NaN operands, the ordered-uint atomics on
encoded NaN and Inf bounds, tr_qframe_make on an infinite extent, tr_qfloor / tr_qceil on NaN, Morton keys that all
collapse to one value, slab tests on boxes with infinite and NaN planes, the predicate on NaN and Inf vertices.

The ground truth is the oracle's BRUTE FORCE (mode 0: no hierarchy, no box), whose BVH mode is shown to agree with it on
these meshes by the CPU module.  Rules that need no oracle (hostile_meshes.check_rules): no output names a face with a
non-finite coordinate, no hit carries a non-finite float, and on the rays that both meshes anchor alike every output
equals the same query on active_faces(mesh), ids mapped, bit for bit."""
import numpy as np
import pytest

import bvh_checks as K
import hostile_meshes as M
import poison
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import ADDRESSING, QUERIES, SHAPES, check_query, expect_launch, run_query

pytestmark = pytest.mark.gpu

SCENES_OF = {"compact": M.FAMILIES, "deep": ("deep_nan",), "generic": M.FAMILIES + ("deep_nan",)}
SEED = 0                # of the families in everything but the builder, which takes all three
# The matrix runs every batch five times over in one launch: a launch learns an order, and a later one carries its sort,
# only from 64 blocks on (csrc/launch_policy.inc, sched_acquire), which 3 500 rays do not fill.
REPS = 5
FLAVOURS = [(q, a, s) for q in QUERIES for a in ADDRESSING for s in SHAPES if q in SHAPES[s][1] and a in SHAPES[s][2]]
DEFAULT_DIRECTION = np.array([0.4395064455, 0.617598629942, 0.652231566745], np.float32)
RETRY = np.array([0.21, -0.43, 0.37], np.float32)


def T(x, dev):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to(dev)           # (a copy: the shared cases are read-only)


def make(v, f, dev):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, dev), faces=T(f, dev))


def host(got):
    return tuple(g.cpu().numpy() for g in got) if isinstance(got, (tuple, list)) else got.cpu().numpy()


def seed_of(name):
    return SEED if name in M.FAMILIES or name == "deep_nan" else None


def expected(name, seed):
    """the brute force's results in the form check_query takes"""
    e = M.oracle(name, seed, 0)
    return {"closest": e["closest"], "count": e["count"], "location": e["location"]}


def all_queries_match(r, ra, name, seed, dev, what):
    """any, first, closest, count and location of intersector r on the case's rays: the brute force's bits, and the rules
    against the same queries of `ra`, an intersector on active_faces(mesh) (None: the mesh has no active face)"""
    c, exp, keep = M.case(name, seed), expected(name, seed), M.same_anchor(name, seed)
    ot, dt = T(c.o, dev), T(c.d, dev)
    for query in QUERIES:
        got = run_query(r, query, ot, dt)
        check_query(query, got, exp, f"{what}: {query}")
        if ra is not None:
            M.check_rules(c, query, host(got), host(run_query(ra, query, ot, dt)), keep, f"{what}: {query}")
        elif query == "count":
            assert not host(got).any(), f"{what}: a mesh without an active face is hit"


def closest_point(r, p, dev, **kw):
    """hops.closest_point_native, synchronised, every output checked for elements never written -> numpy"""
    import torch
    import triro.backend.ops as hops
    res = hops.closest_point_native(r.as_wrapper, T(np.ascontiguousarray(p, np.float32).reshape(-1, 3), dev), **kw)
    torch.cuda.synchronize()
    poison.assert_written(*res, what="closest_point_native (closest, distance, tri)")
    return tuple(x.cpu().numpy() for x in res)


# ---- the flavour matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("query,addressing,shape", FLAVOURS, ids=["-".join(x) for x in FLAVOURS])
def test_flavour_on_hostile_meshes(device, query, addressing, shape):
    import torch
    opts = SHAPES[shape][0]
    streaming = shape.startswith("stream")

    def record(r, what, carried=0):
        if streaming:
            with pytest.raises(ValueError, match="no direct launch"):
                r.as_wrapper.last_launch()
            return None
        li = expect_launch(r, query, shape, addressing, what)
        assert carried is None or li["sort_carried"] == carried, f"{what}: {li}"
        return li

    for name in SCENES_OF[addressing]:
        c, keep = M.case(name, SEED), M.same_anchor(name, SEED)
        exp = M.tiled(expected(name, SEED), REPS, len(c.o))
        fa, _ = M.active_faces(c.v, c.f)
        what = f"{query} / {addressing} / {shape} / {c.name}"
        with options(compact=0 if addressing == "generic" else 1, **opts):
            r = make(c.v, c.f, device)
            depth = r.bvh_info()["depth"]
            assert depth > 32 if addressing == "deep" else (depth <= 32 or addressing == "generic"), (name, depth)
            ot, dt = T(np.tile(c.o, (REPS, 1)), device), T(np.tile(c.d, (REPS, 1)), device)
            alone = host(run_query(make(c.v, fa, device), query, ot, dt))      # the active faces alone, in the same flavour

            def check(got, label):
                check_query(query, got, exp, label)
                M.check_rules(c, query, host(got), alone, keep, label, reps=REPS)

            if shape == "sort_carried":
                for k in range(16):
                    check(run_query(r, query, ot, dt), f"{what} launch {k}")
                    if record(r, f"{what} launch {k}", carried=None)["sort_carried"]:
                        break
                else:
                    raise AssertionError(f"{what}: no launch of 16 carried the sort")
                continue
            for k in range(2):                    # the second launch runs on the learned order
                check(run_query(r, query, ot, dt), f"{what} launch {k}")
                record(r, f"{what} launch {k}")
            torch.cuda.synchronize()


# ---- the builder --------------------------------------------------------------------------------------------------------
def download(r):
    nodes, links, tris = r.as_wrapper.download()
    qnodes, frame = r.as_wrapper.download_qnodes()
    return nodes, links, tris, qnodes, frame


def assert_same_arrays(got, want, what, canon=True):
    """the five arrays byte for byte; canon: every NaN of a float word equal to every NaN (bvh_checks.canon_arrays)"""
    if canon:
        got, want = K.canon_arrays(*got), K.canon_arrays(*want)
    for name, g, w in zip(("nodes", "links", "tris", "qnodes", "frame"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        gb, wb = np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)
        assert np.array_equal(gb, wb), f"{what}: {name} differs in {int(np.sum(np.any((gb != wb).reshape(max(len(g), 1), -1), axis=1)))} rows"


@pytest.mark.parametrize("name,seed", M.ALL_CASES, ids=M.CASE_IDS)
def test_builder_on_hostile_meshes(device, name, seed):
    """the five arrays, depth and key mode of the GPU builder == the host construction, byte for byte with NaN made
    canonical; the NaN-aware check_structure passes; closest and count answer as the brute force"""
    from sim import SimBVH
    c = M.case(name, seed)
    r = make(c.v, c.f, device)
    got, info = download(r), r.bvh_info()
    assert info["num_tris"] == len(c.f) and info["num_nodes"] == max(len(c.f) - 1, 0)
    H = SimBVH(c.v, c.f)
    K.check_structure(c.v, c.f, *got, info, ref_frame=H.frame)
    assert_same_arrays(got, (H.nodes, H.links, H.tris, H.qnodes, H.frame), f"{c.name}: GPU against the host construction")
    assert info["depth"] == H.depth and info["key_mode"] == H.key_mode, (info["depth"], H.depth, info["key_mode"], H.key_mode)
    exp = expected(name, seed)
    ot, dt = T(c.o, device), T(c.d, device)
    check_query("closest", r.intersects_closest(ot, dt), exp, c.name)
    check_query("count", r.intersects_count(ot, dt), exp, c.name)


# ---- refit --------------------------------------------------------------------------------------------------------------
def test_refit_through_hostile_vertices_and_back(device):
    """clean -> non-finite -> far away -> clean, the same faces: after every step all five queries answer as the brute
    force of that step's vertices and the arrays pass check_structure; after the last the arrays are those of the build
    and of a fresh handle refitted to the clean vertices, byte for byte -- nothing a NaN or an Inf touched may stick"""
    from oracle.oracle import OracleIntersector
    from sim import SimBVH
    from test_gpu_builder_matrix import assert_all_queries
    f, steps = M.refit_sequence()
    clean = steps[0][1]
    o, d = M.rays(clean, f, np.zeros(len(f), bool), 5, far=0)
    r = make(clean, f, device)
    built, info = download(r), r.bvh_info()
    order = built[2][:, K.FACE].view(np.int32).copy()
    for label, v in steps:
        r.refit(T(v, device))
        got = download(r)
        K.check_structure(v, f, *got, r.bvh_info(), ref_frame=SimBVH(v, f).frame, order=order)
        assert r.bvh_info()["depth"] == info["depth"]
        R = OracleIntersector(v, f, 0)
        assert R.closest_raw(o, d)[0].sum() >= 1000
        assert_all_queries(r, R, o, d, device, f"refit to the {label} vertices")
        tri = r.intersects_first(T(o, device), T(d, device)).cpu().numpy()
        assert np.isfinite(v[f[tri[tri >= 0]]]).all(), f"refit to the {label} vertices: an inactive face is hit"
    fresh = make(clean, f, device)
    fresh.refit(T(clean, device))
    assert_same_arrays(download(r), download(fresh), "back to the clean vertices against a fresh refit", canon=False)
    assert_same_arrays(download(r), built, "back to the clean vertices against the build", canon=False)
    assert r.bvh_info()["aabb_min"] == info["aabb_min"] and r.bvh_info()["aabb_max"] == info["aabb_max"]


# ---- persistence --------------------------------------------------------------------------------------------------------
def test_save_load_and_update_raw_with_a_hostile_mesh(device, tmp_path):
    from triro.ray.ray_optix import RayMeshIntersector
    name = "faraway_nonfinite"
    c = M.case(name, SEED)
    fa, _ = M.active_faces(c.v, c.f)
    ra = make(c.v, fa, device)
    r = make(c.v, c.f, device)
    path = str(tmp_path / "hostile.npz")
    r.save(path)
    rl = RayMeshIntersector.load(path, device=device)
    assert_same_arrays(download(rl), download(r), "loaded hostile handle", canon=False)          # (bytes copied: the same NaNs)
    for key in ("depth", "key_mode", "num_tris"):
        assert rl.bvh_info()[key] == r.bvh_info()[key], key
    assert np.array_equal(K.canon_bits(np.float32(rl.bvh_info()["aabb_min"] + rl.bvh_info()["aabb_max"])),
                          K.canon_bits(np.float32(r.bvh_info()["aabb_min"] + r.bvh_info()["aabb_max"])))
    all_queries_match(rl, ra, name, SEED, device, "loaded hostile handle")
    # hostile -> clean -> hostile inside one handle
    clean = M.case("unreferenced_nan_vertex")
    r.update_raw(T(clean.v, device), T(clean.f, device))
    assert_same_arrays(download(r), download(make(clean.v, clean.f, device)), "hostile handle rebuilt with a clean mesh", canon=False)
    all_queries_match(r, make(clean.v, clean.f, device), "unreferenced_nan_vertex", None, device, "hostile handle rebuilt with a clean mesh")
    r.update_raw(T(c.v, device), T(c.f, device))
    assert_same_arrays(download(r), download(make(c.v, c.f, device)), "clean handle rebuilt with the hostile mesh")
    all_queries_match(r, ra, name, SEED, device, "clean handle rebuilt with the hostile mesh")


# ---- proximity ----------------------------------------------------------------------------------------------------------
PROXIMITY = [(n, seed_of(n)) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", PROXIMITY, ids=[n for n, _ in PROXIMITY])
def test_closest_point_skips_inactive_triangles(device, name, seed):
    """closest_point at stack limits 0 (all), 1, 2, 3 == the brute force over the active triangles (tests/host_sim), bit for
    bit; the rules against the active faces alone; a mesh without an active face answers (-1, +Inf, NaN)"""
    import nearest_cases as NC
    import nearest_sim
    c = M.case(name, seed)
    fa, _ = M.active_faces(c.v, c.f)
    want = nearest_sim.brute(c.v, c.f, c.p)
    r = make(c.v, c.f, device)
    for entries in (0, 1, 2, 3):
        got = closest_point(r, c.p, device, stack_entries=entries)
        NC.assert_same_bits(got, want, f"{c.name}, stack_entries {entries}")
        M.check_nearest_rules(c, got, nearest_sim.brute(c.v, fa, c.p), f"{c.name}, stack_entries {entries}")
    if len(fa):
        alone = closest_point(make(c.v, fa, device), c.p, device)
        M.check_nearest_rules(c, got, alone, f"{c.name}: against the GPU's own answer on the active faces")
    else:
        assert (got[2] == -1).all() and np.isposinf(got[1]).all() and np.isnan(got[0]).all()
    # signed_distance: the magnitude is closest_point's distance, whatever contains_points makes of the mesh's box
    sd = r.signed_distance(T(c.p, device)).cpu().numpy()
    assert np.array_equal(K.canon_bits(np.abs(sd)), K.canon_bits(want[1])), f"{c.name}: |signed_distance|"


# ---- contains_points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nonfinite", "faraway", "holed_sphere"])
def test_contains_points_on_hostile_meshes(device, name):
    """the native launch with an explicit finite box: counts of both rays, inside and broken against the brute force, as
    tests/test_gpu_contains.py compares; the public method against OracleIntersector.contains_points (a NaN vertex makes the
    box NaN and every point False, as in the reference)"""
    import torch
    import triro.backend.ops as hops
    from oracle.oracle import OracleIntersector
    from test_gpu_contains import decision
    seed = seed_of(name)
    c = M.case(name, seed)
    R = OracleIntersector(c.v, c.f, 0)
    r = make(c.v, c.f, device)
    n = len(c.p)
    pt = T(c.p, device)
    box = (np.float32([-1.25] * 3), np.float32([1.25] * 3))
    for d in (DEFAULT_DIRECTION, np.array([-0.3, 0.2, 0.9], np.float32)):
        res = hops.contains_points_native(r.as_wrapper, pt, T(d, device), T(box[0], device), T(box[1], device), want_counts=True)
        torch.cuda.synchronize()
        poison.assert_written(*res, what="contains_points_native (inside, broken, counts, summary)")
        inside, broken, counts, summary = (x.cpu().numpy() for x in res)
        dirs = np.tile(d, (n, 1)).astype(np.float32)
        cp, cm = R.intersects_count(c.p, dirs), R.intersects_count(c.p, -dirs)
        in_box, want_inside, want_broken = decision(c.p, box, cp, cm)
        assert np.array_equal(counts, np.stack([cp, cm])), f"{c.name}: counts differ from the brute force"
        assert np.array_equal(inside, want_inside) and np.array_equal(broken, want_broken), f"{c.name}: inside / broken"
        assert summary.tolist() == [int(in_box.sum()), int(want_broken.sum())], f"{c.name}: summary"
        assert 0 < in_box.sum() < n and (name == "holed_sphere" or 0.1 < want_inside[in_box].mean() < 0.9)
        # the public method, explicit direction and default direction with a fixed retry
        assert np.array_equal(r.contains_points(pt, T(d, device)).cpu().numpy(), R.contains_points(c.p, d)), f"{c.name}: explicit direction"
    got = r.contains_points(pt, None, _retry_direction=torch.from_numpy(RETRY)).cpu().numpy()
    want = R.contains_points(c.p, None, _retry_dirs=iter([RETRY] * 4))
    assert np.array_equal(got, want), f"{c.name}: default direction"
    assert want.any() == (name == "faraway"), "a NaN vertex makes every point False; far-away vertices only widen the box"


# ---- record forms -------------------------------------------------------------------------------------------------------
def test_record_forms_on_a_hostile_mesh(device):
    """packed records in face and slot form and bare slots on `nonfinite`, expanded with and without row_length: the dense
    call's bits, which are the brute force's; no record names an inactive face"""
    import torch
    c, exp = M.case("nonfinite", SEED), expected("nonfinite", SEED)
    r = make(c.v, c.f, device)
    order = download(r)[2][:, K.FACE].view(np.int32)
    for m, width in ((3488, 16), (2048, 32)):
        assert m % width == 0 and m <= len(c.o)
        ot, dt = T(c.o[:m], device), T(c.d[:m], device)
        dense = r.intersects_closest(ot, dt)
        for key, g, e in zip(("hit", "front", "tri", "loc", "uv"), dense, exp["closest"]):
            assert np.array_equal(g.cpu().numpy(), e[:m]), f"{m} rays: closest {key} against the brute force"
        rec_f, rec_s = r.intersects_closest_packed(ot, dt), r.intersects_closest_packed(ot, dt, slots=True)
        slot = r.intersects_closest_slots(ot, dt)
        miss = ~dense[0]
        assert bool((slot[miss] == -1).all()) and bool((rec_f[miss][:, 0] < 0).all()) and bool((rec_s[miss][:, 0] < 0).all())
        s = slot.cpu().numpy()
        assert np.array_equal(order[s[s >= 0]], exp["closest"][2][:m][s >= 0]) and not c.inactive[order[s[s >= 0]]].any()
        forms = {"faces": r.closest_expand(rec_f), "slot records": r.closest_expand(rec_s, slots=True),
                 "slot records in rows": r.closest_expand(rec_s, slots=True, row_length=width),
                 "slots": r.closest_from_slots(ot, dt, slot), "slots in rows": r.closest_from_slots(ot, dt, slot, row_length=width)}
        for form, got in forms.items():
            for key, a, e in zip(("hit", "front", "tri", "loc", "uv"), got, dense):
                assert torch.equal(a, e), f"{m} rays, {form}: {key} differs from the dense call"


# ---- the rest -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.SINGLE)
def test_single_cases_answer_as_the_brute_force(device, name):
    """the all-NaN triangle, the unreferenced NaN vertex, the holed sphere, the mesh without an active face, one and two
    triangles with a non-finite vertex (no hierarchy), the denormal sphere: all five queries"""
    c = M.case(name)
    fa, _ = M.active_faces(c.v, c.f)
    r = make(c.v, c.f, device)
    ra = make(c.v, fa, device) if len(fa) else None
    all_queries_match(r, ra, name, None, device, name)
    if name == "unreferenced_nan_vertex":
        import workloads as W
        v, f = W.icosphere(2)
        plain = make(v, f, device)
        ot, dt = T(c.o, device), T(c.d, device)
        for query in QUERIES:
            a, b = host(run_query(r, query, ot, dt)), host(run_query(plain, query, ot, dt))
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert M._same(x, y), f"{query}: a vertex that no face references changes an answer"
