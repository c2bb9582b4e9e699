"""CPU checks of libtriro_tris.so (include/triro_tris.h, csrc/tris.hip, csrc/tr_tris.h): the library is built and exports what
its header declares, the ctypes table covers the header, its code object holds exactly the shipped kernels without scratch
or spills, and the core built for the host (tests/host_sim/tris_sim.cpp):
  * the walk over a hierarchy (any, count, fill + ordering) returns what the brute force over the predicate returns, for every
    set of query triangles and stack limit (the overflow path included), on meshes with zero-area triangles, 3 000 coincident
    triangles under a hierarchy of more than 32 levels, and without a hierarchy;
  * on inputs snapped to k * 2^-10, |k| <= 2^11, where every float64 operation of the predicate is exact, the sets EQUAL an
    exact integer reference that is no separating-axis test (tris_cases.exact_meets), pair for pair; of the 15 520 pairs
    2 183 are coplanar and 3 149 meet, 2 638 of them only touching (asserted floors: a tenth and a fifth);
  * identities that need no reference, the symmetry meets(T, Q) == meets(Q, T) among them;
  * invalid and degenerate queries, +-FLT_MAX vertices on either side, inactive and degenerate faces."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hostile_meshes as M
import nearest_cases as NC
import tris_cases as TC
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_tris.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BRUTE = "test_gpu_tris.py::test_kernels_match_the_brute_force_at_every_stack_limit"
TAILS = "test_gpu_tris.py::test_tails_of_the_lane_and_block_indexing"
HOSTILE = "test_gpu_tris.py::test_hostile_triangles"
MISUSE = "test_gpu_tris.py::test_fill_with_counts_of_other_queries_stays_inside_its_rows"
# one row per kernel of libtriro_tris.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "void k_tris<0>": (BRUTE, TAILS, HOSTILE),
    "void k_tris<1>": (BRUTE, TAILS, HOSTILE),
    "void k_tris<2>": (BRUTE, TAILS, HOSTILE, MISUSE),
    "k_tris_rows": (BRUTE, TAILS, MISUSE),
}
WALK_KERNELS = ("void k_tris<0>", "void k_tris<1>", "void k_tris<2>")
SYMBOLS = ["tr_tris_abi_version", "tr_tris_any", "tr_tris_count", "tr_tris_fill", "tr_tris_stack_capacity"]


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.tris_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_tris.h but not exported"
    assert set(hops.TRIS_ABI) == set(syms)


def test_abi_version_and_stack_capacity_match_the_sources():
    import tris_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_TRIS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.TRIS_ABI_VERSION == want == 1
    lib = hops.get_tris_module()
    assert lib.tr_tris_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_tris.h")).read()
    cap = int(re.search(r"#define\s+TR_TRIS_STACK\s+(\d+)", core).group(1))
    assert lib.tr_tris_stack_capacity() == cap == tris_sim.stack_capacity() == 32
    for name, nargs in (("tr_tris_any", 6), ("tr_tris_count", 6), ("tr_tris_fill", 9)):
        res, args = hops.TRIS_ABI[name]
        assert len(args) == nargs and args[2] is ctypes.c_int64 and args[-2] is ctypes.c_int, name
    assert hops.TRIS_ABI["tr_tris_fill"][1][5] is ctypes.c_int64
    # the culling, the activity rule, the row limit and the ordering are included and not copied
    assert '#include "tr_boxes.h"' in core
    for used in ("tr_within_sort(", "tr_rows_limit(", "tr_set_probe<", "tr_set_query(", "tr_set_kernel<", "tr_near_active(", "tr_load_tri<"):
        assert used in core + open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tris.hip")).read(), used
    assert not re.search(r"^TR_HD\w*\s+[\w:<>&* ]+\btr_(within|boxes?|near|load|walk|rows|set)_\w+\s*\(", core, re.M)      # no definition of theirs


def test_the_other_libraries_gained_no_symbol():
    import triro.backend.ops as hops
    others = [hops.library_path(), hops.nearest_library_path(), hops.within_library_path(), hops.boxes_library_path()]
    for path in others:
        lib = ctypes.CDLL(path)
        for s in header_symbols():
            assert not hasattr(lib, s), (path, s)
    text = open(os.path.join(ROOT, "include", "triro_hip.h")).read()
    assert set(hops.ABI) == set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_header_is_strict_c99():
    src = '#include "triro_tris.h"\nint main(void) { return TR_TRIS_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_tris_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_tris_stack_capacity()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.addressof(fake)
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    big = (1 << 31) * 128
    # any / count: (bvh, tri, n, out, stack_entries, stream)
    for fn in (lib.tr_tris_any, lib.tr_tris_count):
        assert fn(None, None, 0, None, 0, None) == 1 and b"bvh" in err()
        assert fn(h, out, -1, out, 0, None) == 1 and b"n < 0" in err()
        assert fn(h, out, 1, out, cap + 1, None) == 1 and b"stack_entries" in err()
        assert fn(h, out, 1, out, -1, None) == 1 and b"stack_entries" in err()
        assert fn(h, None, 1, out, 0, None) == 1 and b"null" in err()
        assert fn(h, out, 1, None, 0, None) == 1 and b"null" in err()
        assert fn(h, out, big, out, 0, None) == 1 and b"too many" in err()
        assert fn(h, None, 0, None, cap, None) == 0
    # fill: (bvh, tri, n, count, offsets, total, face, stack_entries, stream)
    fill = lib.tr_tris_fill
    assert fill(None, None, 0, None, None, 0, None, 0, None) == 1 and b"bvh" in err()
    assert fill(h, out, -1, out, out, 1, out, 0, None) == 1 and b"n < 0" in err()
    assert fill(h, out, 1, out, out, 1, out, cap + 1, None) == 1 and b"stack_entries" in err()
    assert fill(h, out, 1, out, out, 1, out, -1, None) == 1 and b"stack_entries" in err()
    assert fill(h, out, 1, out, out, -1, out, 0, None) == 1 and b"total < 0" in err()
    assert fill(h, None, 1, out, out, 1, out, 0, None) == 1 and b"null" in err()
    assert fill(h, out, 1, None, out, 1, out, 0, None) == 1 and b"null" in err()
    assert fill(h, out, 1, out, None, 1, out, 0, None) == 1 and b"null" in err()
    assert fill(h, out, 1, out, out, 1, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, big, out, out, 1, out, 0, None) == 1 and b"too many" in err()
    assert fill(h, None, 0, None, None, 0, None, cap, None) == 0
    assert fill(h, out, 1, out, out, 0, None, 0, None) == 0          # no rows: nothing to launch


# ---- 2. the code object ----------------------------------------------------------------------------------------------
def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.tris_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_tris_module().tr_tris_stack_capacity()
    for name, row in INVENTORY.items():
        assert row, name
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytest.mark.gpu" in src
        k = kernels[name]
        print(name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        # the stack: capacity node ids for 128 lanes, and nothing else; the ordering pass has no stack
        assert k["lds"] == (cap * 4 * 128 if name in WALK_KERNELS else 0), k
        assert k["vgpr"] <= 128, k          # the float64 leaf test must not limit occupancy below four waves per SIMD
    # the library this one builds on keeps exactly its kernels
    assert {k["name"] for k in con.kernels(hops.boxes_library_path())} == {"void k_boxes<0>", "void k_boxes<1>", "void k_boxes<2>", "k_boxes_rows"}


# ---- 3. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute_results():
    """{case: (v, f, [(label, triangles, brute force)])}, computed once"""
    import tris_sim
    out = {}
    for name, make in TC.CASES.items():
        v, f, _ = make()
        out[name] = (v, f, [(label, tri, tris_sim.brute(v, f, tri)) for label, tri in TC.query_sets(v, f)])
    return out


@pytest.mark.parametrize("name", list(TC.CASES))
def test_host_walk_matches_the_brute_force(name, brute_results):
    import tris_sim
    from sim import SimBVH
    v, f, rows = brute_results[name]
    B = SimBVH(v, f)
    if name == "deep":
        assert B.depth > 32
    overflowed = 0
    for label, tri, want in rows:
        for entries in (1, 2, 32):
            got, lost = tris_sim.walk(B, tri, entries, want_lost=True)
            TC.assert_same(got, want, f"{name}, {label}, stack_entries {entries}")
            if label == "larger than the mesh":
                # a walk of the whole tree pushes at every node with two internal children: one entry is lost on every
                # mesh here; the deep tree also loses entries at two
                assert entries != 1 or lost.all(), f"{name}: a stack of one entry did not overflow on the whole tree"
                overflowed += int(lost.sum()) if entries == 2 else 0
    if name == "deep":
        assert overflowed > 0, "deep: a stack of two entries never overflowed"


@pytest.mark.parametrize("name", list(TC.CASES))
def test_own_faces_meet_themselves_and_their_neighbours(name, brute_results):
    v, f, rows = brute_results[name]
    label, tri, res = rows[0]
    assert label == "own faces"
    TC.check_identities(res, name)
    tv = np.asarray(v, np.float64)[f]
    area = np.any(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 1]) != 0, axis=1)           # (exact for these meshes' own faces or not needed)
    got = TC.listed(res, len(tri), len(f))
    # the query is bit for bit a face of the mesh: find it, and every face that shares a vertex position with it
    flat = tv.reshape(len(f), 9)
    checked = 0
    for i, q in enumerate(np.asarray(tri, np.float64).reshape(-1, 9)):
        same = np.flatnonzero((flat == q).all(1))
        assert len(same) > 0
        if not area[same[0]]:
            assert res.count[i] == 0, f"{name}: a face without area meets something as a query"
            continue
        shares = ((tv[:, :, None, :] == q.reshape(3, 3)[None, None, :, :]).all(-1)).any(axis=(1, 2)) & area
        assert got[i][shares].all(), f"{name}: own face {same[0]} does not meet a face that shares a vertex with it"
        assert got[i][same[area[same]]].all()
        checked += 1
    assert checked > 0
    # displaced far enough, the own faces of a closed or scattered mesh meet fewer faces than in place
    assert rows[3][2].count.sum() < res.count.sum()


def test_meshes_without_a_hierarchy():
    import tris_sim
    from sim import SimBVH
    v, f = W.two_triangles()
    for nt in (2, 1):
        vv, ff = v[:3 * nt], f[:nt]
        seen = set()
        for label, tri in TC.query_sets(v, f):
            want = tris_sim.brute(vv, ff, tri)
            TC.check_identities(want, f"{nt} triangle(s), {label}")
            seen |= set(np.unique(want.count))
            for entries in (1, 0):
                TC.assert_same(tris_sim.walk(SimBVH(vv, ff), tri, entries), want, f"{nt} triangle(s), {label}")
        assert seen == set(range(nt + 1))
    # zero triangles: every query is answered with the miss values
    empty = SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32)))
    tri = TC.larger_than(v)
    for got in (tris_sim.walk(empty, tri), tris_sim.brute(v[:0], f[:0], tri)):
        assert not got.any.any() and not got.count.any() and len(got.faces) == 0 and got.offsets[-1] == 0


# ---- 4. exactness: snapped inputs against an exact integer reference -------------------------------------------------------
def test_snapped_inputs_equal_the_exact_reference():
    """coordinates k * 2^-10, |k| <= 2^11 (asserted by tris_cases.snapped): differences <= 2^12, normals and edge crosses <= 2^25,
    n x e <= 2^38, dots < 2^52 grid units -- every float64 operation of the predicate is exact, so it must EQUAL the exact
    reference, pair for pair"""
    import tris_sim
    from sim import SimBVH
    stats = TC.check_snapped(tris_sim.brute, "brute force")
    print("(pairs, met, only touching, coplanar) per mesh:", stats)
    print("(pairs, met, only touching, coplanar) in all:", TC.check_coverage(stats))
    assert all(0 < met < pairs and touching > 50 for pairs, met, touching, _ in stats.values())
    TC.check_snapped(lambda v, f, tri: tris_sim.walk(SimBVH(v, f), tri, 2), "host walk, two stack entries")


def test_the_predicate_is_symmetric_on_the_snapped_set():
    """meets(T, Q) == meets(Q, T): the faces as queries against the queries as a mesh"""
    import tris_sim
    for name, (v, f, tri, want, _, _) in TC.snapped_reference().items():
        qv = np.asarray(tri, np.float32).reshape(-1, 3)
        qf = np.arange(len(qv), dtype=np.int32).reshape(-1, 3)
        back = tris_sim.brute(qv, qf, np.asarray(v, np.float32)[f])
        assert np.array_equal(TC.listed(back, len(f), len(tri)).T, want), name


# ---- 5. hostile queries ----------------------------------------------------------------------------------------------------
def test_invalid_and_degenerate_queries_meet_nothing_and_flt_max_gives_no_nan():
    import tris_sim
    from sim import SimBVH
    v, f, _ = NC.icosphere()
    ext = TC.extent(v)
    tri, valid, degenerate = TC.hostile_triangles(TC.hashed_triangles(96, v.min(0), v.max(0), ext, seed=3))
    assert (~valid).sum() == 27 and degenerate.sum() == 5 and valid[degenerate].all()
    want = tris_sim.brute(v, f, tri)
    TC.check_identities(want, "hostile triangles")
    for entries in (1, 0):
        TC.assert_same(tris_sim.walk(SimBVH(v, f), tri, entries), want, f"hostile triangles, stack_entries {entries}")
    assert not want.any[~valid].any() and not want.count[~valid].any()
    assert not want.count[degenerate].any()
    assert want.count[32] > 0 and want.count[33] > 0          # the two huge triangles through the sphere
    assert want.count[34] == 0                                # the plane x = FLT_MAX
    assert want.any[valid].sum() >= 10 and (~want.any[valid]).sum() >= 10
    # +-FLT_MAX on the mesh's side: a mesh of the huge triangles, every query against it
    big = tri[32:37]
    bv, bf = big.reshape(-1, 3), np.arange(15, dtype=np.int32).reshape(-1, 3)
    back = tris_sim.brute(bv, bf, tri)
    TC.check_identities(back, "a mesh of huge triangles")
    TC.assert_same(tris_sim.walk(SimBVH(bv, bf), tri, 1), back, "a mesh of huge triangles")
    assert back.count[32:37].min() >= 1                       # each meets itself
    assert np.array_equal(TC.listed(back, len(tri), 5)[32:37], TC.listed(back, len(tri), 5)[32:37].T)


# ---- 6. inactive and degenerate faces -------------------------------------------------------------------------------------
HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_inactive_triangles_are_never_listed_and_never_counted(name, seed):
    import tris_sim
    from sim import SimBVH
    c = M.case(name, seed)
    fa, new = M.active_faces(c.v, c.f)
    B = SimBVH(c.v, c.f) if len(c.f) else None
    for tri in TC.hostile_mesh_triangles(c, fa):
        want = tris_sim.brute(c.v, c.f, tri)
        TC.check_identities(want, c.name)
        assert not c.inactive[want.faces].any(), f"{c.name}: an inactive triangle is listed"
        # the same mesh without its inactive faces answers the same, up to the renumbering of the faces
        alone = tris_sim.brute(c.v, fa, tri)
        assert np.array_equal(want.count, alone.count) and np.array_equal(M.map_ids(want.faces, new), alone.faces)
        if B is not None:
            for entries in (1, 0):
                TC.assert_same(tris_sim.walk(B, tri, entries), want, f"{c.name}, stack_entries {entries}")


def test_degenerate_faces_are_never_met():
    import tris_sim
    v, f, _ = NC.soup_with_degenerates()
    deg = np.arange(len(f) - 6, len(f))
    # queries through and around each zero-area face: triangles that contain its vertices
    tv = v[f[deg]]                                                               # [6, 3, 3]
    tri = np.concatenate([tv + np.float32([[-1, -1, 0], [1, -1, 0], [0, 1, 0]]) * np.float32(s) for s in (0.5, 2.0)] +
                         [tv[:, [0, 0, 0], :] + np.float32([[-1, 0, -1], [1, 0, -1], [0, 0, 1]]) * np.float32(0.25)])
    res = tris_sim.brute(v, f, tri)
    assert not np.isin(res.faces, deg).any() and res.count.sum() > 0
    assert not tris_sim.brute(v, f, tv).any.any()                               # as queries they meet nothing either
