"""CPU checks of libtriro_tri_nearest.so (include/triro_tri_nearest.h, csrc/tri_nearest.hip, csrc/tr_tri_nearest.h): the library
is built, loads through the satellite loader and exports what its header declares, its code object holds exactly
k_triangles_nearest within the register and LDS budget, and the core built for the host (tests/host_sim/tri_nearest_sim.cpp):
  * the walk over a hierarchy returns the bits of the brute force over the distance function of a pair, at every stack limit
    (the overflow path included), with and without a bound, on meshes with ties, zero-area triangles, 3 000 coincident
    triangles under a hierarchy of more than 32 levels, and without a hierarchy;
  * the distance function agrees with an exact evaluation in integers and fractions on snapped inputs -- 0 exactly where a pair
    meets, within one float32 rounding plus 2^-40 of the coordinate scale elsewhere -- and with an independent numpy float64
    evaluation off the grid (tests/tri_nearest_cases.py);
  * the chunked, bound-carrying reduction of mesh_distance does not depend on the chunk."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hostile_meshes as M
import nearest_cases as NC
import tri_nearest_cases as TN
import tris_cases as TC
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_tri_nearest.h")
KEY = "tri_nearest"
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# one row per kernel of libtriro_tri_nearest.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "k_triangles_nearest": ("test_gpu_tri_nearest.py::test_kernel_matches_the_brute_force_at_every_stack_limit",
                            "test_gpu_tri_nearest.py::test_tails_of_the_lane_and_block_indexing",
                            "test_gpu_tri_nearest.py::test_hostile_triangles"),
}
SYMBOLS = ["tr_tri_nearest_abi_version", "tr_tri_nearest_stack_capacity", "tr_triangles_nearest"]


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


def _child(code, **env):
    """run `code` in a fresh interpreter that can import triro; the environment is this one's plus `env`"""
    paths = [ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd")]
    head = f"import sys; sys.path[:0] = {paths!r}; import triro.backend.ops as hops\n"
    return subprocess.run([sys.executable, "-c", head + code], env={**os.environ, **env}, capture_output=True, text=True, timeout=120)


# ---- 1. the library, its loader and its header --------------------------------------------------------------------------
def test_the_path_follows_from_the_key_and_the_environment_overrides_it(monkeypatch):
    import triro.backend.ops as hops
    monkeypatch.delenv("TRIRO_TRI_NEAREST_LIBRARY", raising=False)
    assert hops.tri_nearest_library_path() == os.path.join(os.path.dirname(hops.library_path()), "libtriro_tri_nearest.so")
    monkeypatch.setenv("TRIRO_TRI_NEAREST_LIBRARY", "/somewhere/else.so")
    assert hops.tri_nearest_library_path() == "/somewhere/else.so"


def test_a_missing_library_raises_with_its_path(tmp_path):
    missing = str(tmp_path / "no_such_tri_nearest.so")
    r = _child(f"""
try:
    hops.get_tri_nearest_module()
except RuntimeError as e:
    assert {missing!r} in str(e), str(e)
    print("RAISED")
""", TRIRO_TRI_NEAREST_LIBRARY=missing)
    assert r.returncode == 0 and "RAISED" in r.stdout, r.stdout + r.stderr


def test_a_version_mismatch_raises_with_both_numbers():
    r = _child("""
have = hops.TRI_NEAREST_ABI_VERSION
hops.TRI_NEAREST_ABI_VERSION = 99
try:
    hops.get_tri_nearest_module()
except RuntimeError as e:
    assert f"version {have} " in str(e) and "99" in str(e) and "libtriro_tri_nearest.so" in str(e), str(e)
    print("RAISED")
""")
    assert r.returncode == 0 and "RAISED" in r.stdout, r.stdout + r.stderr


def test_the_library_loads_once_and_every_symbol_of_the_table_is_bound():
    import triro.backend.ops as hops
    lib = hops.get_tri_nearest_module()
    assert hops.get_tri_nearest_module() is lib
    assert header_symbols() == sorted(SYMBOLS) == sorted(hops.TRI_NEAREST_ABI)
    for name, (res, args) in hops.TRI_NEAREST_ABI.items():
        fn = getattr(lib, name)
        assert fn.restype is res, name
        assert list(fn.argtypes or []) == list(args), name
    res, args = hops.TRI_NEAREST_ABI["tr_triangles_nearest"]
    assert len(args) == 11 and args[2] is ctypes.c_int64 and args[4] is ctypes.c_float and args[9] is ctypes.c_int


def test_abi_version_and_stack_capacity_match_the_sources():
    import tri_nearest_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_TRI_NEAREST_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.TRI_NEAREST_ABI_VERSION == want
    lib = hops.get_tri_nearest_module()
    assert lib.tr_tri_nearest_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_nearest.h")).read()
    cap = int(re.search(r"#define\s+TR_NEAR_STACK\s+(\d+)", core).group(1))
    assert lib.tr_tri_nearest_stack_capacity() == cap == tri_nearest_sim.stack_capacity()


def test_libtriro_hip_gained_no_symbol_of_this_library():
    import triro.backend.ops as hops
    hip = ctypes.CDLL(hops.library_path())
    for s in header_symbols():
        assert not hasattr(hip, s), s
    text = open(os.path.join(ROOT, "include", "triro_hip.h")).read()
    assert set(hops.ABI) == set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_header_is_strict_c99():
    src = '#include "triro_tri_nearest.h"\nint main(void) { return TR_TRI_NEAREST_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_tri_nearest_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_tri_nearest_stack_capacity()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.addressof(fake)
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    inf = float("inf")
    fn = lib.tr_triangles_nearest      # (bvh, triangles, n, d_max, max_distance, tri, distance, closest_mesh, closest_query, stack_entries, stream)
    assert fn(None, None, 0, None, inf, None, None, None, None, 0, None) == 1 and b"bvh" in err()
    assert fn(h, out, -1, None, inf, out, out, out, out, 0, None) == 1 and b"n < 0" in err()
    assert fn(h, out, 1, None, inf, out, out, out, out, cap + 1, None) == 1 and b"stack_entries" in err()
    assert fn(h, out, 1, None, inf, out, out, out, out, -1, None) == 1 and b"stack_entries" in err()
    assert fn(h, None, 1, None, inf, out, out, out, out, 0, None) == 1 and b"null" in err()
    assert fn(h, out, 1, None, inf, None, out, out, out, 0, None) == 1 and b"null" in err()
    assert fn(h, out, (1 << 31) * 128, out, 1.0, out, out, out, out, 0, None) == 1 and b"too many" in err()
    # nothing to do is no error, with or without the optional outputs and the bounds
    assert fn(h, None, 0, None, inf, None, None, None, None, cap, None) == 0
    assert fn(h, None, 0, out, 1.0, out, out, out, out, 0, None) == 0


# ---- 2. the code object ----------------------------------------------------------------------------------------------
def test_the_code_object_holds_exactly_the_shipped_kernel_within_its_budget():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.tri_nearest_library_path())}
    assert set(kernels) == set(INVENTORY)
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
        # the far-child stack: capacity entries of {node, bound} for 128 lanes, and nothing else
        assert k["lds"] == hops.get_tri_nearest_module().tr_tri_nearest_stack_capacity() * 8 * 128, k
        assert k["vgpr"] <= 168, k          # the 32 KB of LDS allow five workgroups = ten waves per CU; registers must not limit it further


# ---- 3. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute_results():
    """{case: (v, f, [(label, triangles, brute force)])}, computed once"""
    import tri_nearest_sim
    out = {}
    for name, make in TN.CASES.items():
        v, f, _ = make()
        out[name] = (v, f, [(label, tri, tri_nearest_sim.brute(v, f, tri)) for label, tri in TN.query_sets(v, f)])
    return out


@pytest.mark.parametrize("name", list(TN.CASES))
def test_host_walk_matches_the_brute_force_bit_for_bit(name, brute_results):
    import tri_nearest_sim
    from sim import SimBVH
    v, f, rows = brute_results[name]
    B = SimBVH(v, f)
    if name == "deep":
        assert B.depth > 32
    ever_lost = False
    for label, tri, want in rows:
        assert (want[0] >= 0).all() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all() and np.isfinite(want[3]).all()
        for entries in (0, 1, 2, 3):
            *got, lost = tri_nearest_sim.walk(B, tri, None, entries, want_lost=True)
            TN.assert_same(got, want, f"{name}, {label}, stack_entries {entries}")
            ever_lost |= bool(lost.any())
    assert ever_lost, f"{name}: no stack ever overflowed: the second walk was not exercised"
    # an own face is at distance 0 from the mesh: it meets itself, or -- without area -- touches itself; the smallest face that
    # meets it wins (faces with a smaller index share an edge or a vertex with it)
    label, tri, (face, distance, on_mesh, on_query) = rows[0]
    assert (distance == 0).all()
    own = np.unique(np.linspace(0, len(f) - 1, min(TC.MAX_OWN, len(f))).astype(int))
    assert (face <= own).all() and (face < own).any()
    # two extents away nothing is at distance 0, and the two witnesses are that far apart
    label, tri, (face, distance, on_mesh, on_query) = rows[2]
    assert (distance > 0).all() and np.isfinite(distance).all()


@pytest.mark.parametrize("name", list(TN.CASES))
def test_a_bound_admits_the_faces_within_it(name, brute_results):
    import tri_nearest_sim
    from sim import SimBVH
    v, f, rows = brute_results[name]
    B = SimBVH(v, f)
    tri = np.concatenate([t for _, t, _ in rows])
    free = tuple(np.concatenate([w[k] for _, _, w in rows]) for k in range(4))
    r = TN.half_bound(free[1])
    want = tri_nearest_sim.brute(v, f, tri, r)
    within = want[0] >= 0
    assert within.sum() >= len(tri) // 4 and (~within).sum() >= len(tri) // 8, f"{name}: {within.sum()} of {len(tri)} within {r}"
    # within the bound the answer is the unbounded one, bit for bit; beyond it there is none.  (The identity is one of d2:
    # a distance that rounds to r may belong to a d2 just above r^2.)
    assert (free[1][within] <= r).all() and (free[1][~within] >= r).all()
    TN.assert_same(tuple(a[within] for a in want), tuple(a[within] for a in free), f"{name}, within the bound")
    TN.check_no_result(want, ~within, f"{name}, beyond the bound")
    for entries in (0, 1, 2, 3):
        TN.assert_same(tri_nearest_sim.walk(B, tri, r, entries), want, f"{name}, bounded, stack_entries {entries}")
    # per-query bounds: every other query unbounded, and the invalid radii of tr_within.h
    radii = np.where(np.arange(len(tri)) % 2 == 0, np.float32(np.inf), r).astype(np.float32)
    radii[1:40:4] = np.nan
    radii[3:40:4] = -1.0
    want = tri_nearest_sim.brute(v, f, tri, radii)
    TN.check_no_result(want, np.isnan(radii) | (radii < 0), name)
    TN.assert_same(tuple(a[::2] for a in want), tuple(a[::2] for a in free), f"{name}, +Inf is unbounded")
    for entries in (0, 1):
        TN.assert_same(tri_nearest_sim.walk(B, tri, radii, entries), want, f"{name}, per-query bounds, stack_entries {entries}")
    # a bound of 0 keeps the faces at distance exactly 0
    zero = tri_nearest_sim.brute(v, f, tri, 0.0)
    assert np.array_equal(zero[0] >= 0, free[1] == 0)
    TN.assert_same(tri_nearest_sim.walk(B, tri, 0.0, 1), zero, f"{name}, bound 0")


def test_meshes_without_a_hierarchy():
    import tri_nearest_sim
    from sim import SimBVH
    v, f = W.two_triangles()
    empty = SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32)))
    for label, tri in TN.query_sets(v, f):
        tri = np.concatenate([tri, np.full((1, 3, 3), np.nan, np.float32)])
        for nt in (2, 1, 0):
            vv, ff = v[:3 * nt], f[:nt]
            want = tri_nearest_sim.brute(vv, ff, tri)
            TN.check_no_result(want, [-1] if nt else slice(None), f"{nt} triangle(s), {label}")
            if nt:
                assert (want[0][:-1] >= 0).all() and want[0].max() <= nt - 1
            for entries in (1, 0):
                TN.assert_same(tri_nearest_sim.walk(SimBVH(vv, ff) if nt else empty, tri, None, entries), want, f"{nt} triangle(s), {label}")


def test_ties_go_to_the_smaller_face_index():
    """a flat box and a query triangle in its mid-plane: the two large faces are at exactly the same distance on either side, and
    so are the two triangles of each where the query lies across their diagonal.  The smallest index wins at every stack limit --
    what a `>=` in the cull, or a push that forgot a tie, would break"""
    import tri_nearest_sim
    from sim import SimBVH
    v, f, _ = NC.cube()
    v = (v * np.float32([4, 4, 0.5])).astype(np.float32)
    tri = np.array([[[-0.5, -0.25, 0], [0.75, 0.5, 0], [0.25, 1.0, 0]],           # across the diagonals
                    [[1.0, 0.25, 0], [1.5, 0.25, 0], [1.5, 0.5, 0]],               # beside them
                    [[0, 0, 0], [0, 0, 0], [0, 0, 0]]], np.float32)                # the centre, as a point
    d2 = tri_nearest_sim.pairs_d2(tri, v[f])
    tied = d2 == d2.min(1, keepdims=True)
    z = v[f][:, :, 2]
    low, high = (z == -0.5).all(1), (z == 0.5).all(1)
    assert (d2.min(1) == 0.25).all() and (tied & low).any(1).all() and (tied & high).any(1).all()
    assert tied[0].sum() == 4 and tied[1].sum() == 2 and tied[2].sum() == 4
    want = tri_nearest_sim.brute(v, f, tri)
    assert np.array_equal(want[0], tied.argmax(1)) and (want[1] == 0.5).all()
    for order in (np.arange(len(f)), np.arange(len(f))[::-1]):      # the same faces in both orders: the tree differs, the rule does not
        ff = np.ascontiguousarray(f[order])
        want = tri_nearest_sim.brute(v, ff, tri)
        assert np.array_equal(want[0], tied[:, order].argmax(1))
        for entries in (0, 1, 2, 3):
            TN.assert_same(tri_nearest_sim.walk(SimBVH(v, ff), tri, None, entries), want, f"ties, stack_entries {entries}")
            TN.assert_same(tri_nearest_sim.walk(SimBVH(v, ff), tri, 0.5, entries), want, f"ties at exactly the bound, stack_entries {entries}")
        TN.check_no_result(tri_nearest_sim.walk(SimBVH(v, ff), tri, np.float32(0.49999997), 1), slice(None), "just below the tie")


# ---- 4. independent evaluation 1: exact, on the grid ----------------------------------------------------------------------
def test_the_pair_function_against_the_exact_reference_on_snapped_inputs():
    """every (query, face) pair of the snapped meshes: d2 == 0.0 exactly where the pair meets and > 0 where both have area and
    do not; the distance within one float32 spacing plus 2^-40 of the scale of the exact one; the brute force's winner an exact
    minimiser within the same eps, and the smallest index among bit-equal minimisers"""
    import tri_nearest_sim
    worst, ties = -np.inf, 0
    for name, (v, f, tri, met, area_q, area_t, exact) in TN.exact_reference().items():
        d2 = tri_nearest_sim.pairs_d2(tri, v[f])
        both = area_q[:, None] & area_t[None, :]
        assert not (met & ~both).any()
        assert (d2[met] == 0.0).all(), f"{name}: {int((d2[met] != 0).sum())} meeting pairs are not at 0"
        assert (d2[both & ~met] > 0.0).all(), f"{name}: a pair with area that does not meet is at 0"
        # the pairs the meeting rule does not cover, and the floor on what the fixtures hold
        excluded, held = 1.0 - both.mean(), (~area_q).mean() + (~area_t).mean()
        print(f"{name}: {excluded:.3%} of {both.size} pairs have a triangle without area; without area: {(~area_q).mean():.3%} of the "
              f"queries, {(~area_t).mean():.3%} of the faces")
        assert excluded <= held
        S = float(max(np.abs(v).max(), np.abs(tri).max()))
        got, want = np.sqrt(d2).astype(np.float32).astype(np.float64), np.sqrt(exact)
        excess = np.abs(got - want) - TN.eps_of(want, S)
        worst = max(worst, excess.max())
        print(f"{name}: worst excess of |distance - exact| over its bound (<= 0 passes): {excess.max():.3g}")
        assert (excess <= 0).all(), f"{name}: {int((excess > 0).sum())} pairs, worst excess {excess.max()}"
        res = tri_nearest_sim.brute(v, f, tri)
        assert np.array_equal(res[1], np.sqrt(d2.min(1)).astype(np.float32))
        TN.check_exact_winner(name, res, "brute force")
        # bit-equal ties among the exact minimisers
        for i in range(len(tri)):
            J = np.flatnonzero(exact[i] == exact[i].min())
            if len(J) > 1 and (d2[i, J] == d2[i].min()).all():
                ties += 1
                assert res[0][i] == J[0], f"{name}, query {i}: faces {J} tie exactly, {res[0][i]} was returned"
    print(f"worst excess in all: {worst:.3g}; queries whose exact minimisers tie bit for bit: {ties}")
    assert ties > 50


def test_host_walk_on_snapped_inputs_equals_the_exact_reference():
    import tri_nearest_sim
    from sim import SimBVH
    for name, (v, f, tri, *_) in TN.exact_reference().items():
        want = tri_nearest_sim.brute(v, f, tri)
        for entries in (0, 2):
            got = tri_nearest_sim.walk(SimBVH(v, f), tri, None, entries)
            TN.assert_same(got, want, f"{name}, stack_entries {entries}")
        TN.check_exact_winner(name, got, "host walk")


def test_the_degenerate_caveat_a_piercing_segment_is_not_at_zero():
    """deliberate (csrc/tr_tri_nearest.h): a triangle without area meets nothing, so a segment through the interior of a face has
    the distance of the nearest boundary features, while the same segment widened to a sliver with area is at 0"""
    import tri_nearest_sim
    face = np.float32([[-1, -1, 0], [1, -1, 0], [0, 1, 0]])
    segment = np.float32([[0, -0.25, -1], [0, -0.25, 1], [0, -0.25, 1]])
    sliver = np.float32([[0, -0.25, -1], [0, -0.25, 1], [2.0 ** -10, -0.25, 1]])
    d2, x, y = tri_nearest_sim.pair(segment, face)
    assert d2 > 0.01 and np.isfinite(x).all() and np.isfinite(y).all()
    assert tri_nearest_sim.pair(face, segment)[0] == d2
    assert tri_nearest_sim.pair(sliver, face)[0] == 0.0 and tri_nearest_sim.pair(face, sliver)[0] == 0.0
    # a segment that touches the boundary is at 0 by its candidates
    assert tri_nearest_sim.pair(np.float32([[0, -1, -1], [0, -1, 1], [0, -1, 1]]), face)[0] == 0.0


# ---- 5. independent evaluation 2: numpy float64, off the grid ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "soup"])
def test_brute_force_agrees_with_an_independent_numpy_evaluation(name, brute_results):
    v, f, rows = brute_results[name]
    zero = 0
    for label, tri, want in rows:
        pick = slice(None, None, 3)            # a third of every set: the numpy side evaluates every face at 27 edge points
        TN.check_against_numpy(v, f, tri[pick], tuple(a[pick] for a in want), f"{name}, {label}")
        zero += int((want[1] == 0).sum())
    assert zero > 0


# ---- 6. hostile inputs ---------------------------------------------------------------------------------------------------
def test_invalid_queries_have_no_result_and_flt_max_gives_no_nan():
    import tri_nearest_sim
    from sim import SimBVH
    v, f, _ = NC.icosphere()
    tri, valid, degenerate = TC.hostile_triangles(TC.hashed_triangles(64, v.min(0), v.max(0), TC.extent(v), seed=3))
    want = tri_nearest_sim.brute(v, f, tri)
    for entries in (0, 1):
        TN.assert_same(tri_nearest_sim.walk(SimBVH(v, f), tri, None, entries), want, f"hostile triangles, stack_entries {entries}")
    assert (~valid).sum() == 27
    TN.check_no_result(want, ~valid, "invalid queries")
    face, distance, on_mesh, on_query = (a[valid] for a in want)
    assert (face >= 0).all() and not np.isnan(distance).any() and np.isfinite(on_mesh).all() and np.isfinite(on_query).all()
    assert np.isfinite(distance[degenerate[valid]]).all()             # segments and points are answered as what they are
    assert want[1][32] == 0 and want[1][33] == 0                      # the +-FLT_MAX triangles through the mesh meet it
    assert want[1][34] > 1e38 and want[0][34] >= 0                    # the plane x = FLT_MAX: at the end of the float range, still a face
    # +-FLT_MAX on the mesh's side
    bv, bf = tri[32:37].reshape(-1, 3), np.arange(15, dtype=np.int32).reshape(-1, 3)
    back = tri_nearest_sim.brute(bv, bf, tri)
    TN.assert_same(tri_nearest_sim.walk(SimBVH(bv, bf), tri, None, 1), back, "a mesh of huge triangles")
    TN.check_no_result(back, ~valid, "a mesh of huge triangles")
    assert not np.isnan(back[1]).any() and (back[1][32:37] == 0).all()


HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_inactive_triangles_are_never_returned(name, seed):
    import tri_nearest_sim
    from sim import SimBVH
    c = M.case(name, seed)
    fa, new = M.active_faces(c.v, c.f)
    B = SimBVH(c.v, c.f) if len(c.f) else None
    for tri in TC.hostile_mesh_triangles(c, fa):
        want = tri_nearest_sim.brute(c.v, c.f, tri)
        found = want[0] >= 0
        assert np.array_equal(found, np.isfinite(tri).all(axis=(1, 2)) & (len(fa) > 0)), c.name      # (a query may have overflowed)
        assert not c.inactive[want[0][found]].any(), f"{c.name}: an inactive triangle is returned"
        assert not np.isnan(want[1]).any()
        # the same mesh without its inactive faces answers the same, up to the renumbering of the faces
        alone = tri_nearest_sim.brute(c.v, fa, tri)
        TN.assert_same((M.map_ids(want[0], new), *want[1:]), alone, f"{c.name}, without the inactive faces")
        if B is not None:
            for entries in (1, 0, 3):
                TN.assert_same(tri_nearest_sim.walk(B, tri, None, entries), want, f"{c.name}, stack_entries {entries}")


# ---- 7. mesh_distance's reduction ------------------------------------------------------------------------------------------
def test_the_chunked_reduction_does_not_depend_on_the_chunk(brute_results):
    """a numpy model of mesh_distance (tri_nearest_cases.reduce_rows) on the brute force's rows: the bound carried from chunk to
    chunk loses nothing"""
    for name in ("icosphere", "soup"):
        v, f, rows = brute_results[name]
        for label, tri, want in rows:
            whole = TN.reduce_rows(want)
            k = int(np.flatnonzero(want[1] == want[1].min())[0])
            assert whole[1] == k and whole[0] == want[1][k] and whole[2] == want[0][k]
            for chunk in (7, 64, 1):
                TN.assert_same_pair(TN.reduce_rows(want, chunk), whole, f"{name}, {label}, chunk {chunk}")
            # a bound below the least distance leaves nothing; one at it keeps the winner
            if whole[0] > 0:
                none = TN.reduce_rows(want, 7, np.nextafter(whole[0], np.float32(0)))
                assert np.isposinf(none[0]) and none[1] == -1 and none[2] == -1 and np.isnan(none[3]).all() and np.isnan(none[4]).all()
            TN.assert_same_pair(TN.reduce_rows(want, 7, whole[0]), whole, f"{name}, {label}, bounded at the answer")
