"""CPU checks of libtriro_nearest.so (include/triro_nearest.h, csrc/nearest.hip, csrc/tr_nearest.h): the library is built and
exports what its header declares, the ctypes table covers the header, its code object holds exactly k_closest_point
without scratch or spills, and the core built for the host (tests/host_sim/nearest_sim.cpp):
  * the walk over a hierarchy returns the bits of the brute force over the per-triangle function, at every stack limit
    (the overflow path included), on meshes with face / edge / vertex ties, zero-area triangles, 3 000 coincident
    triangles under a hierarchy of more than 32 levels, and without a hierarchy;
  * the brute force agrees with an independent numpy float64 evaluation (tests/nearest_cases.py) within bounds that come
    from the number formats: one float32 rounding plus 2^-40 of the coordinate scale."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nearest_cases as NC
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_nearest.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# one row per kernel of libtriro_nearest.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "k_closest_point": ("test_gpu_nearest.py::test_hierarchical_meshes_at_every_stack_limit",
                        "test_gpu_nearest.py::test_tails_of_the_lane_and_block_indexing",
                        "test_gpu_nearest.py::test_hostile_points"),
}


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.nearest_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == ["tr_closest_point", "tr_nearest_abi_version", "tr_nearest_stack_capacity"]
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_nearest.h but not exported"
    assert set(hops.NEAREST_ABI) == set(syms)


def test_abi_version_and_stack_capacity_match_the_sources():
    import nearest_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_NEAREST_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.NEAREST_ABI_VERSION == want
    lib = hops.get_nearest_module()
    assert lib.tr_nearest_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_nearest.h")).read()
    cap = int(re.search(r"#define\s+TR_NEAR_STACK\s+(\d+)", core).group(1))
    assert lib.tr_nearest_stack_capacity() == cap == nearest_sim.stack_capacity()
    res, args = hops.NEAREST_ABI["tr_closest_point"]
    assert len(args) == 8 and args[2] is ctypes.c_int64 and args[6] is ctypes.c_int


def test_libtriro_hip_gained_no_symbol_of_the_nearest_library():
    import triro.backend.ops as hops
    hip = ctypes.CDLL(hops.library_path())
    for s in header_symbols():
        assert not hasattr(hip, s), s
    text = open(os.path.join(ROOT, "include", "triro_hip.h")).read()
    assert set(hops.ABI) == set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_header_is_strict_c99():
    src = '#include "triro_nearest.h"\nint main(void) { return TR_NEAREST_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_nearest_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_nearest_stack_capacity()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.addressof(fake)
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    assert lib.tr_closest_point(None, None, 0, None, None, None, 0, None) == 1 and b"bvh" in err()
    assert lib.tr_closest_point(h, out, -1, out, out, out, 0, None) == 1 and b"n < 0" in err()
    assert lib.tr_closest_point(h, out, 1, out, out, out, cap + 1, None) == 1 and b"stack_entries" in err()
    assert lib.tr_closest_point(h, out, 1, out, out, out, -1, None) == 1 and b"stack_entries" in err()
    assert lib.tr_closest_point(h, None, 1, out, out, out, 0, None) == 1 and b"null" in err()
    assert lib.tr_closest_point(h, out, 1, out, out, None, 0, None) == 1 and b"null" in err()
    assert lib.tr_closest_point(h, out, (1 << 31) * 128, out, out, out, 0, None) == 1 and b"too many" in err()
    # nothing to do is no error, with or without the optional outputs
    assert lib.tr_closest_point(h, None, 0, None, None, None, cap, None) == 0


# ---- 2. the code object ----------------------------------------------------------------------------------------------
def test_the_code_object_holds_exactly_the_shipped_kernel_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.nearest_library_path())}
    assert set(kernels) == set(INVENTORY)
    for name, row in INVENTORY.items():
        assert row, name
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytest.mark.gpu" in src
        k = kernels[name]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        # the far-child stack: capacity entries of {node, bound} for 128 lanes, and nothing else
        assert k["lds"] == hops.get_nearest_module().tr_nearest_stack_capacity() * 8 * 128, k
        assert k["vgpr"] <= 168, k          # the 32 KB of LDS allow five workgroups = ten waves per CU; registers must not be what limits it further


# ---- 3. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute_results():
    """the brute force of every hierarchical case, computed once"""
    import nearest_sim
    out = {}
    for name, make in NC.HIERARCHICAL.items():
        v, f, p = make()
        out[name] = (v, f, p, nearest_sim.brute(v, f, p))
    return out


@pytest.mark.parametrize("name", list(NC.HIERARCHICAL))
def test_host_walk_matches_the_brute_force_bit_for_bit(name, brute_results):
    import nearest_sim
    from sim import SimBVH
    v, f, p, want = brute_results[name]
    B = SimBVH(v, f)
    if name == "deep":
        assert B.depth > 32
    assert (want[2] >= 0).all() and np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for entries in (1, 2, 3, 0):
        *got, lost = nearest_sim.walk(B, p, entries, want_lost=True)
        NC.assert_same_bits(got, want, f"{name}, stack_entries {entries}")
        if entries == 1:
            assert lost.any(), f"{name}: a stack of one entry never overflowed: the second walk was not exercised"
        if entries == 0 and name != "deep":
            assert not lost.any(), name
    if name == "cube":
        # the centre is equidistant from every face: all twelve triangles tie, face 0 wins; vertices tie between faces
        centre = (9 * 9 * 9) // 2
        assert want[2][centre] == 0 and want[1][centre] == np.float32(0.5 * (v.max() - v.min()))
        assert (want[1][[0, 8, 728]] == 0).all()
    if name == "deep":
        # 3 000 coincident triangles: a point nearest to the pile gets the first of them
        first = len(f) - 3000
        assert want[2][190] == first and want[1][190] == 0 and (want[2] == first).sum() > 3


def test_meshes_without_a_hierarchy(brute_results):
    import nearest_sim
    from sim import SimBVH
    v, f = W.two_triangles()
    p = np.concatenate([NC.hash_points(60, 5, [-0.8, -0.8, -1.4], [0.8, 0.8, 0.4]),
                        np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.5, -0.5, 0.0], [0.0, 0.5, -2.0]], np.float32)])
    for nt in (2, 1):
        vv, ff = v[:3 * nt], f[:nt]
        want = nearest_sim.brute(vv, ff, p)
        for entries in (1, 0):
            NC.assert_same_bits(nearest_sim.walk(SimBVH(vv, ff), p, entries), want, f"{nt} triangle(s)")
        NC.check_against_numpy(vv, ff, p, *want, what=f"{nt} triangle(s)")
    assert want[2].max() == 0
    # between the two triangles the lower face index wins the tie
    assert nearest_sim.brute(v, f, p)[2][60] == 0 and nearest_sim.brute(v, f, p)[1][60] == 0.5
    # zero triangles: every point is answered (-1, +Inf, NaN)
    empty = SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32)))
    for got in (nearest_sim.walk(empty, p), nearest_sim.brute(v[:0], f[:0], p)):
        assert (got[2] == -1).all() and np.isposinf(got[1]).all() and np.isnan(got[0]).all()


# ---- 4. host brute force against numpy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NC.TOLERANCE_CASES)
def test_brute_force_agrees_with_an_independent_numpy_evaluation(name, brute_results):
    v, f, p, (closest, distance, tri) = brute_results[name]
    NC.check_against_numpy(v, f, p, closest, distance, tri, what=name)
    if name == "soup":
        # the six zero-area triangles are somebody's nearest: the degenerate branch of both sides is exercised
        D = NC.numpy_distances(v, f[-6:], p)
        assert (D.min(1) <= NC.numpy_distances(v, f, p).min(1)).any() and np.isin(tri, np.arange(len(f) - 6, len(f))).any()


def test_degenerate_triangles_are_their_segment_or_point():
    import nearest_sim
    v = np.array([[0, 0, 0], [4, 0, 0], [1, 0, 0], [2, 3, 5], [2, 3, 5], [2, 3, 5], [0, 0, 0], [0, 0, 0], [0, 2, 0]], np.float32)
    p = np.array([[2, 3, 0], [-1, -1, 0], [9, 0, 1], [2, 3, 6], [0, 1, 1]], np.float32)
    for k, want_c, want_d in ((0, [[2, 0, 0], [0, 0, 0], [4, 0, 0], [2, 0, 0], [0, 0, 0]], [3, 2 ** 0.5, 26 ** 0.5, 45 ** 0.5, 2 ** 0.5]),
                              (1, [[2, 3, 5]] * 5, [5, 50 ** 0.5, 74 ** 0.5, 1, 24 ** 0.5]),
                              (2, [[0, 2, 0], [0, 0, 0], [0, 0, 0], [0, 2, 0], [0, 1, 0]], [5 ** 0.5, 2 ** 0.5, 82 ** 0.5, 41 ** 0.5, 1])):
        c, d, t = nearest_sim.brute(v, np.array([[3 * k, 3 * k + 1, 3 * k + 2]], np.int32), p)
        assert np.array_equal(c, np.array(want_c, np.float32)) and np.array_equal(d, np.array(want_d, np.float64).astype(np.float32)), k
        assert (t == 0).all()


# ---- 5. non-finite points ----------------------------------------------------------------------------------------------
def test_non_finite_points_are_answered_with_no_triangle():
    import nearest_sim
    from sim import SimBVH
    v, f, _ = NC.icosphere()
    p = np.full((10, 3), 0.25, np.float32)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for axis in range(3):
            p[3 * k + axis, axis] = bad
    want_ok = nearest_sim.brute(v, f, p[9:])
    for got in (nearest_sim.brute(v, f, p), nearest_sim.walk(SimBVH(v, f), p, 0), nearest_sim.walk(SimBVH(v, f), p, 1)):
        assert (got[2][:9] == -1).all() and np.isposinf(got[1][:9]).all() and np.isnan(got[0][:9]).all()
        assert got[2][9] == want_ok[2][0] >= 0 and np.isfinite(got[0][9]).all()
    # the ends of the float range are finite points: answered, distance +Inf where it exceeds the float range
    far = np.array([[3e38, 3e38, 3e38], [-3e38, 0, 0], [2.0 ** 60, 0, 0], [1e-45, -1e-40, 0]], np.float32)
    c, d, t = nearest_sim.brute(v, f, far)
    NC.assert_same_bits(nearest_sim.walk(SimBVH(v, f), far, 2), (c, d, t), "far points")
    assert (t >= 0).all() and np.isfinite(c).all() and np.isposinf(d[0]) and np.isfinite(d[1:]).all() and not np.isnan(d).any()
