"""CPU checks of libtriro_points.so (include/triro_points.h, csrc/points.hip): the library is built and exports what its
header declares, the ctypes table covers the header, its code object holds exactly the three instantiations of
k_contains_points (each with a row that names the GPU test comparing it with the oracle), and the per-point routine --
two unordered count traversals and the decision function of csrc/tr_points.h, built for the host
(tests/host_sim/points_sim.cpp) -- agrees with the oracle's contains_points and intersects_count."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import workloads as W
from oracle.oracle import OracleIntersector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_points.h")
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

DEFAULT_DIRECTION = np.array([0.4395064455, 0.617598629942, 0.652231566745], np.float32)

# one row per kernel of libtriro_points.so: the GPU test that launches it and compares it with the oracle
ADDRESSING = "test_gpu_contains.py::test_every_addressing_flavour_matches_the_oracle"
LATTICE = "test_gpu_contains.py::test_cube_lattice_with_exact_ties"
SHELLS = "test_gpu_contains.py::test_nested_shells_count_up_to_eight"
INVENTORY = {
    "void k_contains_points<true, false>": (LATTICE, SHELLS, ADDRESSING),      # compact: 32-bit offsets and trail words
    "void k_contains_points<true, true>": (ADDRESSING,),                       # deep: 32-bit offsets, 64-bit trail words
    "void k_contains_points<false, false>": (ADDRESSING,),                     # generic: 64-bit addressing
}


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.points_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == ["tr_contains_addressing", "tr_contains_points", "tr_points_abi_version"]
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_points.h but not exported"
    assert set(hops.POINTS_ABI) == set(syms)
    # ... and the table of libtriro_hip.so stays what its own header says
    hip = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "triro_hip.h")).read(), flags=re.S)
    assert set(hops.ABI) == set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", hip))


def test_abi_version_matches_the_header():
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_POINTS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.POINTS_ABI_VERSION == want
    assert hops.get_points_module().tr_points_abi_version() == want
    # the argument list of the binding is the header's: 12 parameters, the host summary a pointer to int64
    res, args = hops.POINTS_ABI["tr_contains_points"]
    assert len(args) == 12 and args[2] is ctypes.c_int64 and args[10] == ctypes.POINTER(ctypes.c_int64)
    assert hops.get_points_module().tr_contains_addressing(None) == -1


def test_invalid_arguments_are_refused_without_a_device():
    import triro.backend.ops as hops
    lib = hops.get_points_module()
    summary = ctypes.c_int64(7)
    assert lib.tr_contains_points(None, None, 0, None, None, None, None, None, None, None, ctypes.byref(summary), None) == 1
    assert b"bvh" in hops.get_module().tr_last_error()


def test_the_header_is_strict_c99():
    src = '#include "triro_points.h"\nint main(void) { return TR_POINTS_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_the_code_object_holds_exactly_the_three_instantiations():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.points_library_path())}
    assert set(kernels) == set(INVENTORY)
    for name, row in INVENTORY.items():
        assert row, name
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytest.mark.gpu" in src
        # the ring and the leaf queue, once (both passes share them): the LDS budget of the count launch
        assert kernels[name]["lds"] == (16 + 6) * 128 * 4, kernels[name]
    # no instantiation keeps anything in scratch (the 64-bit ones must not: csrc/kernels_direct.inc, TR_COUNT_W)
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in kernels.values()), kernels


def test_libtriro_hip_gained_no_symbol_of_the_points_library():
    import triro.backend.ops as hops
    hip = ctypes.CDLL(hops.library_path())
    for s in header_symbols():
        assert not hasattr(hip, s), s


# ---- the per-point routine on the host against the oracle -----------------------------------------------------------
def _lattice(lo, hi, k):
    """k^3 points that include both bounds on every axis: face, edge and vertex positions of the box"""
    ax = [np.linspace(lo[a], hi[a], k, dtype=np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def _cases():
    g = np.load(os.path.join(GOLD, "cube_axis_rays.npz"))
    v, f = g["vertices"], g["faces"]
    yield "cube lattice", v, f, _lattice(v.min(0), v.max(0), 9), (DEFAULT_DIRECTION, np.array([0, 0, 1], np.float32))
    g = np.load(os.path.join(GOLD, "c1_icosphere80_ortho64.npz"))
    v, f = g["vertices"], g["faces"]
    p = W.hash_rays(1500, 11, v.min(0) * 1.2, v.max(0) * 1.2)[0]
    yield "icosphere", v, f, np.ascontiguousarray(p), (DEFAULT_DIRECTION, np.array([-0.3, 0.2, 0.9], np.float32))
    g = np.load(os.path.join(GOLD, "soup400_hash4096.npz"))
    v, f = g["vertices"], g["faces"]
    p = np.ascontiguousarray(g["origins"][:1500])
    yield "soup", v, f, p, (DEFAULT_DIRECTION, np.array([1.0, 0.0, 0.0], np.float32))


@pytest.mark.parametrize("case", list(_cases()), ids=[c[0] for c in _cases()])
def test_host_routine_matches_the_oracle(case):
    import points_sim
    from sim import SimBVH
    what, v, f, p, directions = case
    B = SimBVH(v, f)
    R = OracleIntersector(v, f, 1)
    box = R.mesh_aabb
    for d in directions:
        got = points_sim.contains(B, p, d, box)
        dirs = np.tile(d, (len(p), 1))
        cp, cm = R.intersects_count(p, dirs), R.intersects_count(p, -dirs)
        assert np.array_equal(got["counts"], np.stack([cp, cm])), what
        odd = (cp & 1).astype(bool) & (cm & 1).astype(bool)
        in_box = (p > box[0]).all(1) & (p < box[1]).all(1)
        assert np.array_equal(got["inside"], in_box & odd), what
        assert np.array_equal(got["broken"], ~odd & ((cp == 0) | (cm == 0))), what
        assert got["summary"].tolist() == [int(in_box.sum()), int(got["broken"].sum())], what
        # the reference's control flow on these flags is the oracle's contains_points with the same explicit direction
        want = R.contains_points(p, d)
        if not in_box.any() or got["broken"].any():
            assert not want.any(), what                      # nothing in the box / the all-False quirk
        else:
            assert np.array_equal(got["inside"], want), what
        # no box: every point passes the box test
        free = points_sim.contains(B, p, d, None)
        assert np.array_equal(free["inside"], odd) and int(free["summary"][0]) == len(p), what
    assert got["inside"].any() or what == "soup"


def test_host_routine_on_meshes_without_a_hierarchy_and_on_invalid_points():
    import points_sim
    from sim import SimBVH
    v, f = W.two_triangles()
    p = np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.0, 0.0, -1.5], [np.nan, 0.0, -0.5], [np.inf, 0.0, 0.0], [3.0, 3.0, 3.0]], np.float32)
    d = np.array([0.0, 0.0, 1.0], np.float32)
    dirs = np.tile(d, (len(p), 1))
    for nt in (2, 1):
        B = SimBVH(v[:3 * nt], f[:nt])
        R = OracleIntersector(v[:3 * nt], f[:nt], 1)
        got = points_sim.contains(B, p, d, R.mesh_aabb)
        assert np.array_equal(got["counts"], np.stack([R.intersects_count(p, dirs), R.intersects_count(p, -dirs)])), nt
        assert got["counts"][:, 3:5].sum() == 0               # non-finite rays count nothing
        assert not got["inside"][3:].any()                    # a NaN is in no box
    assert got["counts"][:, 1].tolist() == [0, 1]             # above the one triangle: only the ray downwards meets it
