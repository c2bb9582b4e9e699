"""CPU checks of libtriro_within.so (include/triro_within.h, csrc/within.hip, csrc/tr_within.h): the library is built and
exports what its header declares, the ctypes table covers the header, its code object holds exactly the shipped kernels
without scratch or spills, and the core built for the host (tests/host_sim/within_sim.cpp):
  * the walks over a hierarchy (any, count, fill + ordering, bounded nearest) return the bits of the brute force over the
    per-triangle function, at every radius and stack limit (the overflow path included), on meshes with exact ties, zero-area
    triangles, 3 000 coincident triangles under a hierarchy of more than 32 levels, and without a hierarchy;
  * identities that need no reference; the bounded nearest against closest_point's brute force on float64 d2;
  * on the cube lattice, where every d2 is exact, sets and counts against a reference in fractions.Fraction, faces at exactly
    r included;
  * on icosphere and soup, the lists against an independent numpy float64 evaluation within a tolerance that comes from the
    number formats;
  * invalid queries and inactive triangles."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hostile_meshes as M
import nearest_cases as NC
import within_cases as WC
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_within.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BRUTE = "test_gpu_within.py::test_kernels_match_the_brute_force_at_every_stack_limit"
TAILS = "test_gpu_within.py::test_tails_of_the_lane_and_block_indexing"
HOSTILE = "test_gpu_within.py::test_hostile_points_and_radii"
MISUSE = "test_gpu_within.py::test_fill_with_counts_of_a_smaller_radius_stays_inside_its_rows"
# one row per kernel of libtriro_within.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "void k_within<0>": (BRUTE, TAILS, HOSTILE),
    "void k_within<1>": (BRUTE, TAILS, HOSTILE),
    "void k_within<2>": (BRUTE, TAILS, HOSTILE, MISUSE),
    "k_within_rows": (BRUTE, TAILS, MISUSE),
    "k_within_closest": (BRUTE, TAILS, HOSTILE),
}
SET_KERNELS = ("void k_within<0>", "void k_within<1>", "void k_within<2>")
SYMBOLS = ["tr_within_abi_version", "tr_within_any", "tr_within_closest", "tr_within_count", "tr_within_fill", "tr_within_stack_capacity"]


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.within_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_within.h but not exported"
    assert set(hops.WITHIN_ABI) == set(syms)


def test_abi_version_and_stack_capacity_match_the_sources():
    import within_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_WITHIN_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.WITHIN_ABI_VERSION == want
    lib = hops.get_within_module()
    assert lib.tr_within_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_within.h")).read()
    cap = int(re.search(r"#define\s+TR_WITHIN_STACK\s+(\d+)", core).group(1))
    assert lib.tr_within_stack_capacity() == cap == within_sim.stack_capacity() == 32
    for name, nargs in (("tr_within_any", 8), ("tr_within_count", 8), ("tr_within_fill", 14), ("tr_within_closest", 10)):
        res, args = hops.WITHIN_ABI[name]
        assert len(args) == nargs and args[2] is ctypes.c_int64 and args[4] is ctypes.c_float and args[-2] is ctypes.c_int, name
    assert hops.WITHIN_ABI["tr_within_fill"][1][7] is ctypes.c_int64
    # tr_within.h includes tr_nearest.h and adds nothing to it: the shared header is the parent's, and no other header changed
    assert '#include "tr_nearest.h"' in core


def test_libtriro_hip_and_libtriro_nearest_gained_no_symbol():
    import triro.backend.ops as hops
    hip = ctypes.CDLL(hops.library_path())
    near = ctypes.CDLL(hops.nearest_library_path())
    for s in header_symbols():
        assert not hasattr(hip, s), s
        assert not hasattr(near, s), s
    text = open(os.path.join(ROOT, "include", "triro_hip.h")).read()
    assert set(hops.ABI) == set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_header_is_strict_c99():
    src = '#include "triro_within.h"\nint main(void) { return TR_WITHIN_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_within_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_within_stack_capacity()
    ncap = hops.get_nearest_module().tr_nearest_stack_capacity()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.addressof(fake)
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    big = (1 << 31) * 128
    # any / count: (bvh, points, n, radii, radius, out, stack_entries, stream)
    for fn in (lib.tr_within_any, lib.tr_within_count):
        assert fn(None, None, 0, None, 1.0, None, 0, None) == 1 and b"bvh" in err()
        assert fn(h, out, -1, None, 1.0, out, 0, None) == 1 and b"n < 0" in err()
        assert fn(h, out, 1, None, 1.0, out, cap + 1, None) == 1 and b"stack_entries" in err()
        assert fn(h, out, 1, None, 1.0, out, -1, None) == 1 and b"stack_entries" in err()
        assert fn(h, None, 1, None, 1.0, out, 0, None) == 1 and b"null" in err()
        assert fn(h, out, 1, out, 1.0, None, 0, None) == 1 and b"null" in err()
        assert fn(h, out, big, None, 1.0, out, 0, None) == 1 and b"too many" in err()
        assert fn(h, None, 0, None, 1.0, None, cap, None) == 0
    # fill: (bvh, points, n, radii, radius, count, offsets, total, face, distance, closest, slot, stack_entries, stream)
    fill = lib.tr_within_fill
    assert fill(None, None, 0, None, 1.0, None, None, 0, None, None, None, None, 0, None) == 1 and b"bvh" in err()
    assert fill(h, out, -1, None, 1.0, out, out, 1, out, None, None, None, 0, None) == 1 and b"n < 0" in err()
    assert fill(h, out, 1, None, 1.0, out, out, 1, out, None, None, None, cap + 1, None) == 1 and b"stack_entries" in err()
    assert fill(h, out, 1, None, 1.0, out, out, 1, out, None, None, None, -1, None) == 1 and b"stack_entries" in err()
    assert fill(h, out, 1, None, 1.0, out, out, -1, out, None, None, None, 0, None) == 1 and b"total < 0" in err()
    assert fill(h, None, 1, None, 1.0, out, out, 1, out, None, None, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, 1, None, 1.0, None, out, 1, out, None, None, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, 1, None, 1.0, out, None, 1, out, None, None, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, 1, None, 1.0, out, out, 1, None, None, None, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, 1, None, 1.0, out, out, 1, out, out, None, None, 0, None) == 1 and b"d_slot" in err()      # rows to evaluate, no scratch
    assert fill(h, out, 1, None, 1.0, out, out, 1, out, None, out, None, 0, None) == 1 and b"d_slot" in err()
    assert fill(h, out, big, None, 1.0, out, out, 1, out, None, None, None, 0, None) == 1 and b"too many" in err()
    assert fill(h, None, 0, None, 1.0, None, None, 0, None, None, None, None, cap, None) == 0
    assert fill(h, out, 1, None, 1.0, out, out, 0, None, None, None, None, 0, None) == 0          # no rows: nothing to launch
    # bounded nearest: (bvh, points, n, radii, radius, closest, distance, tri, stack_entries, stream); capacity of the nearest walk
    cl = lib.tr_within_closest
    assert cl(None, None, 0, None, 1.0, None, None, None, 0, None) == 1 and b"bvh" in err()
    assert cl(h, out, -1, None, 1.0, out, out, out, 0, None) == 1 and b"n < 0" in err()
    assert cl(h, out, 1, None, 1.0, out, out, out, ncap + 1, None) == 1 and b"stack_entries" in err()
    assert cl(h, out, 1, None, 1.0, out, out, out, -1, None) == 1 and b"stack_entries" in err()
    assert cl(h, None, 1, None, 1.0, out, out, out, 0, None) == 1 and b"null" in err()
    assert cl(h, out, 1, None, 1.0, out, out, None, 0, None) == 1 and b"null" in err()
    assert cl(h, out, big, None, 1.0, out, out, out, 0, None) == 1 and b"too many" in err()
    assert cl(h, None, 0, None, 1.0, None, None, None, ncap, None) == 0


# ---- 2. the code object ----------------------------------------------------------------------------------------------
def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.within_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_within_module().tr_within_stack_capacity()
    ncap = hops.get_nearest_module().tr_nearest_stack_capacity()
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
        # the stack: capacity node ids (set kernels) or {node, bound} entries (bounded nearest) for 128 lanes, and nothing else;
        # the ordering pass has no stack
        want_lds = cap * 4 * 128 if name in SET_KERNELS else (ncap * 8 * 128 if name == "k_within_closest" else 0)
        assert k["lds"] == want_lds, k
        assert k["vgpr"] <= 168, k          # registers must not limit occupancy below three waves per SIMD
    # libtriro_nearest.so keeps exactly its one kernel
    assert {k["name"] for k in con.kernels(hops.nearest_library_path())} == {"k_closest_point"}


# ---- 3. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute_results():
    """{case: (v, f, p, [(label, radius, brute force)])}, computed once"""
    import within_sim
    out = {}
    for name, make in WC.CASES.items():
        v, f, p = make()
        out[name] = (v, f, p, [(label, r, within_sim.brute(v, f, p, r)) for label, r in WC.radii(v, len(p))])
    return out


@pytest.mark.parametrize("name", list(WC.CASES))
def test_host_walks_match_the_brute_force_bit_for_bit(name, brute_results):
    import within_sim
    from sim import SimBVH
    v, f, p, rows = brute_results[name]
    B = SimBVH(v, f)
    if name == "deep":
        assert B.depth > 32
    for label, r, want in rows:
        for entries in (1, 2, 3, 32):
            got, lost = within_sim.walk(B, p, r, entries, want_lost=True)
            WC.assert_same(got, want, f"{name}, r = {label}, stack_entries {entries}")
            if entries == 1 and label == "+Inf":
                assert lost.all(), f"{name}: a stack of one entry did not overflow on every walk of the whole tree"
        if label == "+Inf":
            n_active = int(NC.active(v, f).sum())
            assert (want.count == n_active).all() and n_active == len(f)
            assert np.array_equal(want.faces.reshape(len(p), -1), np.tile(np.arange(len(f), dtype=np.int32), (len(p), 1)))
    if name == "deep":
        # 3 000 coincident triangles: at r = 0 the point on the pile lists all of them, in order
        zero = rows[0][2]
        first = len(f) - 3000
        mine = zero.faces[zero.offsets[190]:zero.offsets[191]]
        assert zero.count[190] >= 3000 and np.array_equal(mine[-3000:], np.arange(first, len(f)))


def test_meshes_without_a_hierarchy():
    import within_sim
    from sim import SimBVH
    v, f = W.two_triangles()
    p = np.concatenate([NC.hash_points(60, 5, [-0.8, -0.8, -1.4], [0.8, 0.8, 0.4]),
                        np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.5, -0.5, 0.0], [0.0, 0.5, -2.0]], np.float32)])
    for nt in (2, 1):
        vv, ff = v[:3 * nt], f[:nt]
        seen = set()
        for label, r in WC.radii(v, len(p)):
            want = within_sim.brute(vv, ff, p, r)
            WC.check_identities(want, f"{nt} triangle(s), r = {label}")
            seen |= set(np.unique(want.count))
            for entries in (1, 0):
                WC.assert_same(within_sim.walk(SimBVH(vv, ff), p, r, entries), want, f"{nt} triangle(s), r = {label}")
        assert seen == set(range(nt + 1))
    # zero triangles: every point is answered with the miss values
    empty = SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32)))
    for got in (within_sim.walk(empty, p, np.inf), within_sim.brute(v[:0], f[:0], p, np.inf)):
        assert not got.any.any() and not got.count.any() and len(got.faces) == 0 and got.offsets[-1] == 0
        assert (got.nearest[2] == -1).all() and np.isposinf(got.nearest[1]).all() and np.isnan(got.nearest[0]).all()


# ---- 4. identities on the brute force ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WC.CASES))
def test_identities_of_the_brute_force(name, brute_results):
    import nearest_sim
    v, f, p, rows = brute_results[name]
    unbounded = nearest_sim.brute(v, f, p)
    # closest_point's float64 d2: the brute force with r = +Inf reports it
    d2 = dict((label, res) for label, _, res in rows)["+Inf"].nearest[3]
    NC.assert_same_bits(dict((label, res) for label, _, res in rows)["+Inf"].nearest[:3], unbounded, f"{name}: r = +Inf is closest_point")
    previous = None
    for label, r, res in rows:
        WC.check_identities(res, f"{name}, r = {label}")
        r32 = within_sim_radii(r, len(p))
        R2 = r32.astype(np.float64) ** 2
        keep = d2 <= R2
        c, d, t = res.nearest[:3]
        NC.assert_same_bits((c[keep], d[keep], t[keep]), tuple(x[keep] for x in unbounded), f"{name}, r = {label}: bounded == unbounded where d2 <= R2")
        assert (t[~keep] == -1).all() and np.isposinf(d[~keep]).all() and np.isnan(c[~keep]).all(), f"{name}, r = {label}: misses"
        if label not in ("+Inf", "per point"):
            assert keep.any() or r == 0, f"{name}, r = {label}"
            if previous is not None:
                assert (res.count >= previous).all(), f"{name}: counts are not monotone in r"
            previous = res.count
        # a row is a pure function of (p, face): the rows of the same pair at r = +Inf
        if label != "+Inf":
            full = dict((lb, rs) for lb, _, rs in rows)["+Inf"]
            pt = np.repeat(np.arange(len(p)), res.count)
            at = full.offsets[pt] + res.faces          # (+Inf lists every face: row = offset + face)
            assert np.array_equal(NC.bits(res.distance), NC.bits(full.distance[at])) and np.array_equal(NC.bits(res.closest), NC.bits(full.closest[at]))
    # the float32 distance does not decide: the identity above is stated on d2


def within_sim_radii(r, n):
    import within_sim
    return within_sim.radii(r, n)


# ---- 5. exact ties: the cube lattice against exact rational arithmetic ------------------------------------------------------
def test_cube_lattice_sets_match_an_exact_reference():
    import within_sim
    from sim import SimBVH
    v, f, _ = NC.cube()
    at = WC.check_cube_lattice(lambda p, r: within_sim.brute(v, f, p, r), "brute force")
    print("pairs at distance exactly r, r = 0, 1/4, 1/2, 1:", at)
    assert at == [540, 540, 540, 540]
    B = SimBVH(v, f)
    WC.check_cube_lattice(lambda p, r: within_sim.walk(B, p, r, 2), "host walk, two stack entries")


# ---- 6. the independent tolerance check -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "soup"])
def test_lists_agree_with_an_independent_numpy_evaluation(name, brute_results):
    v, f, p, rows = brute_results[name]
    ext = WC.extent(v)
    by_radius = {float(r): res for label, r, res in rows if np.ndim(r) == 0}
    for fr in WC.TOLERANCE_FRACTIONS:
        r = np.float32(fr * ext)
        within, band = WC.check_tolerance(v, f, p, r, by_radius[float(r)], f"{name}, {fr:g} of the extent")
        assert within > 100


# ---- 7. invalid queries ------------------------------------------------------------------------------------------------------
def hostile_queries():
    """(points [n, 3], radii [n], valid [n]): hostile radii on ordinary points, then hostile points at an ordinary radius"""
    ordinary = NC.hash_points(64, 17, [-1.3] * 3, [1.3] * 3)
    with np.errstate(over="ignore"):
        bad_r = np.array([np.nan, -1.0, -np.inf, -1e-45, -0.0, np.inf, 1e-45, 1e-39, 3e38, 0.0, 0.5, 3.4028235e38], np.float32)
    p = ordinary.copy()
    r = np.full(len(p), 0.75, np.float32)
    r[:len(bad_r)] = bad_r
    k = 20
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p[k, axis] = bad
            k += 1
    p[30] = [3e38, 3e38, 3e38]; p[31] = [-3e38, 0.1, 3e38]; p[32] = [0, 0, -3e38]; p[33] = [2.0 ** 60, 0, 0]
    p[34] = [1e-45, -1e-40, 3e-39]; p[35] = [0, 0, 0]
    r[30:34] = [np.inf, 3e38, 3e38, 2.0 ** 61]
    valid = np.isfinite(p).all(1) & (r >= 0)
    return p, r, valid


def test_invalid_queries_write_the_miss_values():
    import within_sim
    from sim import SimBVH
    v, f, _ = NC.icosphere()
    p, r, valid = hostile_queries()
    assert (~valid).sum() == 4 + 9 and valid[4] and valid[5]          # -0.0 and +Inf are valid radii
    want = within_sim.brute(v, f, p, r)
    WC.check_identities(want, "hostile queries")
    for entries in (1, 0):
        WC.assert_same(within_sim.walk(SimBVH(v, f), p, r, entries), want, f"hostile queries, stack_entries {entries}")
    c, d, t, _ = want.nearest
    assert not want.any[~valid].any() and not want.count[~valid].any()
    assert (t[~valid] == -1).all() and np.isposinf(d[~valid]).all() and np.isnan(c[~valid]).all()
    assert want.count[5] == len(f) and want.count[8] == len(f) and want.count[11] == len(f)      # +Inf, 3e38, FLT_MAX: every face
    assert want.count[4] == 0 and want.count[6] == 0 and want.count[9] == 0                      # -0.0, denormal, 0: nothing that near
    # r = 3e38 keeps R2 finite in float64: a point at 3e38 on every axis is 5.2e38 from the sphere, beyond it, and found by +Inf
    assert np.isfinite(np.float64(np.float32(3e38)) ** 2)
    assert want.count[30] == len(f) and want.count[31] == 0 and want.count[32] == len(f) and want.count[33] == len(f)
    assert np.isposinf(d[30]) and t[30] >= 0                         # within +Inf, its distance beyond the float range


# ---- 8. inactive triangles ----------------------------------------------------------------------------------------------------
HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_inactive_triangles_are_never_listed_and_never_counted(name, seed):
    import within_sim
    from sim import SimBVH
    c = M.case(name, seed)
    fa, new = M.active_faces(c.v, c.f)
    B = SimBVH(c.v, c.f) if len(c.f) else None
    ext = WC.extent(c.v[np.unique(fa)]) if len(fa) else 1.0
    for r in (np.float32(0.25 * ext), np.float32(np.inf), WC.hashed_radii(len(c.p), 2 * ext, seed=3)):
        want = within_sim.brute(c.v, c.f, c.p, r)
        WC.check_identities(want, c.name)
        assert not c.inactive[want.faces].any(), f"{c.name}: an inactive triangle is listed"
        if np.ndim(r) == 0 and np.isinf(r):
            assert (want.count == len(fa)).all()
        # the same mesh without its inactive faces answers the same, up to the renumbering of the faces
        alone = within_sim.brute(c.v, fa, c.p, r)
        assert np.array_equal(want.count, alone.count) and np.array_equal(M.map_ids(want.faces, new), alone.faces)
        assert np.array_equal(NC.bits(want.distance), NC.bits(alone.distance)) and np.array_equal(NC.bits(want.closest), NC.bits(alone.closest))
        assert np.array_equal(M.map_ids(want.nearest[2], new), alone.nearest[2])
        if B is not None:
            for entries in (1, 0):
                WC.assert_same(within_sim.walk(B, c.p, r, entries), want, f"{c.name}, stack_entries {entries}")
