"""CPU checks of libtriro_range.so (include/triro_range.h, csrc/range.hip, csrc/tr_range.h): the library is built and exports
what its header declares, the ctypes table covers the header, its code object holds exactly the two instantiations of
k_range_query without scratch or spills, and the core built for the host (tests/host_sim/range_sim.cpp):
  * the walk over a hierarchy returns the bits of the brute force over the per-triangle predicate, at every stack limit
    (the overflow path included), on an icosphere, on five nested shells and on a hierarchy of more than 32 levels;
  * the brute force agrees with the oracle's multi-hit list filtered by tmin <= t <= tmax, outside the band around a bound
    where the contract's float64 decision may differ from a float32 comparison;
  * with default bounds the brute force IS the old contract on every ray the old contract does not anchor;
  * on a scene whose hit distances are exact, the interval is closed to the last ulp at both ends."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import range_cases as RC
import workloads as W
from oracle.oracle import OracleIntersector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_range.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# one row per kernel of libtriro_range.so: the GPU tests that launch it and compare it with the brute force
_TESTS = ("test_gpu_range.py::test_meshes_at_every_stack_limit",
          "test_gpu_range.py::test_tails_of_the_lane_and_block_indexing",
          "test_gpu_range.py::test_exact_bounds_on_the_sheet_scene",
          "test_gpu_range.py::test_hostile_rays_and_bounds")
INVENTORY = {
    "void k_range_query<0>": _TESTS,      # TR_Q_ANY
    "void k_range_query<2>": _TESTS,      # TR_Q_CLOSEST
}


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. plumbing -------------------------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.range_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == ["tr_range_abi_version", "tr_range_any", "tr_range_closest", "tr_range_stack_capacity"]
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_range.h but not exported"
    assert set(hops.RANGE_ABI) == set(syms)
    hip = ctypes.CDLL(hops.library_path())
    for s in syms:
        assert not hasattr(hip, s), f"libtriro_hip.so gained {s}"


def test_abi_version_and_stack_capacity_match_the_sources():
    import range_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_RANGE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.RANGE_ABI_VERSION == want
    lib = hops.get_range_module()
    assert lib.tr_range_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_range.h")).read()
    cap = int(re.search(r"#define\s+TR_RANGE_STACK\s+(\d+)", core).group(1))
    assert lib.tr_range_stack_capacity() == cap == range_sim.stack_capacity() == 32
    assert len(hops.RANGE_ABI["tr_range_any"][1]) == 7 and len(hops.RANGE_ABI["tr_range_closest"][1]) == 12


def test_the_header_is_strict_c99():
    src = '#include "triro_range.h"\nint main(void) { return TR_RANGE_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_range_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_range_stack_capacity()
    h = ctypes.addressof(ctypes.create_string_buffer(4096))
    out = ctypes.addressof(ctypes.create_string_buffer(64))

    def rays(n, shape=None, o=out, d=out):
        r = hops.TrRays()
        r.d_origins, r.d_directions, r.nray = o, d, n
        r.shape = (ctypes.c_int64 * 4)(*(shape or [hops._INT64_MAX, hops._INT64_MAX, n, 3]))
        r.ostride = (ctypes.c_int64 * 4)(0, 0, 3, 1)
        r.dstride = (ctypes.c_int64 * 4)(0, 0, 3, 1)
        return ctypes.byref(r)

    def both(bvh, r, required, entries):
        """(status of tr_range_any, status of tr_range_closest) with `required` as the one required output"""
        a = lib.tr_range_any(bvh, r, None, None, required, entries, None)
        ea = err()
        c = lib.tr_range_closest(bvh, r, None, None, required, out, out, out, out, out, entries, None)
        return a, c, ea + b" | " + err()

    for args, word in (((None, rays(1), out, 0), b"bvh"), ((h, None, out, 0), b"rays"), ((h, rays(-1), out, 0), b"nray < 0"),
                       ((h, rays(1, [hops._INT64_MAX, hops._INT64_MAX, 2, 3]), out, 0), b"product"),
                       ((h, rays(1, o=None), out, 0), b"null"), ((h, rays(1, d=None), out, 0), b"null"),
                       ((h, rays(1), None, 0), b"null"), ((h, rays(1), out, cap + 1), b"stack_entries"), ((h, rays(1), out, -1), b"stack_entries"),
                       ((h, rays((1 << 31) * 128), out, 0), b"too many")):
        a, c, msg = both(*args)
        assert a == 1 and c == 1 and msg.count(word) == 2, (word, a, c, msg)
    # nothing to do is no error, with or without the outputs
    assert both(h, rays(0, o=None, d=None), None, cap)[:2] == (0, 0)
    # the optional outputs of tr_range_closest are optional: only d_tri is required
    assert lib.tr_range_closest(h, rays(0), None, None, None, None, None, None, None, None, 0, None) == 0


def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.range_library_path())}
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
        # the far-child stack: capacity entries of {node, entry distance} for 128 lanes, and nothing else
        assert k["lds"] == hops.get_range_module().tr_range_stack_capacity() * 8 * 128, k
        assert k["vgpr"] <= 168, k          # 32 KB of LDS allow five workgroups = ten waves per CU: registers must not limit it further


# ---- 2. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """(vertices, faces, origins, directions, tmin, tmax, brute force) of every mesh, computed once"""
    import range_sim
    out = {}
    for name, make in RC.MESHES.items():
        v, f, o, d, lo, hi = make()
        out[name] = (v, f, o, d, lo, hi, range_sim.brute(v, f, o, d, lo, hi))
    return out


@pytest.mark.parametrize("name", list(RC.MESHES))
def test_host_walk_matches_the_brute_force_bit_for_bit(name, cases):
    import range_sim
    from sim import SimBVH
    v, f, o, d, lo, hi, want = cases[name]
    assert len(o) == 20000 and (o >= v.min(0)).all() and (o <= v.max(0)).all()
    assert (0 <= lo).all() and (lo <= hi).all() and (hi <= np.float32(1.5 * RC.extent(v))).all()
    B = SimBVH(v, f)
    if name == "deep":
        assert B.depth > 32
    assert want["hit"].sum() > 100 and (~want["hit"]).sum() > 100, name
    for entries in (0, 1, 2, 3):
        got = range_sim.walk(B, o, d, lo, hi, entries)
        RC.assert_same_bits(got, want, f"{name}, stack_entries {entries}")
        print(f"{name}, stack_entries {entries}: overflowed walks any {int(got['lost_any'].sum())}, closest {int(got['lost'].sum())}")
        if entries == 1:
            assert got["lost"].any() and got["lost_any"].any(), f"{name}: a stack of one entry never overflowed: the second walk was not exercised"
        if entries == 0:
            assert not got["lost"].any() and not got["lost_any"].any(), name


def test_meshes_without_a_hierarchy():
    import range_sim
    from sim import SimBVH
    v, f = W.two_triangles()
    o, d = W.hash_rays(400, 5, [-0.6, -0.6, -1.5], [0.6, 0.6, 0.5])
    d[:, 2] = np.abs(d[:, 2]) * np.sign(-0.5 - o[:, 2])      # towards the plane between the two triangles
    lo, hi = RC.hash_bounds(400, 6, 3.0)
    for nt in (2, 1):
        vv, ff = v[:3 * nt], f[:nt]
        want = range_sim.brute(vv, ff, o, d, lo, hi)
        assert want["hit"].any() and not want["hit"].all()
        for entries in (1, 0):
            RC.assert_same_bits(range_sim.walk(SimBVH(vv, ff), o, d, lo, hi, entries), want, f"{nt} triangle(s)")
    empty = SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32)))
    for got in (range_sim.walk(empty, o, d, lo, hi), range_sim.brute(v[:0], f[:0], o, d, lo, hi)):
        assert not got["any"].any() and not got["hit"].any() and (got["tri"] == -1).all() and np.isposinf(got["t"]).all()


# ---- 3. brute force == the oracle's filtered list ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "shells5"])
def test_brute_force_matches_the_oracles_filtered_hit_list(name, cases):
    v, f, o, d, lo, hi, got = cases[name]
    n = len(o)
    R = OracleIntersector(v, f, 1)
    loc, ray, tri, t = R.intersects_location(o, d, with_t=True, cap=32)
    count = R.intersects_count(o, d)
    anchored = (R.anchor(o, d) != o).any(1)
    many = count > 32
    # a listed t within 2^-9 relative of a bound: there the contract's float64 decision may differ from the oracle's float32 t
    near = (np.abs(t - lo[ray]) <= lo[ray] * np.float32(2.0 ** -9)) | (np.abs(t - hi[ray]) <= hi[ray] * np.float32(2.0 ** -9))
    band = np.zeros(n, bool)
    band[ray[near]] = True
    left_out = anchored | many | band
    print(f"{name}: left out {left_out.mean():.4%} (anchored {int(anchored.sum())}, more than 32 hits {int(many.sum())}, in the band {int(band.sum())}); "
          f"largest hit count {int(count.max())}")
    assert left_out.mean() <= 0.01
    inside = (t >= lo[ray]) & (t <= hi[ray])
    # the list is ordered by (ray, t): the first in-range entry of a ray is its closest
    assert (np.diff(ray) >= 0).all()
    idx = np.flatnonzero(inside)
    first = np.full(n, -1, np.int64)
    first[ray[idx][::-1]] = idx[::-1]
    hit = first >= 0
    only_out = ~hit & (count > 0)
    print(f"{name}: a hit in range {hit.mean():.2%}, a hit only out of range {only_out.mean():.2%}")
    assert hit.mean() >= 0.20 and only_out.mean() >= 0.20
    keep = ~left_out
    assert np.array_equal(got["any"][keep], hit[keep]) and np.array_equal(got["hit"][keep], hit[keep])
    k = keep & hit
    assert np.array_equal(got["tri"][k], tri[first[k]])
    assert np.array_equal(RC.bits(got["t"][k]), RC.bits(t[first[k]]))
    assert np.array_equal(RC.bits(got["loc"][k]), RC.bits(loc[first[k]]))
    assert (got["tri"][keep & ~hit] == -1).all() and np.isposinf(got["t"][keep & ~hit]).all()
    # where the in-range closest is the oracle's closest of the whole ray: front and uv, too
    c_hit, c_front, c_tri, c_loc, c_uv, c_t = R.closest_raw(o, d)
    same = k & c_hit & (c_tri == got["tri"])
    assert same.sum() > 0.05 * n
    assert np.array_equal(got["front"][same], c_front[same]) and np.array_equal(RC.bits(got["uv"][same]), RC.bits(c_uv[same]))


@pytest.mark.parametrize("name", ["icosphere", "shells5"])
def test_default_bounds_are_the_old_contract_on_every_ray(name, cases):
    import range_sim
    v, f, o, d, _, _, _ = cases[name]
    R = OracleIntersector(v, f, 1)
    assert not (R.anchor(o, d) != o).any()          # origins in the box: nothing is anchored
    got = range_sim.brute(v, f, o, d)
    hit, front, tri, loc, uv, t = R.closest_raw(o, d)
    assert hit.sum() > 1000
    assert np.array_equal(got["any"], R.intersects_count(o, d) > 0) and np.array_equal(got["count"], R.intersects_count(o, d))
    assert np.array_equal(got["hit"], hit) and np.array_equal(got["front"], front) and np.array_equal(got["tri"], tri)
    assert np.array_equal(RC.bits(got["loc"]), RC.bits(loc)) and np.array_equal(RC.bits(got["uv"]), RC.bits(uv))
    assert np.array_equal(RC.bits(got["t"][hit]), RC.bits(t[hit])) and np.isposinf(got["t"][~hit]).all()
    # explicit bounds that are no restriction are the defaults
    RC.assert_same_bits(range_sim.brute(v, f, o, d, -1.0, np.inf), got, "(-1, +Inf)")
    RC.assert_same_bits(range_sim.brute(v, f, o, d, 0.0, 1e7), got, "(0, 1e7)")


# ---- 4. exact bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["interior", "diagonal", "vertex"])
def test_exact_bounds_on_the_sheet_scene(kind):
    import range_sim
    from sim import SimBVH
    v, f = RC.sheets()
    o, d, lo, hi, first, count = RC.sheet_cases(kind)
    res = range_sim.brute(v, f, o, d, lo, hi, cap=16)
    RC.check_sheet_results(res, first, count, kind)
    assert (first > 0).sum() > 100 and (first == 0).sum() > 100
    for entries in (0, 1):
        RC.assert_same_bits(range_sim.walk(SimBVH(v, f), o, d, lo, hi, entries), res, f"sheets, {kind}, stack_entries {entries}")


# ---- 5. segments -------------------------------------------------------------------------------------------------------
def test_segments_are_rays_with_the_float32_difference_and_the_range_0_1():
    import range_sim
    v, f = RC.sheets()
    xy = RC.sheet_origins("interior")
    p0 = xy.copy()
    p0[:, 2] = np.float32(0.25)      # (every difference below is exact in float32)
    rows = []
    for k in range(1, RC.SHEETS + 1):
        on = p0.copy()
        on[:, 2] = np.float32(k)                                      # p1 exactly on sheet k: blocked, at the far end
        short = p0.copy()
        short[:, 2] = np.nextafter(np.float32(k), np.float32(0))      # one ulp short of it
        rows.append((k, on, short))
    for k, on, short in rows:
        o, d, lo, hi = RC.segment_rays(p0, on)
        assert (d[:, 2] == np.float32(k - 0.25)).all()
        res = range_sim.brute(v, f, o, d, lo, hi)
        assert res["any"].all() and (res["count"] == k).all() and (res["tri"] // RC.TRIS_PER_SHEET == 0).all()
        o, d, lo, hi = RC.segment_rays(p0, short)
        res = range_sim.brute(v, f, o, d, lo, hi)
        assert (res["count"] == k - 1).all() and np.array_equal(res["any"], np.full(len(o), k > 1))
        if k > 1:
            assert ((res["t"] > 0) & (res["t"] < 1)).all()
    # a segment that ends on the first sheet: the hit is at t = 1, the closed end
    o, d, lo, hi = RC.segment_rays(p0, rows[0][1])
    res = range_sim.brute(v, f, o, d, lo, hi)
    assert (res["t"] == 1.0).all() and (res["loc"][:, 2] == 1.0).all()
    # the reversed segment starts on the sheet: the closed start
    o, d, lo, hi = RC.segment_rays(rows[0][1], p0)
    res = range_sim.brute(v, f, o, d, lo, hi)
    assert (res["t"] == 0.0).all() and res["any"].all()


# ---- 6. hostile rays and bounds ----------------------------------------------------------------------------------------
def test_hostile_rays_and_bounds_miss_by_rule_on_the_host(cases):
    import range_sim
    from sim import SimBVH
    v, f = cases["icosphere"][:2]
    o, d, lo, hi, bad = RC.hostile_rays(*cases["icosphere"][2:6])
    want = range_sim.brute(v, f, o, d, lo, hi)
    RC.check_miss_rule(want, bad, "brute force")
    assert want["hit"][~bad].sum() > 50 and not want["hit"][110]
    for entries in (0, 1):
        RC.assert_same_bits(range_sim.walk(SimBVH(v, f), o, d, lo, hi, entries), want, f"hostile rays, stack_entries {entries}")
