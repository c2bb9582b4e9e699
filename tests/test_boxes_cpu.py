"""CPU checks of libtriro_boxes.so (include/triro_boxes.h, csrc/boxes.hip, csrc/tr_boxes.h): the library is built and exports
what its header declares, the ctypes table covers the header, its code object holds exactly the shipped kernels without
scratch or spills, and the core built for the host (tests/host_sim/boxes_sim.cpp):
  * the walk over a hierarchy (any, count, fill + ordering) returns what the brute force over the predicate returns, for every
    set of boxes and stack limit (the overflow path included), on meshes with zero-area triangles, 3 000 coincident triangles
    under a hierarchy of more than 32 levels, and without a hierarchy;
  * on inputs snapped to k * 2^-10, |k| <= 2^12, where every float64 operation of the predicate is exact, the sets EQUAL an
    exact integer reference that is no separating-axis test (boxes_cases.exact_meets), pairs that only touch included;
  * identities that need no reference;
  * invalid boxes, +-FLT_MAX boxes and inactive triangles."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import boxes_cases as BC
import hostile_meshes as M
import nearest_cases as NC
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_boxes.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BRUTE = "test_gpu_boxes.py::test_kernels_match_the_brute_force_at_every_stack_limit"
TAILS = "test_gpu_boxes.py::test_tails_of_the_lane_and_block_indexing"
HOSTILE = "test_gpu_boxes.py::test_hostile_boxes"
MISUSE = "test_gpu_boxes.py::test_fill_with_counts_of_smaller_boxes_stays_inside_its_rows"
# one row per kernel of libtriro_boxes.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "void k_boxes<0>": (BRUTE, TAILS, HOSTILE),
    "void k_boxes<1>": (BRUTE, TAILS, HOSTILE),
    "void k_boxes<2>": (BRUTE, TAILS, HOSTILE, MISUSE),
    "k_boxes_rows": (BRUTE, TAILS, MISUSE),
}
WALK_KERNELS = ("void k_boxes<0>", "void k_boxes<1>", "void k_boxes<2>")
SYMBOLS = ["tr_boxes_abi_version", "tr_boxes_any", "tr_boxes_count", "tr_boxes_fill", "tr_boxes_stack_capacity"]


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.boxes_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_boxes.h but not exported"
    assert set(hops.BOXES_ABI) == set(syms)


def test_abi_version_and_stack_capacity_match_the_sources():
    import boxes_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_BOXES_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.BOXES_ABI_VERSION == want == 1
    lib = hops.get_boxes_module()
    assert lib.tr_boxes_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_boxes.h")).read()
    cap = int(re.search(r"#define\s+TR_BOXES_STACK\s+(\d+)", core).group(1))
    assert lib.tr_boxes_stack_capacity() == cap == boxes_sim.stack_capacity() == 32
    for name, nargs in (("tr_boxes_any", 7), ("tr_boxes_count", 7), ("tr_boxes_fill", 11)):
        res, args = hops.BOXES_ABI[name]
        assert len(args) == nargs and args[3] is ctypes.c_int64 and args[-2] is ctypes.c_int, name
    assert hops.BOXES_ABI["tr_boxes_fill"][1][6] is ctypes.c_int64
    # the row limit and the ordering are tr_walk.h's / tr_within.h's, included and not copied
    assert '#include "tr_within.h"' in core and "tr_within_sort(" in core and "tr_rows_limit(" in core
    assert not re.search(r"\btr_(within_sort|rows_limit|rows_sift|rows_sort|walk_push|walk_pop)\s*\([^;{]*\)\s*\{", core)


def test_the_other_libraries_gained_no_symbol():
    import triro.backend.ops as hops
    others = [hops.library_path(), hops.nearest_library_path(), hops.within_library_path()]
    for path in others:
        lib = ctypes.CDLL(path)
        for s in header_symbols():
            assert not hasattr(lib, s), (path, s)
    text = open(os.path.join(ROOT, "include", "triro_hip.h")).read()
    assert set(hops.ABI) == set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_header_is_strict_c99():
    src = '#include "triro_boxes.h"\nint main(void) { return TR_BOXES_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_boxes_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_boxes_stack_capacity()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.addressof(fake)
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    big = (1 << 31) * 128
    # any / count: (bvh, lo, hi, n, out, stack_entries, stream)
    for fn in (lib.tr_boxes_any, lib.tr_boxes_count):
        assert fn(None, None, None, 0, None, 0, None) == 1 and b"bvh" in err()
        assert fn(h, out, out, -1, out, 0, None) == 1 and b"n < 0" in err()
        assert fn(h, out, out, 1, out, cap + 1, None) == 1 and b"stack_entries" in err()
        assert fn(h, out, out, 1, out, -1, None) == 1 and b"stack_entries" in err()
        assert fn(h, None, out, 1, out, 0, None) == 1 and b"null" in err()
        assert fn(h, out, None, 1, out, 0, None) == 1 and b"null" in err()
        assert fn(h, out, out, 1, None, 0, None) == 1 and b"null" in err()
        assert fn(h, out, out, big, out, 0, None) == 1 and b"too many" in err()
        assert fn(h, None, None, 0, None, cap, None) == 0
    # fill: (bvh, lo, hi, n, count, offsets, total, face, inside, stack_entries, stream)
    fill = lib.tr_boxes_fill
    assert fill(None, None, None, 0, None, None, 0, None, None, 0, None) == 1 and b"bvh" in err()
    assert fill(h, out, out, -1, out, out, 1, out, None, 0, None) == 1 and b"n < 0" in err()
    assert fill(h, out, out, 1, out, out, 1, out, None, cap + 1, None) == 1 and b"stack_entries" in err()
    assert fill(h, out, out, 1, out, out, 1, out, None, -1, None) == 1 and b"stack_entries" in err()
    assert fill(h, out, out, 1, out, out, -1, out, None, 0, None) == 1 and b"total < 0" in err()
    assert fill(h, None, out, 1, out, out, 1, out, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, None, 1, out, out, 1, out, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, 1, None, out, 1, out, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, 1, out, None, 1, out, None, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, 1, out, out, 1, None, out, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, big, out, out, 1, out, None, 0, None) == 1 and b"too many" in err()
    assert fill(h, None, None, 0, None, None, 0, None, None, cap, None) == 0
    assert fill(h, out, out, 1, out, out, 0, None, None, 0, None) == 0          # no rows: nothing to launch


# ---- 2. the code object ----------------------------------------------------------------------------------------------
def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.boxes_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_boxes_module().tr_boxes_stack_capacity()
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
    # the libraries this one builds on keep exactly their kernels
    assert {k["name"] for k in con.kernels(hops.nearest_library_path())} == {"k_closest_point"}
    assert {k["name"] for k in con.kernels(hops.within_library_path())} == \
        {"void k_within<0>", "void k_within<1>", "void k_within<2>", "k_within_rows", "k_within_closest"}


# ---- 3. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute_results():
    """{case: (v, f, [(label, lo, hi, brute force)])}, computed once"""
    import boxes_sim
    out = {}
    for name, make in BC.CASES.items():
        v, f, p = make()
        out[name] = (v, f, [(label, lo, hi, boxes_sim.brute(v, f, lo, hi)) for label, lo, hi in BC.box_sets(v, p)])
    return out


@pytest.mark.parametrize("name", list(BC.CASES))
def test_host_walk_matches_the_brute_force(name, brute_results):
    import boxes_sim
    from sim import SimBVH
    v, f, rows = brute_results[name]
    B = SimBVH(v, f)
    if name == "deep":
        assert B.depth > 32
    overflowed = 0
    for label, lo, hi, want in rows:
        for entries in (1, 2, 32):
            got, lost = boxes_sim.walk(B, lo, hi, entries, want_lost=True)
            BC.assert_same(got, want, f"{name}, {label}, stack_entries {entries}")
            if label == "the whole mesh":
                # a walk of the whole tree pushes at every node with two internal children: one entry is lost on every
                # mesh here; the deep tree also loses entries at two
                assert entries != 1 or lost.all(), f"{name}: a stack of one entry did not overflow on the whole tree"
                overflowed += int(lost.sum()) if entries == 2 else 0
        if label == "the whole mesh":
            assert (want.count == len(f)).all() and want.inside.all()
            assert np.array_equal(want.faces.reshape(len(lo), -1), np.tile(np.arange(len(f), dtype=np.int32), (len(lo), 1)))
    if name == "deep":
        assert overflowed > 0, "deep: a stack of two entries never overflowed"


def test_meshes_without_a_hierarchy():
    import boxes_sim
    from sim import SimBVH
    v, f = W.two_triangles()
    p = np.concatenate([NC.hash_points(60, 5, [-0.8, -0.8, -1.4], [0.8, 0.8, 0.4]),
                        np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.5, -0.5, 0.0], [0.0, 0.5, -2.0]], np.float32)])
    for nt in (2, 1):
        vv, ff = v[:3 * nt], f[:nt]
        seen = set()
        for label, lo, hi in BC.box_sets(v, p):
            want = boxes_sim.brute(vv, ff, lo, hi)
            BC.check_identities(want, f"{nt} triangle(s), {label}")
            seen |= set(np.unique(want.count))
            for entries in (1, 0):
                BC.assert_same(boxes_sim.walk(SimBVH(vv, ff), lo, hi, entries), want, f"{nt} triangle(s), {label}")
        assert seen == set(range(nt + 1))
    # zero triangles: every box is answered with the miss values
    empty = SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32)))
    big = np.full((len(p), 3), 4.0, np.float32)
    for got in (boxes_sim.walk(empty, -big, big), boxes_sim.brute(v[:0], f[:0], -big, big)):
        assert not got.any.any() and not got.count.any() and len(got.faces) == 0 and len(got.inside) == 0 and got.offsets[-1] == 0


# ---- 4. exactness: snapped inputs against an exact integer reference -------------------------------------------------------
def test_snapped_inputs_equal_the_exact_reference():
    """coordinates k * 2^-10, |k| <= 2^12 (asserted by boxes_cases.snapped): differences <= 2^13, cross products <= 2^27, dots
    <= 2^42 grid units -- every float64 operation of the predicate is exact, so it must EQUAL the exact reference"""
    import boxes_sim
    from sim import SimBVH
    stats = BC.check_snapped(boxes_sim.brute, "brute force")
    print("(pairs, met, only touching) per mesh:", stats)
    assert all(t > 100 for _, _, t in stats.values())
    assert all(0 < met < pairs for pairs, met, _ in stats.values())
    BC.check_snapped(lambda v, f, lo, hi: boxes_sim.walk(SimBVH(v, f), lo, hi, 2), "host walk, two stack entries")


# ---- 5. identities on the brute force ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.CASES))
def test_identities_of_the_brute_force(name, brute_results):
    v, f, rows = brute_results[name]
    tv = v[f]                                                                   # [F, 3, 3]
    sizes = {}
    for label, lo, hi, res in rows:
        BC.check_identities(res, f"{name}, {label}")
        # inside is the exact comparison of the three vertices, and a face inside is in the list by construction: every row
        # of `inside` belongs to a listed face
        box = np.repeat(np.arange(len(lo)), res.count)
        t = tv[res.faces]
        want_inside = ((t >= lo[box][:, None, :]) & (t <= hi[box][:, None, :])).all(axis=(1, 2))
        assert np.array_equal(res.inside, want_inside), f"{name}, {label}: inside"
        # ... and every face with its three vertices in the box is met
        all_in = ((tv[None] >= lo[:, None, None, :]) & (tv[None] <= hi[:, None, None, :])).all(axis=(2, 3))
        assert BC.listed(res, len(lo), len(f))[all_in].all(), f"{name}, {label}: a face inside the box is not met"
        assert int(all_in.sum()) == int(res.inside.sum())
        sizes[label] = res
    # a box that holds another lists a superset
    small, large = sizes["half size 0.125 of the extent"], sizes["half size 0.5 of the extent"]
    assert (BC.listed(large, len(small.count), len(f)) >= BC.listed(small, len(small.count), len(f))).all()
    assert (sizes["half size 0.03125 of the extent"].count >= sizes["points"].count).all()
    whole = sizes["the whole mesh"]
    assert (whole.count == len(f)).all() and whole.inside.all()


# ---- 6. hostile boxes ------------------------------------------------------------------------------------------------------
def test_invalid_boxes_write_the_miss_values_and_flt_max_boxes_meet_everything():
    import boxes_sim
    from sim import SimBVH
    v, f, p = NC.icosphere()
    lo0, hi0 = BC.hashed_boxes(p[:96], BC.extent(v), seed=3)
    lo, hi, valid, whole = BC.hostile_boxes(lo0, hi0)
    assert (~valid).sum() == 18 + 6 and whole.sum() == 3 and valid[whole].all() and valid[27:31].all()
    want = boxes_sim.brute(v, f, lo, hi)
    BC.check_identities(want, "hostile boxes")
    for entries in (1, 0):
        BC.assert_same(boxes_sim.walk(SimBVH(v, f), lo, hi, entries), want, f"hostile boxes, stack_entries {entries}")
    assert not want.any[~valid].any() and not want.count[~valid].any()
    assert (want.count[whole] == len(f)).all()
    assert want.inside[want.offsets[24]:want.offsets[25]].all()                   # [-FLT_MAX, FLT_MAX]^3: every face inside
    assert want.count[27] == 0                                                    # the point at FLT_MAX
    assert want.count[28] >= 2 and want.count[30] == 0                             # the line along x through the sphere
    assert want.any[valid].sum() >= 10 and (~want.any[valid]).sum() >= 10


# ---- 7. inactive triangles ----------------------------------------------------------------------------------------------------
HOSTILE_MESHES = [(n, 0 if n in M.FAMILIES + ("deep_nan",) else None) for n in M.FAMILIES + ("deep_nan",) + M.SINGLE]


def hostile_mesh_boxes(c, fa):
    """[(lo, hi)] for a hostile mesh: hashed boxes around its points, and the box [-FLT_MAX, FLT_MAX]^3 for every point"""
    ext = BC.extent(c.v[np.unique(fa)]) if len(fa) else 1.0
    big = np.full((len(c.p), 3), BC.FLT_MAX, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return [BC.hashed_boxes(c.p, 2 * ext, seed=3), (-big, big)]


@pytest.mark.parametrize("name,seed", HOSTILE_MESHES, ids=[n for n, _ in HOSTILE_MESHES])
def test_inactive_triangles_are_never_listed_and_never_counted(name, seed):
    import boxes_sim
    from sim import SimBVH
    c = M.case(name, seed)
    fa, new = M.active_faces(c.v, c.f)
    B = SimBVH(c.v, c.f) if len(c.f) else None
    for k, (lo, hi) in enumerate(hostile_mesh_boxes(c, fa)):
        want = boxes_sim.brute(c.v, c.f, lo, hi)
        BC.check_identities(want, c.name)
        assert not c.inactive[want.faces].any(), f"{c.name}: an inactive triangle is listed"
        if k == 1:
            assert (want.count == len(fa)).all() and want.inside.all()
        # the same mesh without its inactive faces answers the same, up to the renumbering of the faces
        alone = boxes_sim.brute(c.v, fa, lo, hi)
        assert np.array_equal(want.count, alone.count) and np.array_equal(M.map_ids(want.faces, new), alone.faces)
        assert np.array_equal(want.inside, alone.inside)
        if B is not None:
            for entries in (1, 0):
                BC.assert_same(boxes_sim.walk(B, lo, hi, entries), want, f"{c.name}, stack_entries {entries}")
