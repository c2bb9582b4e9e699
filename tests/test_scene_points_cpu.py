"""CPU checks of libtriro_scene_points.so (include/triro_scene_points.h, csrc/scene_points.hip, csrc/tr_scene_points.h): the
library is built and exports what its header declares, bad arguments are refused without a device, its code object holds exactly
the shipped kernels without scratch, and the core built for the host (tests/host_sim/scene_points_sim.cpp):
  * the per-lane query (any, count, fill) returns the bits of the brute force -- the counts of cross_sim.brute per instance on
    the rays of scene_sim.transform for +d and -d, then the parity in numpy -- on every scene of scene_cases, at stack limits 1,
    2 and 32, with the instances listed and visited in both orders, with and without the shortcut;
  * any is count > 0, the list is the odd-odd instances of the scene's crossing rows, one instance at the identity is the parity
    of the crossing counts of that mesh;
  * on placements that are exact in float32, inside per closed instance against integer parity, along lattice directions too;
  * a stand-alone sanitizer build of the host code.
A stale scene needs a committed member, and so a device: tests/test_gpu_scene_points.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import range_cases as RC
import scene_cases as SC
import scene_points_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_scene_points.h")
CSRC = os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BRUTE = "test_gpu_scene_points.py::test_scenes_at_every_stack_limit"
TAILS = "test_gpu_scene_points.py::test_tails_of_the_lane_and_block_indexing"
SPLIT = "test_gpu_scene_points.py::test_waves_inside_different_instances_and_inside_nothing"
LATTICE = "test_gpu_scene_points.py::test_exact_transforms_against_integer_parity"
MISUSE = "test_gpu_scene_points.py::test_fill_with_counts_of_another_direction_stays_inside_its_rows"
# one row per kernel of libtriro_scene_points.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "void k_scene_points<0>": (BRUTE, TAILS, SPLIT, LATTICE),
    "void k_scene_points<1>": (BRUTE, TAILS, SPLIT, LATTICE),
    "void k_scene_points<2>": (BRUTE, TAILS, SPLIT, LATTICE, MISUSE),
}
SYMBOLS = ["tr_scene_points_abi_version", "tr_scene_points_any", "tr_scene_points_count", "tr_scene_points_fill", "tr_scene_points_stack_capacity"]
STACK_LIMITS = (1, 2, 32)


@pytest.fixture(scope="module", autouse=True)
def built_library():
    """the host simulation stands for the shipped library: without libtriro_scene_points.so built and loadable nothing here counts"""
    import triro.backend.ops as hops
    return hops.get_scene_points_module()


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.scene_points_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_scene_points.h but not exported"
    assert set(hops.SCENE_POINTS_ABI) == set(syms)
    exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bT (tr_[a-z_0-9]+)$", exported, re.M))) == SYMBOLS, "the library exports exactly the header's symbols"
    for other in (hops.library_path(), hops.scene_library_path(), hops.scene_cross_library_path(), hops.points_library_path(), hops.cross_library_path()):
        o = ctypes.CDLL(other)
        for s in syms:
            assert not hasattr(o, s), f"{s} is exported by {os.path.basename(other)}"


def test_abi_version_stack_capacity_and_the_public_methods():
    import scene_points_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_SCENE_POINTS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.SCENE_POINTS_ABI_VERSION == want == 1
    lib = hops.get_scene_points_module()
    assert lib.tr_scene_points_abi_version() == want
    cap = int(re.search(r"#define\s+TR_CROSS_STACK\s+(\d+)", open(os.path.join(CSRC, "tr_cross.h")).read()).group(1))
    assert lib.tr_scene_points_stack_capacity() == cap == scene_points_sim.stack_capacity() == 32
    assert [len(hops.SCENE_POINTS_ABI[k][1]) for k in ("tr_scene_points_any", "tr_scene_points_count", "tr_scene_points_fill")] == [7, 7, 10]
    assert hops.SCENE_POINTS_ABI["tr_scene_points_fill"][1][2] is ctypes.c_int64 and hops.SCENE_POINTS_ABI["tr_scene_points_fill"][1][6] is ctypes.c_int64
    # the header composes the contracts and restates none; the .hip file reads the one definition of the handle
    core = open(os.path.join(CSRC, "tr_scene_points.h")).read()
    assert '#include "tr_scene_cross.h"' in core and '#include "tr_points.h"' in core
    assert "tr_point_decide(" in core and "tr_scene_ray(" in core and "tr_cross_probe<" in core and "tr_cross_visit<" in core
    src = open(os.path.join(CSRC, "scene_points.hip")).read()
    assert '#include "tr_scene_handle.h"' in src and not re.search(r"^struct tr_scene \{", src, re.M)
    assert "hipMalloc" not in src and "Synchronize" not in src and "hipMemset" not in src
    from triro.ray.scene import RaySceneIntersector
    for name in ("contains_points", "contains_count", "containing_instances"):
        assert callable(getattr(RaySceneIntersector, name))
    for name in ("scene_points_any_native", "scene_points_count_native", "scene_points_fill_native", "scene_points_list_native"):
        assert callable(getattr(hops, name))


def test_the_header_is_strict_c99():
    src = '#include "triro_scene_points.h"\nint main(void) { return TR_SCENE_POINTS_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before any device work: a scene that was never committed (or holds the empty scene) has no member
    to compare, so the stale check passes without reading a handle"""
    import triro.backend.ops as hops
    lib, slib = hops.get_scene_points_module(), hops.get_scene_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_scene_points_stack_capacity()
    scene = ctypes.c_void_p()
    assert slib.tr_scene_create(0, ctypes.byref(scene)) == 0 and scene.value
    out = ctypes.addressof(ctypes.create_string_buffer(64))

    def each(s, p, n, d, required, entries):
        """the status of the three entries with `required` as the output (any, count) or the count array (fill), and their messages"""
        a = lib.tr_scene_points_any(s, p, n, d, required, entries, None)
        ea = err()
        c = lib.tr_scene_points_count(s, p, n, d, required, entries, None)
        ec = err()
        f = lib.tr_scene_points_fill(s, p, n, d, required, out, 1, out, entries, None)
        return (a, c, f), ea + b" | " + ec + b" | " + err()

    for args, word in (((None, out, 1, out, out, 0), b"scene == NULL"), ((scene, out, -1, out, out, 0), b"n < 0"),
                       ((scene, out, (1 << 31) * 128, out, out, 0), b"too many points"), ((scene, None, 1, out, out, 0), b"null pointer"),
                       ((scene, out, 1, None, out, 0), b"null pointer"), ((scene, out, 1, out, None, 0), b"null pointer"),
                       ((scene, out, 1, out, out, cap + 1), b"stack_entries"), ((scene, out, 1, out, out, -1), b"stack_entries")):
        status, msg = each(*args)
        assert status == (1, 1, 1) and msg.count(word) == 3, (word, status, msg)
    assert each(scene, None, 0, None, None, cap)[0] == (0, 0, 0)          # nothing to do is no error
    # fill: (scene, points, n, dir3, count, offsets, total, instance, stack_entries, stream)
    fill = lib.tr_scene_points_fill
    assert fill(scene, out, 1, out, out, out, -1, out, 0, None) == 1 and b"total < 0" in err()
    assert fill(scene, out, 1, out, out, None, 1, out, 0, None) == 1 and b"null pointer" in err()
    assert fill(scene, out, 1, out, out, out, 1, None, 0, None) == 1 and b"d_instance" in err()
    assert fill(scene, out, 1, out, out, out, 0, None, 0, None) == 0      # no rows: nothing to launch
    # the empty scene, committed (nothing to upload: no device is needed), is a scene like any other
    assert slib.tr_scene_commit(scene, None, 0, None, None, 0, None) == 0
    assert each(scene, None, 0, None, None, 0)[0] == (0, 0, 0)
    status, msg = each(scene, out, 1, out, out, cap + 1)
    assert status == (1, 1, 1) and msg.count(b"stack_entries") == 3
    assert slib.tr_scene_destroy(scene) == 0


def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.scene_points_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_scene_points_module().tr_scene_points_stack_capacity()
    for name, row in INVENTORY.items():
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytestmark = pytest.mark.gpu" in src
        k = kernels[name]
        print(name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert k["lds"] == cap * 4 * 128, k      # the stack: capacity node ids for 128 lanes, and nothing else
        assert k["vgpr"] <= 128, k               # registers must not limit occupancy below four waves per SIMD


# ---- 2. host walk == composition of existing brute forces ----------------------------------------------------------------
@pytest.fixture(scope="module")
def trees():
    from sim import SimBVH
    out = []
    for v, f in SC.members():
        if len(f) == 0:
            out.append(SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32))))
        else:
            out.append(SimBVH(v, f))
    return out


def test_the_fixtures_are_what_the_comparisons_need():
    PC.check_fixture_conditions()


@pytest.mark.parametrize("name", list(SC.scenes()))
def test_host_walk_matches_the_brute_force_bit_for_bit(name, trees):
    import scene_points_sim
    s = SC.scenes()[name]
    r = SC.reversed_scene(s)
    n = len(s["mesh_of"])
    p = PC.points_of(name)
    want = PC.brute_of(name)
    # the reversed listing renumbers the instances: the same rows after mapping them back
    want_r = scene_points_sim.brute(SC.members(), r["mesh_of"], r["M"], p, PC.DEFAULT)
    PC.assert_same(PC.renumbered(want_r, n), want, f"{name}: the brute force of the reversed listing, renumbered")
    for entries in STACK_LIMITS:
        got, lost = scene_points_sim.walk(trees, s["mesh_of"], s["M"], p, PC.DEFAULT, entries, want_lost=True)
        PC.assert_same(got, want, f"{name}, stack_entries {entries}")
        if entries == 1 and name != "none":
            assert (lost >= 0).any(), f"{name}: a stack of one entry never overflowed"
        if entries == 32:
            assert (lost == -1).all()
        PC.assert_same(scene_points_sim.walk(trees, r["mesh_of"], r["M"], p, PC.DEFAULT, entries), want_r, f"{name}, reversed listing, stack_entries {entries}")
        # the same listing VISITED in reverse: neither the set nor the order of the rows depends on the visiting order
        got = scene_points_sim.walk(trees, s["mesh_of"], s["M"], p, PC.DEFAULT, entries, order=np.arange(n)[::-1])
        PC.assert_same(got, want, f"{name}, visited in reverse, stack_entries {entries}")
        # THE SHORTCUT: the second pass walked for every point gives the same bits
        for order in (None, np.arange(n)[::-1]):
            got = scene_points_sim.walk(trees, s["mesh_of"], s["M"], p, PC.DEFAULT, entries, order=order, both=True)
            PC.assert_same(got, want, f"{name}, second pass forced, stack_entries {entries}")
    got = scene_points_sim.walk(trees, s["mesh_of"], s["M"], p, PC.OTHER, 2)
    PC.assert_same(got, PC.brute_of(name, "other"), f"{name}, another direction")


def test_the_waves_of_the_gpu_test_are_what_it_says(trees):
    """scene_points_cases.split_waves() asserts its own layout from the brute force; the host walk agrees with it"""
    import scene_points_sim
    mesh_of, M, p, want = PC.split_waves()
    for entries in (1, 0):
        PC.assert_same(scene_points_sim.walk(trees, mesh_of, M, p, PC.DEFAULT, entries), want, f"split waves, stack_entries {entries}")


@pytest.mark.parametrize("name", ["three", "many65"])
def test_an_overflow_in_one_instance_leaves_the_other_instances_alone(name, trees):
    """at one stack entry some point overflows in a pass of one instance and is inside ANOTHER: only that pass's count is dropped"""
    import scene_points_sim
    s = SC.scenes()[name]
    want = PC.brute_of(name)
    got, lost = scene_points_sim.walk(trees, s["mesh_of"], s["M"], PC.points_of(name), PC.DEFAULT, 1, want_lost=True)
    PC.assert_same(got, want, name)
    pt = np.repeat(np.arange(len(want.count)), want.count)
    other = np.zeros(len(want.count), bool)
    other[pt[want.instance != lost[pt]]] = True
    assert ((lost >= 0) & other).sum() > 100, f"{name}: no overflowing point is inside another instance"


def test_a_fill_with_counts_of_another_direction_stays_inside_its_rows(trees):
    """the caller's error on the host walk: the array has exactly `total` rows, so numpy's bounds are the guard; what is
    written at a point's rows are instances that hold it, ascending, and the rows it has no instance for stay untouched"""
    import scene_points_sim
    from sim import SimBVH
    q = PC.open_scene()      # (open members: on closed ones the counts of two directions are the same)
    mine, theirs = q["mine"], q["theirs"]
    B = [SimBVH(v, f) for v, f in q["members"]]
    PC.assert_same(scene_points_sim.walk(B, q["mesh_of"], q["M"], q["p"], PC.DEFAULT, 1), mine, "open scene")
    for total in (int(theirs.offsets[-1]), int(theirs.offsets[-1]) - 37):
        for order in (None, [2, 0, 1]):
            got = scene_points_sim.walk(B, q["mesh_of"], q["M"], q["p"], PC.DEFAULT, 1, order=order, count=theirs.count, total=total)
            assert len(got.instance) == total
            PC.check_misdirected_rows(got.instance, mine, theirs, total, got.instance != -7, f"total {total}, order {order}", in_order=order is None)


# ---- 3. the identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.scenes()))
def test_the_list_is_the_odd_odd_instances_of_the_crossing_rows(name):
    """tr_scene_cross_fill's rows (scene_cross_sim.brute: the brute force behind that library) on (p, +d) and (p, -d): the
    instances with an odd number of rows in each"""
    import scene_cross_sim
    s = SC.scenes()[name]
    p = PC.points_of(name)
    want = PC.brute_of(name)
    assert np.array_equal(want.any, want.count > 0)
    n, ninst = len(p), len(s["mesh_of"])
    odd = []
    for d in (PC.DEFAULT, -PC.DEFAULT):
        rows = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], p, np.broadcast_to(d, (n, 3)))
        per = np.zeros((n, max(ninst, 1)), np.int64)
        np.add.at(per, (np.repeat(np.arange(n), rows.count), rows.instance), 1)
        odd.append(per % 2 == 1)
    pt, inst = np.nonzero(odd[0] & odd[1])
    assert np.array_equal(inst.astype(np.int32), want.instance) and np.array_equal(np.bincount(pt, minlength=n).astype(np.int32), want.count)


@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI])
def test_one_instance_at_the_identity_is_the_parity_of_the_crossing_counts(member, trees):
    import cross_sim
    import scene_points_sim
    v, f = SC.members()[member]
    lo, hi = v.min(0), v.max(0)
    import nearest_cases as NC
    p = NC.hash_points(3000, 77, lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo))
    p = np.concatenate([p, PC.hostile_points(p[:60])])
    p = p[~(np.signbit(p) & (p == 0)).any(1)]      # points without a negative-zero component (the direction has none)
    I = np.eye(3, 4, dtype=np.float32)[None]
    n = len(p)
    cp = cross_sim.walk(trees[member], p, np.broadcast_to(PC.DEFAULT, (n, 3)), stack_entries=2).count      # tr_cross_count's walk
    cm = cross_sim.walk(trees[member], p, np.broadcast_to(-PC.DEFAULT, (n, 3)), stack_entries=2).count
    assert np.array_equal(cp, cross_sim.brute(v, f, p, np.broadcast_to(PC.DEFAULT, (n, 3))).count)
    inside = ((cp & 1) == 1) & ((cm & 1) == 1)
    assert member == SC.TRI or inside.sum() > 500
    assert member != SC.TRI or (not inside.any() and ((cp + cm) == 1).sum() > 100)
    for got in (scene_points_sim.brute(SC.members(), [member], I, p, PC.DEFAULT), scene_points_sim.walk(trees, [member], I, p, PC.DEFAULT, 2)):
        assert np.array_equal(got.any, inside) and np.array_equal(got.count, inside.astype(np.int32)) and not got.instance.any()
        assert len(got.instance) == inside.sum()


# ---- 4. the integer reference --------------------------------------------------------------------------------------------
def test_exact_transforms_against_integer_parity():
    import scene_points_sim
    from sim import SimBVH
    L = SC.lattice_scene()
    P = PC.lattice_points()
    want = [scene_points_sim.brute(L["members"], L["mesh_of"], L["M"], P["p"], d) for d in PC.LATTICE_DIRECTIONS]
    PC.check_lattice(lambda j: want[j], "lattice scene, brute force")
    print(f"lattice scene: {len(P['p'])} points, inside per instance {P['inside'].sum(1)}, tie points per lattice direction (of a quarter) {P['ties']}")
    trees = [SimBVH(v, f) for v, f in L["members"]]
    for j, d in enumerate(PC.LATTICE_DIRECTIONS):
        for entries in (1, 0):
            PC.assert_same(scene_points_sim.walk(trees, L["mesh_of"], L["M"], P["p"], d, entries), want[j], f"lattice, direction {d}, stack_entries {entries}")


# ---- 5. a stand-alone sanitizer build ---------------------------------------------------------------------------------------
def test_a_sanitizer_build_of_the_host_code_runs_clean(tmp_path, trees):
    import scene_points_sim
    exe = str(tmp_path / "scene_points_sim_asan")
    # (the runtimes linked statically: the program is complete in itself, whatever else the process environment loads)
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DSCENE_POINTS_SIM_MAIN"] + scene_points_sim.FLAGS + ["-o", exe, scene_points_sim.SOURCE], capture_output=True)
    if r.returncode != 0 and re.search(rb"asan|ubsan|sanitize", r.stderr, re.I) and not re.search(rb"scene_points_sim\.cpp|tr_[a-z_]+\.h", r.stderr):
        pytest.skip("g++ cannot link the sanitizer runtime here: " + r.stderr.decode()[-300:])
    assert r.returncode == 0, r.stderr.decode()
    s = SC.scenes()["many65"]
    p = PC.points_of("many65")
    want = PC.brute_of("many65")
    misdirected = np.roll(want.count, 1)      # the counts of each point's neighbour: many65 is closed wherever it holds anything
    assert (want.count != misdirected).sum() > 200
    path = str(tmp_path / "many65.bin")
    with open(path, "wb") as fp:
        fp.write(np.array([len(trees), len(s["mesh_of"]), len(p), len(want.instance)], np.int64).tobytes())
        for B in trees:
            fp.write(np.array([len(B.nodes), B.nf], np.int64).tobytes())
            for a, ty in ((B.nodes, np.uint32), (B.links, np.int32), (B.tris, np.uint32)):
                fp.write(np.ascontiguousarray(a, ty).tobytes())
        for a, ty in ((s["mesh_of"], np.int32), (s["M"], np.float32), (p, np.float32), (PC.DEFAULT, np.float32), (want.any, np.uint8),
                      (want.count, np.int32), (want.instance, np.int32), (misdirected, np.int32)):
            fp.write(np.ascontiguousarray(a, ty).tobytes())
    run = subprocess.run([exe, path, "1"], capture_output=True, timeout=600)
    print(run.stdout.decode())
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    out = run.stdout.decode()
    assert "same bits as the brute force" in out and "inside its rows, ascending" in out
    assert int(re.search(r"(\d+) points overflowed a stack", out).group(1)) > 0 and int(re.search(r"longest list (\d+)", out).group(1)) >= 2
