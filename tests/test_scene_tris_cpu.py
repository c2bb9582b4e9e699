"""CPU checks of libtriro_scene_tris.so (include/triro_scene_tris.h, csrc/scene_tris.hip, csrc/tr_scene_tris.h): the library is
built and exports what its header declares, the loader treats the new key as it treats every key, bad arguments are refused
without a device, its code object holds exactly the shipped kernels without scratch or spills, and the core built for the host
(tests/host_sim/scene_tris_sim.cpp):
  * the per-lane instance loop returns the answers of the brute force -- the placed copies baked into one float32 mesh by
    scene_sim.points, then tris_sim.brute on it -- in any, count and rows, on every scene of scene_tris_cases (those of
    scene_cases, the overflowing placement, the scenes of small members), at stack limits 1, 2, 3 and 32, visiting the
    instances in ascending, reversed and a shuffled order;
  * one instance at the identity is tris_sim's answer on that mesh, negative-zero coordinates included; on placements that are
    exact in float32 the rows are those of the integer reference of tris_cases, pair by pair;
  * the culling itself: a culled box holds no meeting face, a box with a NaN corner never culls, and two planted mutants of it
    are killed;
  * a stand-alone sanitizer build of the host code.
A stale scene needs a committed member, and so a device: tests/test_gpu_scene_tris.py."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import scene_cases as SC
import scene_nearest_cases as NN
import scene_tris_cases as ST
import tris_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_scene_tris.h")
CSRC = os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KEY = "scene_tris"
BRUTE = "test_gpu_scene_tris.py::test_scenes_at_every_stack_limit"
TAILS = "test_gpu_scene_tris.py::test_tails_of_the_lane_and_block_indexing"
SPLIT = "test_gpu_scene_tris.py::test_a_wave_whose_lanes_meet_different_instances"
LIMITS = "test_gpu_scene_tris.py::test_row_limits"
BAKED = "test_gpu_scene_tris.py::test_the_baked_identity_on_the_same_gpu"
# one row per kernel of libtriro_scene_tris.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {"void k_scene_tris<0>": (BRUTE, TAILS, SPLIT, BAKED), "void k_scene_tris<1>": (BRUTE, TAILS, SPLIT, BAKED),
             "void k_scene_tris<2>": (BRUTE, TAILS, SPLIT, LIMITS, BAKED), "k_scene_tris_rows": (BRUTE, TAILS, LIMITS, BAKED)}
SYMBOLS = ["tr_scene_tris_abi_version", "tr_scene_tris_any", "tr_scene_tris_count", "tr_scene_tris_fill", "tr_scene_tris_stack_capacity"]
STACK_LIMITS = (1, 2, 3, 32)
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def built_library():
    """the host simulation stands for the shipped library: without libtriro_scene_tris.so built and loadable nothing here counts"""
    import triro.backend.ops as hops
    return hops.get_scene_tris_module()


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


def _child(code, **env):
    """run `code` in a fresh interpreter that can import triro; the environment is this one's plus `env`"""
    paths = [ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd")]
    head = f"import sys; sys.path[:0] = {paths!r}; import triro.backend.ops as hops\n"
    return subprocess.run([sys.executable, "-c", head + code], env={**os.environ, **env}, capture_output=True, text=True, timeout=120)


# ---- 1. the library, its header, its loader ------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.scene_tris_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_scene_tris.h but not exported"
    assert set(hops.SCENE_TRIS_ABI) == set(syms)
    exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bT (tr_[a-z_0-9]+)$", exported, re.M))) == SYMBOLS, "the library exports exactly the header's symbols"
    for other in (hops.library_path(), hops.scene_library_path(), hops.scene_nearest_library_path(), hops.tris_library_path()):
        o = ctypes.CDLL(other)
        for s in syms:
            assert not hasattr(o, s), f"{s} is exported by {os.path.basename(other)}"


def test_abi_version_stack_capacity_and_the_public_methods():
    import scene_tris_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_SCENE_TRIS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.SCENE_TRIS_ABI_VERSION == want == 1
    lib = hops.get_scene_tris_module()
    assert lib.tr_scene_tris_abi_version() == want
    cap = int(re.search(r"#define\s+TR_TRIS_STACK\s+(\d+)", open(os.path.join(CSRC, "tr_tris.h")).read()).group(1))
    assert lib.tr_scene_tris_stack_capacity() == cap == scene_tris_sim.stack_capacity() == 32
    assert len(hops.SCENE_TRIS_ABI["tr_scene_tris_any"][1]) == 6 and len(hops.SCENE_TRIS_ABI["tr_scene_tris_fill"][1]) == 10
    # the header composes the contracts and restates none of their arithmetic; the .hip file reads the one definition of the handle
    core = open(os.path.join(CSRC, "tr_scene_tris.h")).read()
    assert '#include "tr_scene_nearest.h"' in core and '#include "tr_tris.h"' in core
    for used in ("tr_scene_near_place(", "tr_scene_near_load_tri(", "tr_box_apart(", "tr_near_active(", "tr_tris_meets(", "tr_tris_live(",
                 "tr_tris_box(", "tr_rows_sort(", "tr_rewalk(", "tr_walk_push(", "tr_walk_pop("):
        assert used in core, used
    for restated in ("TR_HD bool tr_tris_meets", "TR_HD bool tr_box_apart", "TR_HD void tr_scene_point", "TR_HD void tr_scene_near_place",
                     "TR_HD float tr_scene_near_pick"):
        assert restated not in core
    for section in ("THE CONTRACT", "BAKED MESH", "IDENTITY PLACEMENT", "CULLING", "THE WALK", "OVERFLOW", "FILL", "REGISTERS"):
        assert section in core, section
    src = open(os.path.join(CSRC, "scene_tris.hip")).read()
    assert '#include "tr_scene_handle.h"' in src and not re.search(r"^struct tr_scene \{", src, re.M)
    assert "hipMalloc" not in src and "Synchronize" not in src and "hipMemset" not in src and "__launch_bounds__(ST_BS)" in src
    from triro.ray.scene import RaySceneIntersector
    for name in ("triangles_any", "triangles_count", "faces_meeting_triangles", "mesh_collides", "mesh_contacts", "colliding_instances"):
        assert callable(getattr(RaySceneIntersector, name))
    for name in ("scene_tris_native", "scene_tris_fill_native", "scene_faces_meeting_triangles_native"):
        assert callable(getattr(hops, name))
    # the argument checks of mesh against mesh are one function that both classes call
    import triro.ray.ray_optix as ro
    import triro.ray.scene as sc
    assert sc._other_triangles is ro._other_triangles
    assert "_other_triangles(vertices, faces, chunk, self.mesh_vertices.device)" in open(ro.__file__).read()


def test_the_header_is_strict_c99():
    src = '#include "triro_scene_tris.h"\nint main(void) { return TR_SCENE_TRIS_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_the_path_follows_from_the_key_and_the_environment_overrides_it(monkeypatch):
    import triro.backend.ops as hops
    var = f"TRIRO_{KEY.upper()}_LIBRARY"
    monkeypatch.delenv(var, raising=False)
    assert hops.scene_tris_library_path() == os.path.join(os.path.dirname(hops.library_path()), f"libtriro_{KEY}.so")
    monkeypatch.setenv(var, "/somewhere/else.so")
    assert hops.scene_tris_library_path() == "/somewhere/else.so"


def test_a_missing_library_raises_with_its_path(tmp_path):
    missing = str(tmp_path / f"no_such_{KEY}.so")
    r = _child(f"""
try:
    hops.get_{KEY}_module()
except RuntimeError as e:
    assert {missing!r} in str(e), str(e)
    print("RAISED")
""", **{f"TRIRO_{KEY.upper()}_LIBRARY": missing})
    assert r.returncode == 0 and "RAISED" in r.stdout, r.stdout + r.stderr


def test_the_library_loads_once_and_every_symbol_of_the_table_is_bound():
    import triro.backend.ops as hops
    lib = hops.get_scene_tris_module()
    assert hops.get_scene_tris_module() is lib
    assert len(hops.SCENE_TRIS_ABI) == 5
    for name, (res, args) in hops.SCENE_TRIS_ABI.items():
        fn = getattr(lib, name)
        assert fn.restype is res, name
        assert list(fn.argtypes or []) == list(args), name
    assert lib.tr_scene_tris_abi_version() == hops.SCENE_TRIS_ABI_VERSION


def test_a_version_mismatch_raises_with_both_numbers():
    r = _child(f"""
have = hops.{KEY.upper()}_ABI_VERSION
hops.{KEY.upper()}_ABI_VERSION = 99
try:
    hops.get_{KEY}_module()
except RuntimeError as e:
    assert f"version {{have}} " in str(e) and "99" in str(e) and "libtriro_{KEY}.so" in str(e), str(e)
    print("RAISED")
""")
    assert r.returncode == 0 and "RAISED" in r.stdout, r.stdout + r.stderr


def test_the_scene_library_is_loaded_before_this_library_on_its_handles():
    r = _child(f"""
import os
mapped = lambda: {{line.split()[-1] for line in open("/proc/self/maps") if "libtriro_" in line}}
scene, own = os.path.realpath(hops.scene_library_path()), os.path.realpath(hops.{KEY}_library_path())
assert scene not in mapped()                 # nothing is loaded at import time
hops.get_{KEY}_module()
assert {{scene, own, os.path.realpath(hops.library_path())}} <= mapped(), mapped()
print("LOADED")
""")
    assert r.returncode == 0 and "LOADED" in r.stdout, r.stdout + r.stderr


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before any device work: a scene that was never committed (or holds the empty scene) has no member
    to compare, so the stale check passes without reading a handle"""
    import triro.backend.ops as hops
    lib, slib = hops.get_scene_tris_module(), hops.get_scene_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_scene_tris_stack_capacity()
    scene = ctypes.c_void_p()
    assert slib.tr_scene_create(0, ctypes.byref(scene)) == 0 and scene.value
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    many = (1 << 31) * 128
    for call in (lib.tr_scene_tris_any, lib.tr_scene_tris_count):      # (scene, tri, n, out, stack_entries, stream)
        for args, word in (((None, out, 1, out, 0), b"scene == NULL"), ((scene, out, -1, out, 0), b"n < 0"),
                           ((scene, out, many, out, 0), b"too many triangles"), ((scene, None, 1, out, 0), b"null pointer"),
                           ((scene, out, 1, None, 0), b"null pointer"), ((scene, out, 1, out, cap + 1), b"stack_entries"),
                           ((scene, out, 1, out, -1), b"stack_entries")):
            assert call(*args, None) == 1 and word in err(), (word, err())
        assert call(scene, None, 0, None, cap, None) == 0          # nothing to do is no error
    fill = lib.tr_scene_tris_fill      # (scene, tri, n, count, offsets, total, instance, face, stack_entries, stream)
    for args, word in (((None, out, 1, out, out, 1, out, out, 0), b"scene == NULL"), ((scene, out, -1, out, out, 1, out, out, 0), b"n < 0"),
                       ((scene, out, many, out, out, 1, out, out, 0), b"too many triangles"),
                       ((scene, None, 1, out, out, 1, out, out, 0), b"null pointer"), ((scene, out, 1, None, out, 1, out, out, 0), b"null pointer"),
                       ((scene, out, 1, out, None, 1, out, out, 0), b"null pointer"), ((scene, out, 1, out, out, -1, out, out, 0), b"total < 0"),
                       ((scene, out, 1, out, out, 1, None, out, 0), b"d_instance, d_face"), ((scene, out, 1, out, out, 1, out, None, 0), b"d_instance, d_face"),
                       ((scene, out, 1, out, out, 1, out, out, cap + 1), b"stack_entries"), ((scene, out, 1, out, out, 1, out, out, -1), b"stack_entries")):
        assert fill(*args, None) == 1 and word in err(), (word, err())
    assert fill(scene, None, 0, None, None, 0, None, None, 0, None) == 0
    # the empty scene, committed (nothing to upload: no device is needed), is a scene like any other
    assert slib.tr_scene_commit(scene, None, 0, None, None, 0, None) == 0
    assert lib.tr_scene_tris_any(scene, None, 0, None, 0, None) == 0 and fill(scene, None, 0, None, None, 0, None, None, 0, None) == 0
    assert lib.tr_scene_tris_count(scene, out, 1, out, cap + 1, None) == 1 and b"stack_entries" in err()
    assert slib.tr_scene_destroy(scene) == 0


def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch_or_spills():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.scene_tris_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_scene_tris_module().tr_scene_tris_stack_capacity()
    for name, row in INVENTORY.items():
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytestmark = pytest.mark.gpu" in src
        k = kernels[name]
        print(name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        if name == "k_scene_tris_rows":
            assert k["lds"] == 0, k
        else:
            assert k["lds"] == cap * 4 * 128 == 16384, k      # the stack: capacity node ids for 128 lanes, and nothing else
            assert k["vgpr"] <= 128, f"{name}: {k['vgpr']} VGPRs, fewer than four waves per SIMD"


# ---- 2. host loop == brute force on the baked mesh -------------------------------------------------------------------------
def _trees(members):
    from sim import SimBVH
    return [SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32))) if len(f) == 0
            else SimBVH(v, f) for v, f in members]


@pytest.fixture(scope="module")
def trees():
    """member set -> [sim.SimBVH], built once"""
    return {"scene_cases": _trees(SC.members()), "overflow": _trees(NN.overflow_scene()["members"]), "small": _trees(ST.small_members())}


def test_the_fixtures_are_what_the_comparisons_need():
    ST.check_fixture_conditions()
    ST.split_wave()


@pytest.mark.parametrize("name", ST.names())
def test_host_loop_matches_the_brute_force_bit_for_bit(name, trees):
    import scene_tris_sim as S
    members, mesh_of, M = ST.scene_of(name)
    B = trees[ST.member_set(name)]
    tri, want = ST.queries_of(name), ST.brute_of(name)
    n = len(mesh_of)
    shuffled = np.random.default_rng(5).permutation(n)
    lost_at = {}
    for entries in STACK_LIMITS:
        for label, order in (("ascending", None), ("reversed", np.arange(n)[::-1]), ("shuffled", shuffled)):
            got, lost = S.walk(B, mesh_of, M, tri, entries, order=order, want_lost=True)
            ST.assert_same(got, want, f"{name}, stack_entries {entries}, visited {label}")
            lost_at[entries] = lost_at.get(entries, 0) + int(lost.sum())
    assert lost_at[32] == 0
    if name not in ("none", "small2"):      # (small2: one and two triangles, nothing is ever pushed)
        assert lost_at[1] > 0 and lost_at[2] > 0 and lost_at[3] > 0, f"{name}: the small stacks never overflowed: {lost_at}"
    else:
        assert lost_at[1] == 0
    # the same instances LISTED in another order: the same pairs under the other numbering
    if n > 1:
        with np.errstate(all="ignore"):
            again = S.brute(members, mesh_of[shuffled], M[shuffled], tri)
        ST.assert_same(ST.renumbered(again, shuffled), want, f"{name}: the brute force of the shuffled listing, renumbered")
        ST.assert_same(S.walk(B, mesh_of[shuffled], M[shuffled], tri, 2), again, f"{name}: the shuffled listing, stack_entries 2")


def test_the_wave_of_the_gpu_test(trees):
    import scene_tris_sim as S
    mesh_of, M, tri, want = ST.split_wave()
    for entries in (1, 2, 0):
        got, lost = S.walk(trees["small"], mesh_of, M, tri, entries, want_lost=True)
        ST.assert_same(got, want, f"split wave, stack_entries {entries}")
        if entries == 1:
            assert lost[192:].any(), "no long triangle overflows a stack of one entry in the icosphere"


# ---- 3. the identities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI, SC.INACTIVE])
def test_one_instance_at_the_identity_is_the_triangle_query_of_that_mesh(member, trees):
    import scene_tris_sim as S
    import tris_sim
    v, f = SC.members()[member]
    tri = np.concatenate([q for _, q in TC.query_sets(v, f)]) if member != SC.INACTIVE else TC.hashed_triangles(150, [-2] * 3, [2] * 3, 2.0, seed=5)
    tri = np.concatenate([tri, TC.hostile_triangles(tri[:40])[0]])
    eye = np.eye(3, 4, dtype=F32)[None]
    want = tris_sim.brute(v, f, tri)
    assert member == SC.INACTIVE or want.any.sum() > 20
    assert member != SC.INACTIVE or not want.any.any()
    TC.assert_same(tris_sim.walk(trees["scene_cases"][member], tri, 2), want, "the member's own walk")
    zero = np.zeros(len(want.faces), np.int32)
    for got in (S.brute(SC.members(), [member], eye, tri), S.walk(trees["scene_cases"], [member], eye, tri, 2),
                S.walk(trees["scene_cases"], [member], eye, tri, 0)):
        ST.assert_same(got, (want.any, want.count, want.offsets, zero, want.faces), f"member {member} at the identity")


def test_the_identity_holds_for_negative_zero_coordinates():
    """csrc/tr_scene_tris.h, IDENTITY PLACEMENT: the chain turns -0 into +0 and no output can tell.  The cube on even grid steps
    moved so that faces lie IN the coordinate planes, every zero coordinate written as -0, against queries that touch those
    faces, lie in their planes and carry negative zeros themselves"""
    import scene_tris_sim as S
    import tris_sim
    from sim import SimBVH
    v, f = TC.snapped_meshes()["cube"]
    v = (v + F32(0.25)).astype(F32)                      # the faces x = 0, y = 0, z = 0
    tri = TC.lattice_triangles(v, f, 300, seed=11)
    neg = v.copy()
    neg[neg == 0] = -0.0
    qneg = tri.copy()
    qneg[::2][qneg[::2] == 0] = -0.0
    assert np.signbit(neg[neg == 0]).all() and (neg == 0).sum() >= 12 and np.signbit(qneg).any()
    want = tris_sim.brute(v, f, tri)
    assert want.any.sum() > 100 and not want.any.all()
    eye = np.eye(3, 4, dtype=F32)[None]
    B = [SimBVH(neg, f)]
    zero = np.zeros(len(want.faces), np.int32)
    for q in (tri, qneg):
        TC.assert_same(tris_sim.brute(neg, f, q), want, "the mesh with negative zeros, on its own")
        for got in (S.brute([(neg, f)], [0], eye, q), S.walk(B, [0], eye, q, 1), S.walk(B, [0], eye, q, 0)):
            ST.assert_same(got, (want.any, want.count, want.offsets, zero, want.faces), "negative zeros at the identity")


def test_exact_placements_against_the_integer_reference():
    import scene_tris_sim as S
    import tris_sim
    from sim import SimBVH
    E = ST.exact_scene()
    # the chain's baking IS the integer baking, bit for bit
    v, f, inst_of, tri_of = S.bake(E["members"], E["mesh_of"], E["M"])
    assert np.array_equal(v.view(np.uint32) & 0x7fffffff, E["v"].view(np.uint32) & 0x7fffffff) and np.array_equal(v, E["v"]) and np.array_equal(f, E["f"])
    assert np.array_equal(E["face_base"][inst_of] + tri_of, np.arange(len(f)))
    stats = ST.check_exact(S.brute(E["members"], E["mesh_of"], E["M"], E["tri"]), "exact scene: the brute force")
    print("pairs %d, meeting %d, of which only touching %d, coplanar and meeting %d" % stats)
    B = [SimBVH(v, f) for v, f in E["members"]]
    n = len(E["mesh_of"])
    for entries in (1, 2, 0):
        for order in (None, np.arange(n)[::-1]):
            ST.check_exact(S.walk(B, E["mesh_of"], E["M"], E["tri"], entries, order=order), f"exact scene, stack_entries {entries}")
    # and the baked mesh as one mesh
    got = tris_sim.brute(E["v"], E["f"], E["tri"])
    assert np.array_equal(TC.listed(got, len(E["tri"]), len(E["f"])), E["met"])


# ---- 4. the culling itself ---------------------------------------------------------------------------------------------------
def _placements():
    """every finite placement of the fixtures, and the cases the proof names: negative entries, zero entries, negative zeros,
    entries that overflow"""
    Ms = [M for name in ST.names() for M in ST.scene_of(name)[2] if np.isfinite(M).all()]
    Ms += list(ST.exact_scene()["M"]) + list(ST.split_wave()[1])
    Ms.append(SC.placement(-np.ones((3, 3)), [1, 2, 3]))
    Ms.append(SC.placement([[0, 0, 1], [0, -1, 0], [1, 0, 0]], [0, 0, 0]))
    Ms.append(SC.placement([[-0.0, 2, 0], [0, -0.0, -3], [-0.5, 0, -0.0]], [-0.0, 0, 1]))
    Ms.append(SC.placement([[3e38, -3e38, 1], [1e30, 1e30, 1e30], [-1e38, 0, 1e38]], [3e38, -3e38, 0]))
    return [np.asarray(M, F32) for M in Ms]


def culled_boxes_hold_no_meeting_face(L=None):
    """THE COMPOSED STATEMENT: over placements, object-space boxes and faces with vertices inside them (the corners among
    them), no query triangle whose box tr_scene_tris_apart calls apart from the placed box meets the placed face.  The queries
    are drawn AT the placed box: around it, across it, and with a vertex exactly in one of its six planes, where strict and
    non-strict comparisons part.  -> (triples checked, culled, meeting)"""
    import scene_sim
    import scene_tris_sim as S
    rng = np.random.default_rng(12)
    nbox, per = 24, 48
    checked = culls = met = 0
    Ms = _placements()
    assert len(Ms) > 80 and any((M[:, :3] < 0).any() for M in Ms) and any((M[:, :3] == 0).any() for M in Ms)
    for j, M in enumerate(Ms):
        scale = F32(10.0) ** rng.integers(-2, 3, (nbox, 1))
        c = (rng.normal(size=(nbox, 3)) * scale).astype(F32)
        h = (np.abs(rng.normal(size=(nbox, 3))) * scale * rng.choice([0.0, 1e-3, 1.0], (nbox, 3))).astype(F32)      # flat and point boxes too
        lo, hi = c - h, c + h
        u = rng.random((nbox, per, 3, 3)).astype(F32)
        u[:, ::2] = np.round(u[:, ::2])                                      # every other face: corners of the box
        face = np.clip(lo[:, None, None] + u * (hi - lo)[:, None, None], lo[:, None, None], hi[:, None, None]).astype(F32)
        with np.errstate(all="ignore"):
            placed = scene_sim.points(M, face.reshape(-1, 3)).reshape(nbox, per, 3, 3)
            LO, HI = placed.reshape(nbox, -1, 3).min(1), placed.reshape(nbox, -1, 3).max(1)
            size = np.where(np.isfinite(HI - LO), HI - LO, F32(1e30)).max(1) + F32(1e-6)
            # queries: a placed vertex of the face moved along one axis, with two more vertices that stay on the far side of it
            # or cross back -- so the query's box ends EXACTLY at a placed coordinate, or just beyond, or overlaps
            k = rng.integers(0, 3, (nbox, per))
            base = np.take_along_axis(placed, k[:, :, None, None].repeat(3, 3), 2)[:, :, 0]          # [nbox, per, 3]
            q = np.repeat(base[:, :, None, :], 3, 2).astype(np.float64)
            axis = rng.integers(0, 3, (nbox, per))
            side = rng.choice([-1.0, 1.0], (nbox, per))
            away = rng.choice([0.0, 0.0, 1e-3, 1.0], (nbox, per)) * size[:, None]
            spread = rng.normal(size=(nbox, per, 3, 3)) * size[:, None, None, None] * 0.5
            spread[:, :, 0] = 0
            q += spread
            for a in range(3):      # the two free vertices on the chosen side of the placed vertex along `axis`, `away` from it
                sel = axis == a
                q[sel, 1:, a] = base[sel, None, a] + side[sel, None] * (away[sel, None] + np.abs(spread[sel, 1:, a]))
                q[sel, 0, a] = base[sel, a] + side[sel] * away[sel]
            q = np.clip(q, -3e38, 3e38).astype(F32)
        flat_q = q.reshape(-1, 3, 3)
        ap = S.apart(M, flat_q, np.repeat(lo, per, 0), np.repeat(hi, per, 0), L=L)
        mt = S.meets(M, flat_q, face.reshape(-1, 3, 3))
        bad = ap & mt
        assert not bad.any(), f"placement {j}: a culled box holds a meeting face, first {np.flatnonzero(bad)[:4]}"
        checked += len(ap); culls += int(ap.sum()); met += int(mt.sum())
    return checked, culls, met


def nan_cornered_boxes_never_cull(L=None):
    """boxes as the builder leaves them above inactive triangles -- NaN, -Inf and +Inf corners -- against zero entries and
    mixed signs: wherever a NaN appears among the six placed values the box is not apart from anything, however far the query
    lies from the values that are not NaN.  -> (boxes with a NaN among the placed values, boxes without that cull)"""
    import scene_nearest_sim
    import scene_tris_sim as S
    inf, nan = np.inf, np.nan
    lo = np.array([[-inf, 0, 0], [0, nan, 0], [0, 0, -inf], [-1, -1, -1], [nan, nan, nan], [-inf, -inf, -inf], [inf, 0, 0], [nan, 0, 0], [0, 0, 0]], F32)
    hi = np.array([[inf, 1, 1], [1, 1, nan], [1, 1, 1], [inf, inf, inf], [nan, nan, nan], [inf, inf, inf], [inf, 1, 1], [1, 1, 1], [1, 1, 1]], F32)
    far = np.array([[[1e6, 2e6, -3e6], [1.1e6, 2e6, -3e6], [1e6, 2.1e6, -3.1e6]], [[-1e6, -2e6, 3e6], [-1.1e6, -2e6, 3e6], [-1e6, -2.1e6, 3.1e6]]], F32)
    seen_nan = proven_culls = 0
    for M in _placements():
        with np.errstate(all="ignore"):
            LO, HI = scene_nearest_sim.place(M, lo, hi)
        unproven = np.isnan(LO).any(1) | np.isnan(HI).any(1)
        for q in far:
            ap = S.apart(M, np.repeat(q[None], len(lo), 0), lo, hi, L=L)
            assert not ap[unproven].any(), f"a box with a NaN among its placed values culls: {np.flatnonzero(ap & unproven)}, M = {M.tolist()}"
            proven_culls += int(ap[~unproven].sum())
        seen_nan += int(unproven.sum())
    assert seen_nan > 100 and proven_culls > 100, (seen_nan, proven_culls)
    return seen_nan, proven_culls


def test_a_culled_box_holds_no_meeting_face():
    checked, culls, met = culled_boxes_hold_no_meeting_face()
    print(f"{checked} (query, box, face) triples, culled {culls}, meeting {met}")
    assert culls > checked // 10 and met > checked // 10


def test_a_box_with_a_nan_corner_never_culls():
    print("boxes with a NaN among the placed values %d, proven boxes that cull %d" % nan_cornered_boxes_never_cull())


def _mutant(tmp_path, header, old, new):
    """a build of the host simulation with `old` -> `new` in a copy of csrc/`header`, bound"""
    import scene_tris_sim as S
    here = tmp_path / "tests" / "host_sim"
    csrc = tmp_path / "trimesh-ray-optix_amd" / "csrc"
    os.makedirs(here); os.makedirs(csrc)
    shutil.copy(S.SOURCE, here)
    for h in glob.glob(os.path.join(CSRC, "*.h")):
        shutil.copy(h, csrc)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    text = open(csrc / header).read()
    assert text.count(old) == 1, f"{header}: the text to replace occurs {text.count(old)} times"
    with open(csrc / header, "w") as fp:
        fp.write(text.replace(old, new))
    so = str(here / "libscene_tris_sim_mutant.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + S.FLAGS + ["-o", so, str(here / "scene_tris_sim.cpp")])
    return S.bind(ctypes.CDLL(so))


def test_a_mutant_that_culls_on_an_unproven_bound_is_killed(tmp_path):
    L = _mutant(tmp_path, "tr_scene_tris.h", "return proven && tr_box_apart(qb,", "return tr_box_apart(qb,")
    with pytest.raises(AssertionError, match="a box with a NaN among its placed values culls"):
        nan_cornered_boxes_never_cull(L)


def test_a_mutant_that_swaps_strict_and_non_strict_in_the_box_test_is_killed(tmp_path):
    """(the leaf boxes of a built hierarchy are padded, so a walk cannot tell `<` from `<=`; the composed statement on boxes
    that end exactly at their vertices can)"""
    L = _mutant(tmp_path, "tr_boxes.h", "return hix < q.lox || lox > q.hix ||", "return hix <= q.lox || lox >= q.hix ||")
    with pytest.raises(AssertionError, match="a culled box holds a meeting face"):
        culled_boxes_hold_no_meeting_face(L)


# ---- 5. a stand-alone sanitizer build ------------------------------------------------------------------------------------------
def test_a_sanitizer_build_of_the_host_code_runs_clean(tmp_path, trees):
    import scene_tris_sim as S
    exe = str(tmp_path / "scene_tris_sim_asan")
    # (the runtimes linked statically: the program is complete in itself, whatever else the process environment loads)
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DSCENE_TRIS_SIM_MAIN"] + S.FLAGS + ["-o", exe, S.SOURCE], capture_output=True)
    if r.returncode != 0 and re.search(rb"asan|ubsan|sanitize", r.stderr, re.I) and not re.search(rb"scene_tris_sim\.cpp|tr_[a-z_]+\.h", r.stderr):
        pytest.skip("g++ cannot link the sanitizer runtime here: " + r.stderr.decode()[-300:])
    assert r.returncode == 0, r.stderr.decode()
    name = "small8"
    members, mesh_of, M = ST.scene_of(name)
    B = trees["small"]
    tri, want = ST.queries_of(name), ST.brute_of(name)
    path = str(tmp_path / f"{name}.bin")
    with open(path, "wb") as fp:
        fp.write(np.array([len(B), len(mesh_of), len(tri), want.offsets[-1]], np.int64).tobytes())
        for b in B:
            fp.write(np.array([len(b.nodes), b.nf], np.int64).tobytes())
            for a, ty in ((b.nodes, np.uint32), (b.links, np.int32), (b.tris, np.uint32)):
                fp.write(np.ascontiguousarray(a, ty).tobytes())
        for a, ty in ((mesh_of, np.int32), (M, np.float32), (tri, np.float32), (want.count, np.int32), (want.instance, np.int32),
                      (want.face, np.int32)):
            fp.write(np.ascontiguousarray(a, ty).tobytes())
    run = subprocess.run([exe, path, "1"], capture_output=True, timeout=600)
    print(run.stdout.decode())
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    out = run.stdout.decode()
    assert "same as the brute force" in out
    assert int(re.search(r"(\d+) triangles overflowed a stack", out).group(1)) > 0 and int(re.search(r"(\d+) that meet something", out).group(1)) > 50
