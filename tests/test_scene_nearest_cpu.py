"""CPU checks of libtriro_scene_nearest.so (include/triro_scene_nearest.h, csrc/scene_nearest.hip, csrc/tr_scene_nearest.h): the
library is built and exports what its header declares, the loader treats the new key as it treats every key, bad arguments
are refused without a device, its code object holds exactly the shipped kernel without scratch or spills, and the core built
for the host (tests/host_sim/scene_nearest_sim.cpp):
  * the per-lane instance loop returns the bits of the brute force -- the placed copies baked into one float32 mesh by
    scene_sim.points, then the brute forces of nearest_sim / within_sim on it -- in all four outputs, on every scene of
    scene_cases and its reversed listing, at stack limits 1, 2, 3 and 32, in both visiting orders, unbounded and under three
    max_distance arrays;
  * one instance at the identity is nearest_sim's answer on that mesh; the answers hold the tolerances of the independent
    float64 numpy evaluation on the baked vertices; on placements that are exact in float32 the answer is the brute force on
    the integer-baked mesh;
  * the culling bound itself: placed vertices inside the placed box, the bound below the computed d2;
  * a stand-alone sanitizer build of the host code.
A stale scene needs a committed member, and so a device: tests/test_gpu_scene_nearest.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nearest_cases as NC
import scene_cases as SC
import scene_nearest_cases as NN
import scene_points_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_scene_nearest.h")
CSRC = os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KEY = "scene_nearest"
BRUTE = "test_gpu_scene_nearest.py::test_scenes_at_every_stack_limit"
TAILS = "test_gpu_scene_nearest.py::test_tails_of_the_lane_and_block_indexing"
SPLIT = "test_gpu_scene_nearest.py::test_a_wave_whose_lanes_have_their_winners_in_different_instances"
BAKED = "test_gpu_scene_nearest.py::test_the_baked_identity_on_the_same_gpu"
# one row per kernel of libtriro_scene_nearest.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {"k_scene_closest_point": (BRUTE, TAILS, SPLIT, BAKED)}
SYMBOLS = ["tr_scene_closest_point", "tr_scene_nearest_abi_version", "tr_scene_nearest_stack_capacity"]
STACK_LIMITS = (1, 2, 3, 32)
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def built_library():
    """the host simulation stands for the shipped library: without libtriro_scene_nearest.so built and loadable nothing here counts"""
    import triro.backend.ops as hops
    return hops.get_scene_nearest_module()


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
    path = hops.scene_nearest_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_scene_nearest.h but not exported"
    assert set(hops.SCENE_NEAREST_ABI) == set(syms)
    exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bT (tr_[a-z_0-9]+)$", exported, re.M))) == SYMBOLS, "the library exports exactly the header's symbols"
    for other in (hops.library_path(), hops.scene_library_path(), hops.scene_points_library_path(), hops.nearest_library_path(),
                  hops.within_library_path()):
        o = ctypes.CDLL(other)
        for s in syms:
            assert not hasattr(o, s), f"{s} is exported by {os.path.basename(other)}"


def test_abi_version_stack_capacity_and_the_public_methods():
    import scene_nearest_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_SCENE_NEAREST_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.SCENE_NEAREST_ABI_VERSION == want == 1
    lib = hops.get_scene_nearest_module()
    assert lib.tr_scene_nearest_abi_version() == want
    cap = int(re.search(r"#define\s+TR_NEAR_STACK\s+(\d+)", open(os.path.join(CSRC, "tr_nearest.h")).read()).group(1))
    assert lib.tr_scene_nearest_stack_capacity() == cap == scene_nearest_sim.stack_capacity() == 32
    args = hops.SCENE_NEAREST_ABI["tr_scene_closest_point"][1]
    assert len(args) == 11 and args[2] is ctypes.c_int64 and args[4] is ctypes.c_float
    # the header composes the contracts and restates none of their arithmetic; the .hip file reads the one definition of the handle
    core = open(os.path.join(CSRC, "tr_scene_nearest.h")).read()
    assert '#include "tr_scene.h"' in core and '#include "tr_within.h"' in core
    for used in ("tr_scene_point(", "tr_near_tri(", "tr_near_box(", "tr_near_active(", "tr_near_push(", "tr_near_pop(", "tr_within_r2(",
                 "tr_near_distance("):
        assert used in core, used
    for restated in ("TR_HD tr_near_pt tr_near_tri", "TR_HD double tr_near_box", "TR_HD void tr_scene_point"):
        assert restated not in core
    for section in ("THE CONTRACT", "BAKED MESH", "IDENTITY PLACEMENT", "THE BOUND", "CARRYING THE BEST", "THE WALK"):
        assert section in core, section
    src = open(os.path.join(CSRC, "scene_nearest.hip")).read()
    assert '#include "tr_scene_handle.h"' in src and not re.search(r"^struct tr_scene \{", src, re.M)
    assert "hipMalloc" not in src and "Synchronize" not in src and "hipMemset" not in src and "__launch_bounds__(SN_BS)" in src
    from triro.ray.scene import RaySceneIntersector
    for name in ("closest_point", "signed_distance"):
        assert callable(getattr(RaySceneIntersector, name))
    assert callable(hops.scene_closest_point_native)


def test_the_header_is_strict_c99():
    src = '#include "triro_scene_nearest.h"\nint main(void) { return TR_SCENE_NEAREST_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_the_path_follows_from_the_key_and_the_environment_overrides_it(monkeypatch):
    import triro.backend.ops as hops
    var = f"TRIRO_{KEY.upper()}_LIBRARY"
    monkeypatch.delenv(var, raising=False)
    assert hops.scene_nearest_library_path() == os.path.join(os.path.dirname(hops.library_path()), f"libtriro_{KEY}.so")
    monkeypatch.setenv(var, "/somewhere/else.so")
    assert hops.scene_nearest_library_path() == "/somewhere/else.so"


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
    lib = hops.get_scene_nearest_module()
    assert hops.get_scene_nearest_module() is lib
    assert len(hops.SCENE_NEAREST_ABI) == 3
    for name, (res, args) in hops.SCENE_NEAREST_ABI.items():
        fn = getattr(lib, name)
        assert fn.restype is res, name
        assert list(fn.argtypes or []) == list(args), name
    assert lib.tr_scene_nearest_abi_version() == hops.SCENE_NEAREST_ABI_VERSION


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
    lib, slib = hops.get_scene_nearest_module(), hops.get_scene_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_scene_nearest_stack_capacity()
    scene = ctypes.c_void_p()
    assert slib.tr_scene_create(0, ctypes.byref(scene)) == 0 and scene.value
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    inf = float("inf")
    call = lib.tr_scene_closest_point      # (scene, points, n, max_distance [n], max_distance, closest, distance, instance, tri, stack_entries, stream)
    for args, word in (((None, out, 1, None, inf, out, out, out, out, 0), b"scene == NULL"),
                       ((scene, out, -1, None, inf, out, out, out, out, 0), b"n < 0"),
                       ((scene, out, (1 << 31) * 128, None, inf, out, out, out, out, 0), b"too many points"),
                       ((scene, None, 1, None, inf, out, out, out, out, 0), b"null pointer"),
                       ((scene, out, 1, None, inf, out, out, None, out, 0), b"null pointer"),
                       ((scene, out, 1, None, inf, out, out, out, None, 0), b"null pointer"),
                       ((scene, out, 1, out, inf, None, None, out, out, cap + 1), b"stack_entries"),
                       ((scene, out, 1, None, inf, out, out, out, out, -1), b"stack_entries")):
        assert call(*args, None) == 1 and word in err(), (word, err())
    assert call(scene, None, 0, None, inf, None, None, None, None, cap, None) == 0          # nothing to do is no error
    # the empty scene, committed (nothing to upload: no device is needed), is a scene like any other
    assert slib.tr_scene_commit(scene, None, 0, None, None, 0, None) == 0
    assert call(scene, None, 0, None, 1.0, None, None, None, None, 0, None) == 0
    assert call(scene, out, 1, None, inf, out, out, out, out, cap + 1, None) == 1 and b"stack_entries" in err()
    assert slib.tr_scene_destroy(scene) == 0


def test_the_code_object_holds_exactly_the_shipped_kernel_without_scratch_or_spills():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.scene_nearest_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_scene_nearest_module().tr_scene_nearest_stack_capacity()
    for name, row in INVENTORY.items():
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytestmark = pytest.mark.gpu" in src
        k = kernels[name]
        print(name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert k["lds"] == cap * 8 * 128 == 32768, k      # the stack: capacity {node, bound} entries for 128 lanes, and nothing else


# ---- 2. host loop == brute force on the baked mesh -------------------------------------------------------------------------
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
    NN.check_fixture_conditions()


@pytest.mark.parametrize("name", list(SC.scenes()))
def test_host_loop_matches_the_brute_force_bit_for_bit(name, trees):
    import scene_nearest_sim as S
    s = SC.scenes()[name]
    r = SC.reversed_scene(s)
    n = len(s["mesh_of"])
    p = NN.points_of(name)
    back = np.arange(n)[::-1]
    for kind in NN.KINDS:
        md = NN.max_distance_of(name, kind)
        want = NN.brute_of(name, kind)
        # the reversed listing renumbers the instances: the same answer after mapping them back, except where two DIFFERENT
        # instances tie exactly in d2 -- there the one listed first wins, in either listing, at the same distance
        want_r = S.brute(SC.members(), r["mesh_of"], r["M"], p, md)
        back_r = NN.renumbered(want_r, n)
        ties = NN.cross_instance_ties(name)
        NN.assert_same([x[~ties] for x in back_r], [x[~ties] for x in want], f"{name}, {kind}: the brute force of the reversed listing, renumbered")
        assert np.array_equal(NN.bits(want_r.distance), NN.bits(want.distance))
        hit = ties & (want.instance >= 0)
        assert (want.instance[hit] <= back_r.instance[hit]).all() and (want_r.instance[hit] <= n - 1 - want.instance[hit]).all()
        for entries in STACK_LIMITS:
            got, lost = S.walk(trees, s["mesh_of"], s["M"], p, md, entries, want_lost=True)
            NN.assert_same(got, want, f"{name}, {kind}, stack_entries {entries}")
            if entries == 1 and name != "none" and kind == "none":
                assert lost.any(), f"{name}: a stack of one entry never overflowed"
            if entries == 32:
                assert not lost.any()
            NN.assert_same(S.walk(trees, r["mesh_of"], r["M"], p, md, entries), want_r, f"{name}, {kind}, reversed listing, stack_entries {entries}")
            # the same listing VISITED in reverse: nothing depends on the visiting order
            NN.assert_same(S.walk(trees, s["mesh_of"], s["M"], p, md, entries, order=back), want, f"{name}, {kind}, visited in reverse, stack_entries {entries}")
    # the optional outputs left out: the others do not change
    for outputs in (("closest",), ("distance",), ()):
        got = S.walk(trees, s["mesh_of"], s["M"], p, None, 2, outputs=outputs)
        assert (got.closest is None) == ("closest" not in outputs) and (got.distance is None) == ("distance" not in outputs)
        NN.assert_same(got, NN.brute_of(name), f"{name}, outputs {outputs}")
    # a scalar max_distance: the bounded answer is the unbounded one wherever that one's d2 is within, and nothing elsewhere
    free, d2 = S.brute(SC.members(), s["mesh_of"], s["M"], p, None, want_d2=True)
    finite = free.distance[np.isfinite(free.distance)]
    radius = F32(np.median(finite)) if len(finite) else F32(1)
    got = S.walk(trees, s["mesh_of"], s["M"], p, radius, 2)
    keep = d2 <= float(radius) * float(radius)
    assert name == "none" or (keep.sum() > 100 and (~keep).sum() > 100)
    assert np.array_equal(got.instance, np.where(keep, free.instance, -1)) and np.array_equal(got.tri, np.where(keep, free.tri, -1))
    assert np.array_equal(NN.bits(got.distance[keep]), NN.bits(free.distance[keep])) and np.isinf(got.distance[~keep]).all()
    assert np.array_equal(NN.bits(got.closest[keep]), NN.bits(free.closest[keep])) and np.isnan(got.closest[~keep]).all()


def test_the_wave_of_the_gpu_test_and_the_overflowing_placement(trees):
    """scene_nearest_cases.split_waves() and overflow_scene() assert their own layout from the brute force; the host loop agrees"""
    import scene_nearest_sim as S
    from sim import SimBVH
    mesh_of, M, p, want = NN.split_waves()
    for entries in (1, 0):
        NN.assert_same(S.walk(trees, mesh_of, M, p, None, entries), want, f"split waves, stack_entries {entries}")
    q = NN.overflow_scene()
    B = [SimBVH(v, f) for v, f in q["members"]]
    for entries in (1, 3, 0):
        for order in (None, [1, 0]):
            got = S.walk(B, q["mesh_of"], q["M"], q["p"], None, entries, order=order)
            NN.assert_same(got, q["want"], f"overflowing placement, stack_entries {entries}, order {order}")
    assert not np.isnan(got.distance).any() and not np.isnan(got.closest[got.instance >= 0]).any()


# ---- 3. the identities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI, SC.INACTIVE])
def test_one_instance_at_the_identity_is_closest_point_of_that_mesh(member, trees):
    import nearest_sim
    import scene_nearest_sim as S
    v, f = SC.members()[member]
    assert not (np.signbit(v) & (v == 0)).any(), "the identity is stated for meshes without a negative-zero coordinate"
    fin = v[np.isfinite(v).all(1)]
    lo, hi = (fin.min(0), fin.max(0)) if len(fin) else (-np.ones(3), np.ones(3))
    p = NC.hash_points(2000, 77, lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo))
    p = np.concatenate([p, fin[::7], PC.hostile_points(p[:60])])
    I = np.eye(3, 4, dtype=F32)[None]
    want = nearest_sim.brute(v, f, p)
    inst = np.where(want[2] >= 0, 0, -1).astype(np.int32)
    assert member == SC.INACTIVE or (inst == 0).sum() > 2000
    assert member != SC.INACTIVE or (inst == -1).all()
    NC.assert_same_bits(nearest_sim.walk(trees[member], p, 2), want, "the member's own walk")
    for got in (S.brute(SC.members(), [member], I, p), S.walk(trees, [member], I, p, None, 2), S.walk(trees, [member], I, p, None, 0)):
        NN.assert_same(got, (want[0], want[1], inst, want[2]), f"member {member} at the identity")


@pytest.mark.parametrize("name", ["one_affine", "three", "many65"])
def test_the_answers_hold_the_tolerances_of_the_independent_float64_evaluation(name, trees):
    """nearest_cases.check_against_numpy (a Gram-system point-triangle distance in numpy float64 that shares no formulation
    with csrc/tr_nearest.h) on the baked float32 vertices, with its existing tolerance"""
    import scene_nearest_sim as S
    s = SC.scenes()[name]
    p = NN.points_of(name)
    ok = NN.valid_points(p) & (np.abs(np.nan_to_num(p)) < 1e30).all(1)
    p = p[ok][::3]
    v, f, inst_of, tri_of = S.bake(SC.members(), s["mesh_of"], s["M"])
    got = S.walk(trees, s["mesh_of"], s["M"], p, None, 2)
    first = np.full(len(s["mesh_of"]) + 1, len(f))
    for k in np.unique(inst_of)[::-1]:
        first[k] = np.flatnonzero(inst_of == k)[0]
    baked = (first[got.instance] + got.tri).astype(np.int32)
    assert (inst_of[baked] == got.instance).all() and (tri_of[baked] == got.tri).all()
    NC.check_against_numpy(v, f, p, got.closest, got.distance, baked, f"{name}: the scene's answer on the baked vertices")


def test_exact_placements_against_the_integer_baked_mesh():
    import scene_nearest_sim as S
    from sim import SimBVH
    L = NN.lattice()
    NN.assert_same(S.brute(L["members"], L["mesh_of"], L["M"], L["p"]), L["want"], "lattice scene: the chain's baking against the integer baking")
    B = [SimBVH(v, f) for v, f in L["members"]]
    for entries in (1, 2, 0):
        for order in (None, np.arange(len(L["mesh_of"]))[::-1]):
            NN.assert_same(S.walk(B, L["mesh_of"], L["M"], L["p"], None, entries, order=order), L["want"], f"lattice scene, stack_entries {entries}")


# ---- 4. the bound itself -----------------------------------------------------------------------------------------------------
def _placements():
    """every placement of the fixtures that a walk can meet, and the cases the proof names: negative entries, zero entries,
    negative zeros, entries that overflow"""
    Ms = [M for s in SC.scenes().values() for k, M in enumerate(s["M"]) if np.isfinite(M).all()]
    Ms += list(SC.lattice_scene()["M"]) + list(NN.overflow_scene()["M"]) + list(NN.split_waves()[1])
    Ms.append(SC.placement(-np.ones((3, 3)), [1, 2, 3]))
    Ms.append(SC.placement([[0, 0, 1], [0, -1, 0], [1, 0, 0]], [0, 0, 0]))
    Ms.append(SC.placement([[-0.0, 2, 0], [0, -0.0, -3], [-0.5, 0, -0.0]], [-0.0, 0, 1]))
    Ms.append(SC.placement([[3e38, -3e38, 1], [1e30, 1e30, 1e30], [-1e38, 0, 1e38]], [3e38, -3e38, 0]))
    return [np.asarray(M, F32) for M in Ms]


def test_placed_vertices_lie_in_the_placed_box_and_the_bound_is_below_the_computed_d2():
    import scene_nearest_sim as S
    import scene_sim
    rng = np.random.default_rng(12)
    nbox, per = 40, 64
    checked = culls = infinite = 0
    Ms = _placements()
    assert len(Ms) > 80 and any((M[:, :3] < 0).any() for M in Ms) and any((M[:, :3] == 0).any() for M in Ms)
    for j, M in enumerate(Ms):
        scale = F32(10.0) ** rng.integers(-3, 4, (nbox, 1))
        if np.abs(M).max() > 1e20:
            scale = scale * F32(1e9)      # (boxes that overflow under the large placements)
        c = (rng.normal(size=(nbox, 3)) * scale).astype(F32)
        h = (np.abs(rng.normal(size=(nbox, 3))) * scale * rng.choice([0.0, 1e-3, 1.0], (nbox, 3))).astype(F32)      # flat and point boxes too
        lo, hi = c - h, c + h
        # vertices hashed inside each box, the corners themselves among them
        u = rng.random((nbox, per, 3)).astype(F32)
        u[:, :8] = np.array([[(i >> a) & 1 for a in range(3)] for i in range(8)], F32)
        v = np.clip(lo[:, None] + u * (hi - lo)[:, None], lo[:, None], hi[:, None]).astype(F32)
        assert (v >= lo[:, None]).all() and (v <= hi[:, None]).all()
        with np.errstate(all="ignore"):
            w = scene_sim.points(M, v.reshape(-1, 3)).reshape(nbox, per, 3)
        LO, HI = S.place(M, lo, hi)
        assert not np.isnan(w).any() and not np.isnan(LO).any() and not np.isnan(HI).any(), "finite M and finite corners give no NaN"
        assert (w >= LO[:, None]).all() and (w <= HI[:, None]).all(), f"placement {j}: a placed vertex outside the placed box"
        infinite += int(np.isinf(LO).any() or np.isinf(HI).any())
        # triangles of those vertices, query points around the placed box: the bound against the computed d2
        tri = w[:, rng.integers(0, per, (per, 3))]                       # [nbox, per, 3, 3]
        with np.errstate(all="ignore"):
            size = np.where(np.isfinite(HI - LO), HI - LO, F32(1e30)).max(1, keepdims=True) + np.abs(np.nan_to_num(LO, posinf=0, neginf=0)).max(1, keepdims=True) * F32(1e-3) + F32(1e-6)
            q = (np.nan_to_num((LO + HI) / 2, nan=0, posinf=0, neginf=0)[:, None] + rng.normal(size=(nbox, per, 3)) * 2 * size[:, None]).astype(F32)
            q = np.clip(q, -3e38, 3e38).astype(F32)
        d2 = S.d2(q.reshape(-1, 3), tri.reshape(-1, 3, 3)).reshape(nbox, per)
        lb = S.bound(M, q.reshape(-1, 3), np.repeat(lo, per, 0), np.repeat(hi, per, 0)).reshape(nbox, per)
        assert not np.isnan(lb).any() and (lb >= 0).all()
        assert (lb <= d2).all(), f"placement {j}: the bound exceeds a computed d2 by {np.nanmax(lb - d2)}"
        checked += lb.size
        culls += int((lb > 0).sum())
    print(f"{len(Ms)} placements, {checked} (point, triangle, box) triples, bound > 0 on {culls}, placements with an infinite placed corner {infinite}")
    assert culls > checked // 2 and infinite >= 2


def test_a_bound_that_is_not_proven_never_culls():
    """boxes as the builder leaves them above inactive triangles -- NaN, -Inf and +Inf corners -- against zero entries and
    mixed signs: wherever a NaN appears among the six placed values the bound is 0, and where none does the placed box still
    holds the placed finite vertices"""
    import scene_nearest_sim as S
    import scene_sim
    inf, nan = np.inf, np.nan
    lo = np.array([[-inf, 0, 0], [0, nan, 0], [0, 0, -inf], [-1, -1, -1], [nan, nan, nan], [-inf, -inf, -inf], [inf, 0, 0]], F32)
    hi = np.array([[inf, 1, 1], [1, 1, nan], [1, 1, 1], [inf, inf, inf], [nan, nan, nan], [inf, inf, inf], [inf, 1, 1]], F32)
    p = np.tile(F32([50, -60, 70]), (len(lo), 1))
    seen_nan = seen_inf = 0
    for M in _placements():
        with np.errstate(all="ignore"):
            LO, HI = S.place(M, lo, hi)
            lb = S.bound(M, p, lo, hi)
        unproven = np.isnan(LO).any(1) | np.isnan(HI).any(1)
        assert (lb[unproven] == 0).all() and not np.isnan(lb).any()
        seen_nan += int(unproven.sum())
        seen_inf += int((~unproven & (np.isinf(LO).any(1) | np.isinf(HI).any(1))).sum())
        # finite vertices inside such a box (the active triangles beside an inactive one) stay inside the placed box
        v = np.array([[0.25, 0.5, 0.75], [1, 1, 1], [0, 0, 0]], F32)
        for b in np.flatnonzero(~unproven):
            inside = v[((v >= lo[b]) & (v <= hi[b])).all(1)]
            w = scene_sim.points(M, inside)
            assert (w >= LO[b]).all() and (w <= HI[b]).all()
    assert seen_nan > 100 and seen_inf > 100, (seen_nan, seen_inf)
    # the identity: a NaN corner is unproven, an infinite one is not
    I = np.eye(3, 4, dtype=F32)
    LO, HI = S.place(I, lo, hi)
    assert np.array_equal(np.isnan(LO).any(1) | np.isnan(HI).any(1), [True, True, True, True, True, True, True])      # 0 x Inf in the other rows
    D = SC.placement(np.ones((3, 3)), [0, 0, 0])
    assert S.bound(D, p[:1], F32([[-inf, 0, 0]]), F32([[0, 1, 1]]))[0] > 0      # (-Inf is an ordinary lower corner: HI is finite, p is beyond it)


# ---- 5. a stand-alone sanitizer build ------------------------------------------------------------------------------------------
def test_a_sanitizer_build_of_the_host_code_runs_clean(tmp_path, trees):
    import scene_nearest_sim as S
    exe = str(tmp_path / "scene_nearest_sim_asan")
    # (the runtimes linked statically: the program is complete in itself, whatever else the process environment loads)
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DSCENE_NEAREST_SIM_MAIN"] + S.FLAGS + ["-o", exe, S.SOURCE], capture_output=True)
    if r.returncode != 0 and re.search(rb"asan|ubsan|sanitize", r.stderr, re.I) and not re.search(rb"scene_nearest_sim\.cpp|tr_[a-z_]+\.h", r.stderr):
        pytest.skip("g++ cannot link the sanitizer runtime here: " + r.stderr.decode()[-300:])
    assert r.returncode == 0, r.stderr.decode()
    s = SC.scenes()["many65"]
    p = NN.points_of("many65")
    md = NN.max_distance_of("many65", "hash")
    want = NN.brute_of("many65", "hash")
    path = str(tmp_path / "many65.bin")
    with open(path, "wb") as fp:
        fp.write(np.array([len(trees), len(s["mesh_of"]), len(p)], np.int64).tobytes())
        for B in trees:
            fp.write(np.array([len(B.nodes), B.nf], np.int64).tobytes())
            for a, ty in ((B.nodes, np.uint32), (B.links, np.int32), (B.tris, np.uint32)):
                fp.write(np.ascontiguousarray(a, ty).tobytes())
        for a, ty in ((s["mesh_of"], np.int32), (s["M"], np.float32), (p, np.float32), (md, np.float32), (want.closest, np.float32),
                      (want.distance, np.float32), (want.instance, np.int32), (want.tri, np.int32)):
            fp.write(np.ascontiguousarray(a, ty).tobytes())
    run = subprocess.run([exe, path, "1"], capture_output=True, timeout=600)
    print(run.stdout.decode())
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    out = run.stdout.decode()
    assert "same bits as the brute force" in out
    assert int(re.search(r"(\d+) points overflowed a stack", out).group(1)) > 0 and int(re.search(r"(\d+) with a nearest triangle", out).group(1)) > 500
