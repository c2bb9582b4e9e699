"""CPU checks of libtriro_scene_cross.so (include/triro_scene_cross.h, csrc/scene_cross.hip, csrc/tr_scene_cross.h): the library
is built and exports what its header declares, bad arguments are refused without a device, its code object holds exactly the
shipped kernels without scratch, and the core built for the host (tests/host_sim/scene_cross_sim.cpp):
  * the per-lane instance loop (count, fill + ordering + rows) returns the bits of the brute force -- cross_sim.brute per
    instance on the rays of scene_sim.transform, ordered by numpy.lexsort on (ray, t, instance, face) -- on every scene of
    scene_cases, under no bounds, hash bounds and bounds placed exactly on hits, at stack limits 1, 2 and 32, with the
    instances listed and visited in both orders;
  * count > 0 is the scene's any, the first row is the scene's closest hit, one instance at the identity is the crossing query
    of that mesh;
  * a stack of quads placed three times gives long lists whose rows interleave between the instances;
  * on placements that are exact in float32, count, set and order against integer arithmetic;
  * the heapsort on (t, instance, face) against numpy.lexsort, ties, signed zeros and NaN keys included;
  * a stand-alone sanitizer build of the host code."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cross_cases as CC
import range_cases as RC
import scene_cases as SC
import scene_cross_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_scene_cross.h")
CSRC = os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BRUTE = "test_gpu_scene_cross.py::test_scenes_at_every_stack_limit"
TAILS = "test_gpu_scene_cross.py::test_tails_of_the_lane_and_block_indexing"
SPLIT = "test_gpu_scene_cross.py::test_a_wave_whose_lanes_split_between_instances"
QUADS = "test_gpu_scene_cross.py::test_long_interleaved_lists_in_one_wave"
MISUSE = "test_gpu_scene_cross.py::test_fill_with_counts_of_a_narrower_interval_stays_inside_its_rows"
# one row per kernel of libtriro_scene_cross.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "void k_scene_cross<0>": (BRUTE, TAILS, SPLIT, QUADS),
    "void k_scene_cross<1>": (BRUTE, TAILS, SPLIT, QUADS, MISUSE),
    "k_scene_cross_rows": (BRUTE, TAILS, SPLIT, QUADS, MISUSE),
}
SYMBOLS = ["tr_scene_cross_abi_version", "tr_scene_cross_count", "tr_scene_cross_fill", "tr_scene_cross_stack_capacity"]
STACK_LIMITS = (1, 2, 32)
KINDS = ("none", "hash", "exact")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    """the host simulation stands for the shipped library: without libtriro_scene_cross.so built and loadable nothing here counts"""
    import triro.backend.ops as hops
    return hops.get_scene_cross_module()


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.scene_cross_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_scene_cross.h but not exported"
    assert set(hops.SCENE_CROSS_ABI) == set(syms)
    for other in (hops.library_path(), hops.scene_library_path(), hops.cross_library_path()):
        o = ctypes.CDLL(other)
        for s in syms:
            assert not hasattr(o, s), f"{s} is exported by {os.path.basename(other)}"


def test_abi_version_stack_capacity_and_the_public_methods():
    import scene_cross_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_SCENE_CROSS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.SCENE_CROSS_ABI_VERSION == want
    lib = hops.get_scene_cross_module()
    assert lib.tr_scene_cross_abi_version() == want
    cap = int(re.search(r"#define\s+TR_CROSS_STACK\s+(\d+)", open(os.path.join(CSRC, "tr_cross.h")).read()).group(1))
    assert lib.tr_scene_cross_stack_capacity() == cap == scene_cross_sim.stack_capacity() == 32
    assert len(hops.SCENE_CROSS_ABI["tr_scene_cross_count"][1]) == 7 and len(hops.SCENE_CROSS_ABI["tr_scene_cross_fill"][1]) == 18
    assert hops.SCENE_CROSS_ABI["tr_scene_cross_fill"][1][6] is ctypes.c_int64 and hops.SCENE_CROSS_ABI["tr_scene_cross_fill"][1][14] is ctypes.c_int64
    # the header composes the two contracts and restates neither; both .hip files read the one definition of the handle
    core = open(os.path.join(CSRC, "tr_scene_cross.h")).read()
    assert '#include "tr_scene.h"' in core and '#include "tr_cross.h"' in core
    for name in ("scene.hip", "scene_cross.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert '#include "tr_scene_handle.h"' in src and not re.search(r"^struct tr_scene \{", src, re.M), name
    from triro.ray.scene import RaySceneIntersector
    for name in ("intersects_count", "intersects_all", "segments_count", "segments_all"):
        assert callable(getattr(RaySceneIntersector, name))


def test_the_header_is_strict_c99():
    src = '#include "triro_scene_cross.h"\nint main(void) { return TR_SCENE_CROSS_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before any device work: a scene that was never committed (or holds the empty scene) has no member
    to compare, so the stale check passes without reading a handle"""
    import triro.backend.ops as hops
    lib, slib = hops.get_scene_cross_module(), hops.get_scene_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_scene_cross_stack_capacity()
    scene = ctypes.c_void_p()
    assert slib.tr_scene_create(0, ctypes.byref(scene)) == 0 and scene.value
    out = ctypes.addressof(ctypes.create_string_buffer(64))

    def rays(n, shape=None, o=out, d=out):
        r = hops.TrRays()
        r.d_origins, r.d_directions, r.nray = o, d, n
        r.shape = (ctypes.c_int64 * 4)(*(shape or [hops._INT64_MAX, hops._INT64_MAX, n, 3]))
        r.ostride = (ctypes.c_int64 * 4)(0, 0, 3, 1)
        r.dstride = (ctypes.c_int64 * 4)(0, 0, 3, 1)
        return ctypes.byref(r)

    def both(s, r, required, entries):
        """(status of tr_scene_cross_count, status of tr_scene_cross_fill) with `required` as the count array"""
        a = lib.tr_scene_cross_count(s, r, None, None, required, entries, None)
        ea = err()
        c = lib.tr_scene_cross_fill(s, r, None, None, required, out, 1, out, out, out, None, None, None, None, 0, None, entries, None)
        return a, c, ea + b" | " + err()

    for args, word in (((None, rays(1), out, 0), b"scene == NULL"), ((scene, None, out, 0), b"rays"), ((scene, rays(-1), out, 0), b"nray < 0"),
                       ((scene, rays(1, [hops._INT64_MAX, hops._INT64_MAX, 2, 3]), out, 0), b"product"),
                       ((scene, rays(1, o=None), out, 0), b"null"), ((scene, rays(1, d=None), out, 0), b"null"),
                       ((scene, rays(1), None, 0), b"null"), ((scene, rays(1), out, cap + 1), b"stack_entries"), ((scene, rays(1), out, -1), b"stack_entries"),
                       ((scene, rays((1 << 31) * 128), out, 0), b"too many")):
        a, c, msg = both(*args)
        assert a == 1 and c == 1 and msg.count(word) == 2, (word, a, c, msg)
    assert both(scene, rays(0, o=None, d=None), None, cap)[:2] == (0, 0)          # nothing to do is no error
    # fill: (scene, rays, tmin, tmax, count, offsets, total, instance, face, t, front, loc, uv, ray, ray_base, slot, stack_entries, stream)
    fill = lib.tr_scene_cross_fill
    assert fill(scene, rays(1), None, None, out, out, -1, out, out, out, None, None, None, None, 0, None, 0, None) == 1 and b"total < 0" in err()
    assert fill(scene, rays(1), None, None, out, None, 1, out, out, out, None, None, None, None, 0, None, 0, None) == 1 and b"null" in err()
    for k, word in enumerate((b"d_instance", b"d_face", b"d_t")):
        req = [out, out, out]
        req[k] = None
        assert fill(scene, rays(1), None, None, out, out, 1, *req, None, None, None, None, 0, None, 0, None) == 1 and word in err()
    for k in range(3):      # rows to evaluate, no scratch
        opt = [None, None, None]
        opt[k] = out
        assert fill(scene, rays(1), None, None, out, out, 1, out, out, out, *opt, None, 0, None, 0, None) == 1 and b"d_slot" in err()
    assert fill(scene, rays(1), None, None, out, out, 0, None, None, None, None, None, None, None, 0, None, 0, None) == 0      # no rows: nothing to launch
    # the empty scene, committed (nothing to upload: no device is needed), is a scene like any other
    assert slib.tr_scene_commit(scene, None, 0, None, None, 0, None) == 0
    assert both(scene, rays(0, o=None, d=None), None, 0)[:2] == (0, 0)
    a, c, msg = both(scene, rays(1), out, cap + 1)
    assert a == 1 and c == 1 and msg.count(b"stack_entries") == 2
    # (a stale scene needs a committed member, and so a device: tests/test_gpu_scene_cross.py, the lifecycle)
    assert slib.tr_scene_destroy(scene) == 0


def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.scene_cross_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_scene_cross_module().tr_scene_cross_stack_capacity()
    for name, row in INVENTORY.items():
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytestmark = pytest.mark.gpu" in src
        k = kernels[name]
        print(name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        # the stack: capacity node ids for 128 lanes, and nothing else; the ordering pass has no stack
        assert k["lds"] == (0 if name == "k_scene_cross_rows" else cap * 4 * 128), k
        assert k["vgpr"] <= 128, k          # registers must not limit occupancy below four waves per SIMD
    # the move of the handle into tr_scene_handle.h changed no kernel of libtriro_scene.so
    assert {k["name"] for k in con.kernels(hops.scene_library_path())} == {"void k_scene_query<0>", "void k_scene_query<2>"}


# ---- 2. host walk == brute force -----------------------------------------------------------------------------------------
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
    XC.check_fixture_conditions()


@pytest.mark.parametrize("name", list(SC.scenes()))
def test_host_walk_matches_the_brute_force_bit_for_bit(name, trees):
    import scene_cross_sim
    s = SC.scenes()[name]
    r = SC.reversed_scene(s)
    n = len(s["mesh_of"])
    for kind in KINDS:
        lo, hi = XC.bounds_of(name, kind)
        want = XC.brute_of(name, kind)
        # the reversed listing renumbers the instances: the same rows after mapping them back
        want_r = scene_cross_sim.brute(SC.members(), r["mesh_of"], r["M"], s["o"], s["d"], lo, hi)
        XC.assert_same(XC.renumbered(want_r, n), want, f"{name}, {kind}: the brute force of the reversed listing, renumbered")
        for entries in STACK_LIMITS:
            got, lost = scene_cross_sim.walk(trees, s["mesh_of"], s["M"], s["o"], s["d"], lo, hi, entries, want_lost=True)
            XC.assert_same(got, want, f"{name}, {kind}, stack_entries {entries}")
            if entries == 1 and name != "none":
                assert lost.any(), f"{name}: a stack of one entry never overflowed"
                if name in ("three", "many65"):      # the c0 reset path: an overflow on a ray with rows of other instances
                    assert (lost & (XC.instances_per_ray(want) >= 2)).any(), f"{name}, {kind}: no overflowing ray crosses two instances"
            if entries == 32:
                assert not lost.any()
            got = scene_cross_sim.walk(trees, r["mesh_of"], r["M"], s["o"], s["d"], lo, hi, entries)
            XC.assert_same(got, want_r, f"{name}, {kind}, reversed listing, stack_entries {entries}")
            # the same listing VISITED in reverse: neither the rows nor their order depend on the visiting order
            got = scene_cross_sim.walk(trees, s["mesh_of"], s["M"], s["o"], s["d"], lo, hi, entries, order=np.arange(n)[::-1])
            XC.assert_same(got, want, f"{name}, {kind}, visited in reverse, stack_entries {entries}")


def test_a_fill_with_counts_of_a_narrower_interval_stays_inside_its_rows(trees):
    """the caller's error on the host walk: the arrays have exactly `total` rows, so numpy's bounds are the guard for reads,
    and every row written is a crossing of its ray on the wider interval"""
    import scene_cross_sim
    s = SC.scenes()["three"]
    wide = XC.brute_of("three", "hash")
    with np.errstate(invalid="ignore"):      # (the hostile bounds: Inf - Inf)
        lo2, hi2 = CC.narrower(s["lo"], s["hi"])
    small = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], s["o"], s["d"], lo2, hi2)
    assert (wide.count >= small.count).all() and wide.offsets[-1] > small.offsets[-1] > 100
    key = (wide.ray * 8 + wide.instance) * 4096 + wide.faces
    for total in (int(small.offsets[-1]), int(small.offsets[-1]) - 37):
        got = scene_cross_sim.walk(trees, s["mesh_of"], s["M"], s["o"], s["d"], s["lo"], s["hi"], 1, count=small.count, total=total)
        mine = np.repeat(np.arange(len(s["o"])), small.count)[:total]
        assert np.array_equal(got.ray, mine)
        mykey = (mine * 8 + got.instance) * 4096 + got.faces
        assert np.isin(mykey, key).all(), "a row is no crossing of its ray on the wider interval"
        at = np.searchsorted(key, mykey, sorter=np.argsort(key))
        at = np.argsort(key)[at]
        for k in ("t", "front", "loc", "uv"):
            assert np.array_equal(RC.bits(getattr(got, k)), RC.bits(getattr(wide, k)[at])), k


# ---- 3. the identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.scenes()))
def test_count_is_any_and_the_first_row_is_the_closest_hit_of_the_scene(name):
    for kind in KINDS:
        ref = SC.brute_of(name, kind)[2]
        want = XC.brute_of(name, kind)
        assert np.array_equal(want.count, ref["count"]), f"{name}, {kind}: count against the accepted pairs of scene_sim.brute"
        assert np.array_equal(want.count > 0, ref["any"]) and np.array_equal(want.count > 0, ref["hit"])
        first = want.offsets[:-1][want.count > 0]
        hit = ref["hit"]
        for key, mine in (("instance", want.instance), ("tri", want.faces), ("t", want.t), ("front", want.front), ("loc", want.loc), ("uv", want.uv)):
            assert np.array_equal(RC.bits(mine[first]), RC.bits(ref[key][hit])), f"{name}, {kind}: {key} of the first row"


@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI])
def test_one_instance_at_the_identity_is_the_crossing_query(member, trees):
    import cross_sim
    import scene_cross_sim
    v, f = SC.members()[member]
    make = (RC.icosphere, RC.shells5, RC.icosphere)[member]
    o, d, lo, hi = make()[2:6]
    ho, hd, hlo, hhi, _ = RC.hostile_rays(o, d, lo, hi)
    o, d, lo, hi = (np.concatenate(x) for x in ((o[:6000], ho), (d[:6000], hd), (lo[:6000], hlo), (hi[:6000], hhi)))
    keep = ~(np.signbit(o) & (o == 0)).any(1) & ~(np.signbit(d) & (d == 0)).any(1)      # rays without a negative-zero component
    assert keep.sum() > 6000
    o, d, lo, hi = o[keep], d[keep], lo[keep], hi[keep]
    I = np.eye(3, 4, dtype=np.float32)[None]
    for blo, bhi in ((None, None), (lo, hi)):
        want = cross_sim.brute(v, f, o, d, blo, bhi)
        assert (want.count > 0).sum() > (20 if member == SC.TRI else 500)
        for got in (scene_cross_sim.brute(SC.members(), [member], I, o, d, blo, bhi),
                    scene_cross_sim.walk(trees, [member], I, o, d, blo, bhi, 2)):
            CC.assert_same(got, want, f"member {member} at the identity")
            assert not got.instance.any()


# ---- 4. long, interleaved lists ------------------------------------------------------------------------------------------------
def test_a_stack_of_quads_placed_three_times_interleaves_its_rows():
    import scene_cross_sim
    from sim import SimBVH
    q = XC.quad_scene()
    want = scene_cross_sim.brute(q["members"], q["mesh_of"], q["M"], q["o"], q["d"])
    XC.check_quad_scene(want, "quads, brute force")
    assert np.array_equal(want.count, 3 * q["expected"])
    B = [SimBVH(*q["members"][0])]
    for entries in (0, 1):
        for order in (None, [2, 0, 1]):
            got = scene_cross_sim.walk(B, q["mesh_of"], q["M"], q["o"], q["d"], stack_entries=entries, order=order)
            XC.assert_same(got, want, f"quads, stack_entries {entries}, order {order}")


# ---- 5. the integer-arithmetic reference ---------------------------------------------------------------------------------
def test_exact_transforms_against_the_integer_reference():
    import scene_cross_sim
    from sim import SimBVH
    L = SC.lattice_scene()
    want = scene_cross_sim.brute(L["members"], L["mesh_of"], L["M"], L["o"], L["d"])
    full, pairs = XC.check_lattice(want, "lattice scene, brute force")
    print(f"lattice scene: {full} rays without a tie compared in full, {pairs} pairs of consecutive rows in the exact order")
    assert full > 7000 and pairs > 1000
    trees = [SimBVH(v, f) for v, f in L["members"]]
    for entries in (1, 0):
        XC.assert_same(scene_cross_sim.walk(trees, L["mesh_of"], L["M"], L["o"], L["d"], None, None, entries), want, f"lattice, stack_entries {entries}")


# ---- 6. the ordering ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 2, 3, 33, 3000])
def test_the_heapsort_against_lexsort(m):
    import scene_cross_sim
    rng = np.random.default_rng(m)
    for trial in range(6):
        face = rng.integers(0, 50, m).astype(np.int32)
        inst = rng.integers(0, 7, m).astype(np.int32)
        slot = rng.permutation(m).astype(np.int32)                    # distinct: tells rows with equal keys apart
        if trial == 0:
            t = rng.random(m).astype(np.float32)
        elif trial == 1:
            t = rng.integers(0, 4, m).astype(np.float32)                    # equal t in bulk: the instance, then the face
        elif trial == 2:
            t = np.where(rng.random(m) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)      # +-0: a tie in t
        elif trial == 3:
            t = np.full(m, 1.5, np.float32)                                 # all equal
        elif trial == 4:
            t = np.sort(rng.random(m).astype(np.float32))[::-1].copy()      # descending
        else:
            t = np.concatenate([np.full(m // 2, np.inf, np.float32), rng.random(m - m // 2).astype(np.float32)])
        gt, gi, gf, gs = scene_cross_sim.sort(t, inst, face, slot)
        order = np.lexsort((face, inst, t))
        assert np.array_equal(gi, inst[order]) and np.array_equal(gf, face[order]), f"m {m}, trial {trial}"
        assert np.array_equal(gt, t[order])
        # rows travel whole: every output row is an input row (rows with wholly equal keys may swap, a heapsort is not stable)
        back = np.empty(m, np.int64)
        back[slot] = np.arange(m)
        src = back[gs]
        assert np.array_equal(np.sort(src), np.arange(m))
        assert np.array_equal(RC.bits(gt), RC.bits(t[src])) and np.array_equal(gi, inst[src]) and np.array_equal(gf, face[src])
        gt2, gi2, gf2, _ = scene_cross_sim.sort(t, inst, face)                               # without the slots
        assert np.array_equal(gi2, gi) and np.array_equal(gf2, gf) and np.array_equal(gt2, gt)
    # NaN keys (rows nobody wrote): no order is claimed, the rows stay a permutation and travel together
    for frac in (1.0, 0.5):
        t = rng.random(m).astype(np.float32)
        t[rng.random(m) < frac] = np.nan
        face = rng.permutation(m).astype(np.int32)
        inst = (face % 5).astype(np.int32)
        gt, gi, gf, gs = scene_cross_sim.sort(t, inst, face, face.copy())
        assert np.array_equal(np.sort(gf), np.arange(m)) and np.array_equal(gf, gs) and np.array_equal(gi, gf % 5)
        back = np.empty(m, np.int64)
        back[face] = np.arange(m)
        assert np.array_equal(RC.bits(gt), RC.bits(t[back[gf]]))


# ---- 7. a stand-alone sanitizer build -------------------------------------------------------------------------------------------
def test_a_sanitizer_build_of_the_host_code_runs_clean(tmp_path, trees):
    import scene_cross_sim
    exe = str(tmp_path / "scene_cross_sim_asan")
    # (the runtimes linked statically: the program is complete in itself, whatever else the process environment loads)
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DSCENE_CROSS_SIM_MAIN"] + scene_cross_sim.FLAGS + ["-o", exe, scene_cross_sim.SOURCE], capture_output=True)
    if r.returncode != 0 and re.search(rb"asan|ubsan|sanitize", r.stderr, re.I) and not re.search(rb"scene_cross_sim\.cpp|tr_[a-z_]+\.h", r.stderr):
        pytest.skip("g++ cannot link the sanitizer runtime here: " + r.stderr.decode()[-300:])
    assert r.returncode == 0, r.stderr.decode()
    s = SC.scenes()["many65"]
    want = XC.brute_of("many65", "hash")
    with np.errstate(invalid="ignore"):      # (the hostile bounds: Inf - Inf)
        lo2, hi2 = CC.narrower(s["lo"], s["hi"])
    small = scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], s["o"], s["d"], lo2, hi2)
    path = str(tmp_path / "many65.bin")
    with open(path, "wb") as fp:
        fp.write(np.array([len(trees), len(s["mesh_of"]), len(s["o"]), len(want.t)], np.int64).tobytes())
        for B in trees:
            fp.write(np.array([len(B.nodes), B.nf], np.int64).tobytes())
            for a, ty in ((B.nodes, np.uint32), (B.links, np.int32), (B.tris, np.uint32)):
                fp.write(np.ascontiguousarray(a, ty).tobytes())
        for a, ty in ((s["mesh_of"], np.int32), (s["M"], np.float32), (s["o"], np.float32), (s["d"], np.float32), (s["lo"], np.float32),
                      (s["hi"], np.float32), (want.count, np.int32), (want.instance, np.int32), (want.faces, np.int32), (want.t, np.float32),
                      (want.front, np.uint8), (want.loc, np.float32), (want.uv, np.float32), (small.count, np.int32)):
            fp.write(np.ascontiguousarray(a, ty).tobytes())
    run = subprocess.run([exe, path, "1"], capture_output=True, timeout=600)
    print(run.stdout.decode())
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    out = run.stdout.decode()
    assert "same bits as the brute force" in out and "inside its rows, ordered" in out
    assert int(re.search(r"(\d+) rays overflowed a stack", out).group(1)) > 0 and int(re.search(r"longest list (\d+)", out).group(1)) >= 10
