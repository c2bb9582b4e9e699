"""CPU checks of libtriro_cross.so (include/triro_cross.h, csrc/cross.hip, csrc/tr_cross.h): the library is built and exports
what its header declares, its code object holds exactly the shipped kernels without scratch, and the core built for the host
(tests/host_sim/cross_sim.cpp):
  * the walk over a hierarchy (count, fill + ordering + rows) returns the bits of the brute force over the per-triangle
    predicate of the range contract ordered by numpy.lexsort, at every stack limit (the overflow path included), on meshes
    with nested shells and with 3 000 coincident triangles under a hierarchy of more than 32 levels;
  * the brute force counts and lists what range_sim's brute force accepts, and its first row is range_sim's closest hit;
  * on the sheet scene and on a stack of quads the lists are known analytically;
  * the heapsort against numpy.lexsort, ties, signed zeros and NaN keys included;
  * on the lattice scenes of exact_ref, count and order against integer arithmetic;
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_cross.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BRUTE = "test_gpu_cross.py::test_kernels_match_the_brute_force_at_every_stack_limit"
TAILS = "test_gpu_cross.py::test_tails_of_the_lane_and_block_indexing"
MISUSE = "test_gpu_cross.py::test_fill_with_counts_of_a_narrower_interval_stays_inside_its_rows"
# one row per kernel of libtriro_cross.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "void k_cross<0>": (BRUTE, TAILS),
    "void k_cross<1>": (BRUTE, TAILS, MISUSE),
    "k_cross_rows": (BRUTE, TAILS, MISUSE),
}
SYMBOLS = ["tr_cross_abi_version", "tr_cross_count", "tr_cross_fill", "tr_cross_stack_capacity"]
STACK_LIMITS = (0, 1, 2, 3)


@pytest.fixture(scope="module", autouse=True)
def built_library():
    """the host simulation stands for the shipped library: without libtriro_cross.so built and loadable nothing here counts"""
    import triro.backend.ops as hops
    return hops.get_cross_module()


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 8. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.cross_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_cross.h but not exported"
    assert set(hops.CROSS_ABI) == set(syms)
    hip = ctypes.CDLL(hops.library_path())
    for s in syms:
        assert not hasattr(hip, s), f"{s} is exported by libtriro_hip.so"


def test_abi_version_and_stack_capacity_match_the_sources():
    import cross_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_CROSS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.CROSS_ABI_VERSION == want
    lib = hops.get_cross_module()
    assert lib.tr_cross_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_cross.h")).read()
    cap = int(re.search(r"#define\s+TR_CROSS_STACK\s+(\d+)", core).group(1))
    assert lib.tr_cross_stack_capacity() == cap == cross_sim.stack_capacity() == 32
    assert len(hops.CROSS_ABI["tr_cross_count"][1]) == 7 and len(hops.CROSS_ABI["tr_cross_fill"][1]) == 17
    assert hops.CROSS_ABI["tr_cross_fill"][1][6] is ctypes.c_int64 and hops.CROSS_ABI["tr_cross_fill"][1][13] is ctypes.c_int64
    # the predicate and the box tests are tr_range.h's; tr_within.h is restated where needed, not included
    assert '#include "tr_range.h"' in core and '#include "tr_within.h"' not in core


def test_the_header_is_strict_c99():
    src = '#include "triro_cross.h"\nint main(void) { return TR_CROSS_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_cross_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_cross_stack_capacity()
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
        """(status of tr_cross_count, status of tr_cross_fill) with `required` as the count array"""
        a = lib.tr_cross_count(bvh, r, None, None, required, entries, None)
        ea = err()
        c = lib.tr_cross_fill(bvh, r, None, None, required, out, 1, out, out, None, None, None, None, 0, None, entries, None)
        return a, c, ea + b" | " + err()

    for args, word in (((None, rays(1), out, 0), b"bvh"), ((h, None, out, 0), b"rays"), ((h, rays(-1), out, 0), b"nray < 0"),
                       ((h, rays(1, [hops._INT64_MAX, hops._INT64_MAX, 2, 3]), out, 0), b"product"),
                       ((h, rays(1, o=None), out, 0), b"null"), ((h, rays(1, d=None), out, 0), b"null"),
                       ((h, rays(1), None, 0), b"null"), ((h, rays(1), out, cap + 1), b"stack_entries"), ((h, rays(1), out, -1), b"stack_entries"),
                       ((h, rays((1 << 31) * 128), out, 0), b"too many")):
        a, c, msg = both(*args)
        assert a == 1 and c == 1 and msg.count(word) == 2, (word, a, c, msg)
    assert both(h, rays(0, o=None, d=None), None, cap)[:2] == (0, 0)          # nothing to do is no error
    # fill: (bvh, rays, tmin, tmax, count, offsets, total, face, t, front, loc, uv, ray, ray_base, slot, stack_entries, stream)
    fill = lib.tr_cross_fill
    assert fill(h, rays(1), None, None, out, out, -1, out, out, None, None, None, None, 0, None, 0, None) == 1 and b"total < 0" in err()
    assert fill(h, rays(1), None, None, out, None, 1, out, out, None, None, None, None, 0, None, 0, None) == 1 and b"null" in err()
    assert fill(h, rays(1), None, None, out, out, 1, None, out, None, None, None, None, 0, None, 0, None) == 1 and b"d_face" in err()
    assert fill(h, rays(1), None, None, out, out, 1, out, None, None, None, None, None, 0, None, 0, None) == 1 and b"d_t" in err()
    for k in range(3):      # rows to evaluate, no scratch
        opt = [None, None, None]
        opt[k] = out
        assert fill(h, rays(1), None, None, out, out, 1, out, out, *opt, None, 0, None, 0, None) == 1 and b"d_slot" in err()
    assert fill(h, rays(1), None, None, out, out, 0, None, None, None, None, None, None, 0, None, 0, None) == 0      # no rows: nothing to launch


def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.cross_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_cross_module().tr_cross_stack_capacity()
    for name, row in INVENTORY.items():
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytest.mark.gpu" in src
        k = kernels[name]
        print(name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        # the stack: capacity node ids for 128 lanes, and nothing else; the ordering pass has no stack
        assert k["lds"] == (0 if name == "k_cross_rows" else cap * 4 * 128), k
        assert k["vgpr"] <= 128, k          # registers must not limit occupancy below four waves per SIMD


# ---- 1. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """(vertices, faces, origins, directions, tmin, tmax, brute force) of every mesh, computed once"""
    import cross_sim
    out = {}
    for name, make in RC.MESHES.items():
        v, f, o, d, lo, hi = make()
        out[name] = (v, f, o, d, lo, hi, cross_sim.brute(v, f, o, d, lo, hi))
    return out


@pytest.mark.parametrize("name", list(RC.MESHES))
def test_host_walk_matches_the_brute_force_bit_for_bit(name, cases):
    import cross_sim
    from sim import SimBVH
    v, f, o, d, lo, hi, want = cases[name]
    B = SimBVH(v, f)
    assert want.count.max() >= 2 and (want.count == 0).any()
    if name == "deep":
        assert B.depth > 32 and (want.count[-1000:] >= 3000).sum() > 100          # 3 000 exact ties per aimed ray within its bounds
    for entries in STACK_LIMITS:
        got, lost = cross_sim.walk(B, o, d, lo, hi, entries, want_lost=True)
        CC.assert_same(got, want, f"{name}, stack_entries {entries}")
        if entries == 1:
            assert lost.any(), f"{name}: no walk overflowed a stack of one entry"
        if entries == 0:
            assert not lost.any() or name == "deep"


def test_the_rows_are_a_pure_function_of_ray_bounds_and_face(cases):
    """the rows of a narrower interval are the wider interval's rows of the same (ray, face) where no band moved the distance
    to float64: every row of the narrower list appears, bit for bit, in the default-bounds list unless it sits in a band"""
    import cross_sim
    v, f, o, d, lo, hi, want = cases["shells5"]
    full = cross_sim.brute(v, f, o, d)
    ray = want.ray
    key_full = full.ray * len(f) + full.faces
    at = np.searchsorted(key_full, ray * len(f) + want.faces, sorter=np.argsort(key_full))
    at = np.argsort(key_full)[at]
    assert np.array_equal(full.faces[at], want.faces)
    for k in ("front", "loc", "uv"):
        assert np.array_equal(RC.bits(getattr(full, k)[at]), RC.bits(getattr(want, k))), k
    band = (np.abs(want.t - lo[ray]) <= lo[ray] * np.float32(2.0 ** -10)) | (np.abs(want.t - hi[ray]) <= hi[ray] * np.float32(2.0 ** -10))
    assert np.array_equal(RC.bits(full.t[at][~band]), RC.bits(want.t[~band]))


# ---- 2. the brute force against range_sim's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "shells5"])
def test_brute_force_accepts_what_the_range_brute_force_accepts(name, cases):
    import range_sim
    v, f, o, d, lo, hi, want = cases[name]
    cap = 16
    ref = range_sim.brute(v, f, o, d, lo, hi, cap=cap)
    assert ref["count"].max() < cap and ref["count"].max() >= 2
    assert np.array_equal(want.count, ref["count"])
    acc = ref["accepted"]
    for i in range(len(o)):
        assert np.array_equal(np.sort(want.faces[CC.rows_of(want, i)]), acc[i][acc[i] >= 0]), f"{name}: ray {i}"


# ---- 4. the first row is the closest hit --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.MESHES))
def test_the_first_row_is_the_closest_hit_of_the_range_contract(name, cases):
    import range_sim
    v, f, o, d, lo, hi, want = cases[name]
    ref = range_sim.brute(v, f, o, d, lo, hi)
    assert np.array_equal(want.count > 0, ref["any"]) and np.array_equal(want.count > 0, ref["hit"])
    first = want.offsets[:-1][want.count > 0]
    hit = ref["hit"]
    assert hit.sum() > 100
    for key, mine in (("tri", want.faces), ("t", want.t), ("front", want.front), ("loc", want.loc), ("uv", want.uv)):
        assert np.array_equal(RC.bits(mine[first]), RC.bits(ref[key][hit])), f"{name}: {key} of the first row"


# ---- 3. scenes with known lists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["interior", "diagonal", "vertex"])
def test_exact_lists_on_the_sheet_scene(kind):
    import cross_sim
    from sim import SimBVH
    v, f = RC.sheets()
    o, d, lo, hi, first, count = RC.sheet_cases(kind)
    want = cross_sim.brute(v, f, o, d, lo, hi)
    CC.check_sheets(want, lo, hi, count, f"sheets, {kind}")
    B = SimBVH(v, f)
    for entries in (0, 1):
        CC.assert_same(cross_sim.walk(B, o, d, lo, hi, entries), want, f"sheets, {kind}, stack_entries {entries}")


def test_a_stack_of_quads_lists_what_each_ray_reaches():
    import cross_sim
    from sim import SimBVH
    v, f, o, d, expected = CC.quad_stack()
    B = SimBVH(v, f)
    for tmax in (None, 20.75):
        want = cross_sim.brute(v, f, o, d, None, tmax)
        CC.check_quad_stack(want, expected, tmax, f"quads, tmax {tmax}")
        for entries in (0, 1):
            CC.assert_same(cross_sim.walk(B, o, d, None, tmax, entries), want, f"quads, tmax {tmax}, stack_entries {entries}")
    assert set(np.unique(want.count)) == {0, 1, 2, 3, 21}


# ---- 5. the ordering ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 2, 3, 33, 3000])
def test_the_heapsort_against_lexsort(m):
    import cross_sim
    rng = np.random.default_rng(m)
    for trial in range(6):
        face = rng.permutation(max(m, 1) * 3)[:m].astype(np.int32)          # distinct faces
        if trial == 0:
            t = rng.random(m).astype(np.float32)
        elif trial == 1:
            t = rng.integers(0, 4, m).astype(np.float32)                    # equal t in bulk, distinct faces
        elif trial == 2:
            t = np.where(rng.random(m) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)      # +-0: a tie, broken by the face
        elif trial == 3:
            t = np.full(m, 1.5, np.float32)                                 # all equal: ascending faces
        elif trial == 4:
            t = np.sort(rng.random(m).astype(np.float32))[::-1].copy()      # descending
        else:
            t = np.concatenate([np.full(m // 2, np.inf, np.float32), rng.random(m - m // 2).astype(np.float32)])
        slot = (face.astype(np.int64) * 7 % 1000003).astype(np.int32)
        gt, gf, gs = cross_sim.sort(t, face, slot)
        order = np.lexsort((face, t))
        assert np.array_equal(gf, face[order]) and np.array_equal(gs, slot[order]), f"m {m}, trial {trial}"
        if trial == 2:
            assert np.array_equal(gt == 0, np.ones(m, bool)) and np.array_equal(RC.bits(gt), RC.bits(t[order]))      # each zero keeps its sign
        else:
            assert np.array_equal(RC.bits(gt), RC.bits(t[order]))
        gt2, gf2, _ = cross_sim.sort(t, face)                               # without the slots
        assert np.array_equal(gf2, gf) and np.array_equal(RC.bits(gt2), RC.bits(gt))
    # NaN keys (rows nobody wrote): no order is claimed, the rows stay a permutation and travel together
    for frac in (1.0, 0.5):
        t = rng.random(m).astype(np.float32)
        t[rng.random(m) < frac] = np.nan
        face = rng.permutation(m).astype(np.int32)
        gt, gf, gs = cross_sim.sort(t, face, face.copy())
        assert np.array_equal(np.sort(gf), np.arange(m)) and np.array_equal(gf, gs)
        back = np.empty(m, np.int64)
        back[face] = np.arange(m)
        assert np.array_equal(RC.bits(gt), RC.bits(t[back[gf]]))


# ---- 6. the lattice scenes against integer arithmetic ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.LATTICE_SCENES)
def test_lattice_lists_match_the_integer_arithmetic_ideal(name):
    import cross_sim
    from sim import SimBVH
    s, ideal, _ = CC.lattice_lists(name)
    want = cross_sim.brute(s["v"], s["f"], s["o"], s["d"])
    lists, ties = CC.check_lattice(name, want, f"{name}, brute force")
    print(f"{name}: {len(s['o'])} rays, {lists} lists of two or more, {ties} with two faces at one distance")
    assert lists == np.count_nonzero(ideal.count >= 2) > 0
    if name in ("cube2", "cube5", "cube8", "nested3"):
        assert ties > 0, f"{name}: no ray meets two faces at exactly the same distance"
    CC.assert_same(cross_sim.walk(SimBVH(s["v"], s["f"]), s["o"], s["d"], stack_entries=2), want, f"{name}, host walk")


# ---- 7. a stand-alone sanitizer build -------------------------------------------------------------------------------------------
def test_a_sanitizer_build_of_the_host_code_runs_clean(tmp_path, cases):
    import cross_sim
    from sim import SimBVH
    exe = str(tmp_path / "cross_sim_asan")
    # (the runtimes linked statically: the program is complete in itself, whatever else the process environment loads)
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DCROSS_SIM_MAIN"] + cross_sim.FLAGS + ["-o", exe, cross_sim.SOURCE], capture_output=True)
    if r.returncode != 0 and re.search(rb"asan|ubsan|sanitize", r.stderr, re.I) and not re.search(rb"cross_sim\.cpp|tr_[a-z]+\.h", r.stderr):
        pytest.skip("g++ cannot link the sanitizer runtime here: " + r.stderr.decode()[-300:])
    assert r.returncode == 0, r.stderr.decode()
    v, f, o, d, lo, hi, want = cases["deep"]
    keep = np.r_[0:300, len(o) - 40:len(o)]                  # hash rays, and aimed rays with 3 000 ties each
    o, d, lo, hi = (np.ascontiguousarray(x[keep]) for x in (o, d, lo, hi))
    lo2, hi2 = CC.narrower(lo, hi)
    B = SimBVH(v, f)
    path = str(tmp_path / "deep.bin")
    with open(path, "wb") as fp:
        fp.write(np.array([len(v), len(f), len(B.nodes), len(o)], np.int64).tobytes())
        for a, ty in ((v, np.float32), (f, np.int32), (B.nodes, np.uint32), (B.links, np.int32), (B.tris, np.uint32), (o, np.float32),
                      (d, np.float32), (lo, np.float32), (hi, np.float32), (lo2, np.float32), (hi2, np.float32)):
            fp.write(np.ascontiguousarray(a, ty).tobytes())
    run = subprocess.run([exe, path, "1"], capture_output=True, timeout=600)
    print(run.stdout.decode())
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    out = run.stdout.decode()
    assert "same bits as the brute force" in out and "inside its rows, ordered" in out
    assert int(re.search(r"longest list (\d+)", out).group(1)) >= 3000 and int(re.search(r"(\d+) count walks overflowed", out).group(1)) > 0
