"""CPU checks of libtriro_planes.so (include/triro_planes.h, csrc/planes.hip, csrc/tr_planes.h): the library is built and exports
what its header declares, the ctypes table covers the header, its code object holds exactly the shipped kernels without scratch or
spills, a strict-C99 client of every entry compiles and links, and the core built for the host (tests/host_sim/planes_sim.cpp):
  * the walk of a simulated wave of 64 lanes (any, count, fill + ordering + segments) returns what the brute force over the
    predicates returns, bit for bit, for MEET and CUT, at frontier capacities 1, 2, 63, 64 and all -- the small ones through the
    subtree walks, asserted -- on meshes of 0 .. 3 triangles, icospheres, cubes and a mesh with NaN / Inf / FLT_MAX vertices;
  * on inputs snapped to k * 2^-10 with integer normals, where s is exact, the classification EQUALS an integer restatement;
  * the segments of a closed mesh pair up, end for end, as bits; known answers on the 4-cell cube;
  * the ordering network alone equals numpy.sort and forms no index at or beyond m;
  * misdirected fills never write outside [0, total)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import planes_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_planes.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BRUTE = "test_gpu_planes.py::test_kernels_match_the_brute_force_at_every_frontier_capacity"
BATCH = "test_gpu_planes.py::test_batch_sizes_and_one_large_batch"
ORDER = "test_gpu_planes.py::test_the_ordering_network_alone"
MISUSE = "test_gpu_planes.py::test_misdirected_fills_stay_inside_their_rows"
# one row per kernel of libtriro_planes.so: the GPU tests that launch it and compare it with the brute force
INVENTORY = {
    "void k_planes<0>": (BRUTE, BATCH),
    "void k_planes<1>": (BRUTE, BATCH),
    "void k_planes<2>": (BRUTE, BATCH, MISUSE),
    "k_planes_rows": (BRUTE, ORDER, MISUSE),
    "k_planes_segments": (BRUTE, BATCH, MISUSE),
}
SYMBOLS = ["tr_planes_abi_version", "tr_planes_any", "tr_planes_count", "tr_planes_fill", "tr_planes_frontier_capacity", "tr_planes_order"]


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. the library and its header -------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.planes_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_planes.h but not exported"
    assert set(hops.PLANES_ABI) == set(syms)


def test_abi_version_and_frontier_capacity_match_the_sources():
    import planes_sim
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_PLANES_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.PLANES_ABI_VERSION == want == 1
    lib = hops.get_planes_module()
    assert lib.tr_planes_abi_version() == want
    core = open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "tr_planes.h")).read()
    cap = int(re.search(r"#define\s+TR_PLANES_FRONTIER\s+(\d+)", core).group(1))
    assert lib.tr_planes_frontier_capacity() == cap == planes_sim.frontier_capacity() >= 64
    for name, nargs in (("tr_planes_any", 8), ("tr_planes_count", 8), ("tr_planes_fill", 12)):
        res, args = hops.PLANES_ABI[name]
        assert len(args) == nargs and args[3] is ctypes.c_int64 and args[-2] is ctypes.c_int and args[-3] is ctypes.c_int, name
    assert hops.PLANES_ABI["tr_planes_fill"][1][6] is ctypes.c_int64
    # the row limit and the activity rule are tr_within.h's / tr_nearest.h's, included and not copied
    assert '#include "tr_within.h"' in core and "tr_rows_limit(" in open(os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc", "planes.hip")).read()
    assert "tr_near_active(" in core and not re.search(r"\btr_(rows_limit|near_active)\s*\([^;{]*\)\s*\{", core)


def test_the_other_libraries_gained_no_symbol():
    import triro.backend.ops as hops
    for path in (hops.library_path(), hops.boxes_library_path(), hops.within_library_path()):
        lib = ctypes.CDLL(path)
        for s in header_symbols():
            assert not hasattr(lib, s), (path, s)
    text = open(os.path.join(ROOT, "include", "triro_hip.h")).read()
    assert set(hops.ABI) == set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_header_is_strict_c99():
    src = '#include "triro_planes.h"\nint main(void) { return TR_PLANES_ABI_VERSION - 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def build_planes_client():
    """tests/c_client/planes_client.c -> tests/c_client/_build/planes_client (strict C99, every entry of the header once)"""
    import triro.backend.ops as hops
    libdir = os.path.dirname(hops.planes_library_path())
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = os.path.join(ROOT, "tests", "c_client", "planes_client.c")
    out = os.path.join(ROOT, "tests", "c_client", "_build", "planes_client")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include"), src, "-o", out,
           "-L", libdir, "-ltriro_planes", "-ltriro_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lm",
           "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return out


def test_a_strict_c99_client_of_every_entry_compiles_and_links():
    exe = build_planes_client()
    src = open(os.path.join(ROOT, "tests", "c_client", "planes_client.c")).read()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", src), f"planes_client.c does not call {s}"
    needed = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True).stdout
    libs = [ln.split("[")[1].split("]")[0] for ln in needed.splitlines() if "(NEEDED)" in ln]
    assert any(x.startswith("libtriro_planes") for x in libs) and any(x.startswith("libtriro_hip") for x in libs)
    assert not any(("torch" in x) or ("python" in x) or ("stdc++" in x) for x in libs), libs


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before the handle is read: a block of zeros stands in for it"""
    import triro.backend.ops as hops
    lib = hops.get_planes_module()
    err = hops.get_module().tr_last_error
    cap = lib.tr_planes_frontier_capacity()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.addressof(fake)
    out = ctypes.addressof(ctypes.create_string_buffer(64))
    big = 1 << 31
    # any / count: (bvh, origins, normals, n, out, cut, frontier_entries, stream)
    for fn in (lib.tr_planes_any, lib.tr_planes_count):
        assert fn(None, None, None, 0, None, 0, 0, None) == 1 and b"bvh" in err()
        assert fn(h, out, out, -1, out, 0, 0, None) == 1 and b"n < 0" in err()
        assert fn(h, out, out, 1, out, 0, cap + 1, None) == 1 and b"frontier_entries" in err()
        assert fn(h, out, out, 1, out, 0, -1, None) == 1 and b"frontier_entries" in err()
        assert fn(h, out, out, 1, out, 2, 0, None) == 1 and b"cut" in err()
        assert fn(h, out, out, 1, out, -1, 0, None) == 1 and b"cut" in err()
        assert fn(h, None, out, 1, out, 0, 0, None) == 1 and b"null" in err()
        assert fn(h, out, None, 1, out, 0, 0, None) == 1 and b"null" in err()
        assert fn(h, out, out, 1, None, 0, 0, None) == 1 and b"null" in err()
        assert fn(h, out, out, big, out, 0, 0, None) == 1 and b"too many" in err()
        assert fn(h, None, None, 0, None, 1, cap, None) == 0
    # fill: (bvh, origins, normals, n, count, offsets, total, face, segments, cut, frontier_entries, stream)
    fill = lib.tr_planes_fill
    assert fill(None, None, None, 0, None, None, 0, None, None, 0, 0, None) == 1 and b"bvh" in err()
    assert fill(h, out, out, -1, out, out, 1, out, None, 0, 0, None) == 1 and b"n < 0" in err()
    assert fill(h, out, out, 1, out, out, 1, out, None, 0, cap + 1, None) == 1 and b"frontier_entries" in err()
    assert fill(h, out, out, 1, out, out, 1, out, None, 3, 0, None) == 1 and b"cut" in err()
    assert fill(h, out, out, 1, out, out, -1, out, None, 0, 0, None) == 1 and b"total < 0" in err()
    assert fill(h, out, out, 1, out, out, 1, out, out, 0, 0, None) == 1 and b"segments" in err()
    assert fill(h, None, out, 1, out, out, 1, out, None, 0, 0, None) == 1 and b"null" in err()
    assert fill(h, out, None, 1, out, out, 1, out, None, 0, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, 1, None, out, 1, out, None, 0, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, 1, out, None, 1, out, None, 0, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, 1, out, out, 1, None, out, 1, 0, None) == 1 and b"null" in err()
    assert fill(h, out, out, big, out, out, 1, out, None, 0, 0, None) == 1 and b"too many" in err()
    assert fill(h, None, None, 0, None, None, 0, None, None, 1, cap, None) == 0
    assert fill(h, out, out, 1, out, out, 0, None, None, 1, 0, None) == 0          # no rows: nothing to launch
    # order: (device, n, count, offsets, total, keys, stream)
    order = lib.tr_planes_order
    assert order(0, -1, out, out, 1, out, None) == 1 and b"n < 0" in err()
    assert order(0, 1, out, out, -1, out, None) == 1 and b"total < 0" in err()
    assert order(0, 1, None, out, 1, out, None) == 1 and b"null" in err()
    assert order(0, 1, out, None, 1, out, None) == 1 and b"null" in err()
    assert order(0, 1, out, out, 1, None, None) == 1 and b"null" in err()
    assert order(0, big, out, out, 1, out, None) == 1 and b"too many" in err()
    assert order(0, 0, None, None, 0, None, None) == 0 and order(0, 1, out, out, 0, None, None) == 0


# ---- 2. the code object ----------------------------------------------------------------------------------------------
def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.planes_library_path())}
    assert set(kernels) == set(INVENTORY)
    cap = hops.get_planes_module().tr_planes_frontier_capacity()
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
        # the frontier of one wave; the tile of the ordering pass (keys and the words that ride along); nothing for the rows
        assert k["lds"] == (cap * 4 if name.startswith("void k_planes<") else (2 * 4096 * 4 if name == "k_planes_rows" else 0)), k
        assert k["vgpr"] <= 128, k          # the float64 signed values must not limit occupancy below four waves per SIMD
    # the libraries this one builds on keep exactly their kernels
    assert {k["name"] for k in con.kernels(hops.within_library_path())} == \
        {"void k_within<0>", "void k_within<1>", "void k_within<2>", "k_within_rows", "k_within_closest"}


# ---- 3. host walk == host brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute_results():
    """{mesh: (v, f, origins, normals, {cut: brute force})} for 257 hashed planes per mesh, computed once"""
    import planes_sim
    out = {}
    for k, name in enumerate(PC.MESHES):
        v, f = PC.mesh(name)
        o, nr = PC.hashed_planes(v, max(PC.BATCHES), seed=10 * k)
        out[name] = (v, f, o, nr, {c: planes_sim.brute(v, f, o, nr, cut=c) for c in (False, True)})
    return out


def sim_tree(v, f):
    from sim import SimBVH
    if len(f) == 0:
        return SimBVH(arrays=(np.zeros((0, 16), np.uint32), np.zeros((0, 2), np.int32), np.zeros((0, 12), np.uint32)))
    return SimBVH(v, f)


@pytest.mark.parametrize("name", list(PC.MESHES))
def test_host_walk_matches_the_brute_force_at_every_frontier_capacity(name, brute_results):
    import planes_sim
    v, f, o, nr, want = brute_results[name]
    B = sim_tree(v, f)
    for cut in (False, True):
        PC.check_identities(want[cut], f"{name}, cut={cut}")
        for entries in PC.FRONTIERS:
            got, stats = planes_sim.walk(B, o, nr, cut=cut, frontier_entries=entries, want_stats=True)
            PC.assert_same(got, want[cut], f"{name}, cut={cut}, frontier_entries {entries}")
            if len(f) >= 80 and name != "hostile":
                busy = want[False].count >= 16
                assert busy.sum() >= 100
                if entries in (1, 2):
                    # a plane that meets sixteen faces has pushed more than two nodes at once: the subtree walks ran
                    assert (stats.overflows[busy] > 0).all() and (stats.sub_steps[busy] > 0).all(), f"{name}: no overflow at {entries}"
                if entries == 0:
                    assert not stats.overflows.any() and not stats.sub_steps.any()
    if len(f) >= 80:
        assert 0 < want[True].count.sum() < want[False].count.sum()
    if name == "hostile":
        inactive = ~np.isfinite(v[f]).all(axis=(1, 2))
        assert inactive.sum() > 0 and not inactive[want[False].faces].any()
    if len(f) == 0:
        assert not want[False].any.any() and want[False].offsets[-1] == 0


def test_overflow_with_a_frontier_of_63_and_64_entries():
    """the capacities next to the wave width overflow only where a round pushes more: a plane through the middle of the 3 072-face
    cube does, and the results do not move"""
    import planes_sim
    v, f = PC.mesh("cube16")
    B = sim_tree(v, f)
    o = np.float32([[0.5, 0.5, 0.5]] * 3)
    nr = np.float32([[1, 1, 1], [0, 0, 1], [1, 2, 3]])
    for cut in (False, True):
        want = planes_sim.brute(v, f, o, nr, cut=cut)
        assert (want.count >= 64).all()
        for entries in (63, 64, 65, 200):
            got, stats = planes_sim.walk(B, o, nr, cut=cut, frontier_entries=entries, want_stats=True)
            PC.assert_same(got, want, f"cube16, cut={cut}, frontier_entries {entries}")
            if entries <= 64:
                assert (stats.overflows > 0).all(), entries


def test_a_plane_with_more_rows_than_the_ordering_tile():
    import planes_sim
    v, f = PC.comb()
    o, nr = PC.COMB_PLANES
    B = sim_tree(v, f)
    for cut in (False, True):
        want = planes_sim.brute(v, f, o, nr, cut=cut)
        assert want.count[0] == len(f) == 6000 and want.count[1] > 4096 and want.count[2] > 0
        assert want.count[3:].tolist() == ([1200, 0] if cut else [6000, 6000])      # edges in the plane; faces that hang from it
        for entries in (0, 1, 64):
            PC.assert_same(planes_sim.walk(B, o, nr, cut=cut, frontier_entries=entries), want, f"comb, cut={cut}, frontier_entries {entries}")


@pytest.mark.parametrize("n", PC.BATCHES)
def test_batch_sizes(n, brute_results):
    import planes_sim
    v, f, o, nr, want = brute_results["icosphere80"]
    B = sim_tree(v, f)
    for cut in (False, True):
        got = planes_sim.walk(B, o[:n], nr[:n], cut=cut)
        assert got.count.shape == (n,) and got.offsets.shape == (n + 1,)
        PC.assert_same(got, planes_sim.brute(v, f, o[:n], nr[:n], cut=cut), f"{n} planes, cut={cut}")


def test_hostile_planes_yield_empty_rows():
    import planes_sim
    v, f = PC.mesh("icosphere1280")
    o0, n0 = PC.hashed_planes(v, 64, seed=5)
    o, nr, valid, empty = PC.hostile_planes(o0, n0)
    assert (~valid).sum() == 20 and empty.sum() == 29 and valid[33:].all()
    B = sim_tree(v, f)
    for cut in (False, True):
        want = planes_sim.brute(v, f, o, nr, cut=cut)
        PC.check_identities(want, "hostile planes")
        assert not want.any[empty].any() and not want.count[empty].any()
        assert (want.count[29:33] > 0).all(), "denormal and FLT_MAX normals through the origin cut the sphere"
        for entries in (1, 0):
            PC.assert_same(planes_sim.walk(B, o, nr, cut=cut, frontier_entries=entries), want, f"hostile planes, frontier_entries {entries}")


# ---- 4. exactness: snapped inputs against an integer restatement -------------------------------------------------------------
def test_snapped_inputs_equal_the_exact_reference():
    """coordinates k * 2^-10, |k| <= 2^12, integer normals: s is exact, so the classification must EQUAL the integer restatement;
    planes through vertices, along edges and coplanar with faces included"""
    import planes_sim
    v, f = PC.mesh("cube4")
    o, nr = PC.lattice_planes()
    stats = PC.check_exact(lambda o_, n_, c: planes_sim.brute(v, f, o_, n_, cut=c), v, f, o, nr, "brute force, cube4")
    print("(pairs, met, cut, met with a vertex in the plane):", stats)
    assert 0 < stats[2] < stats[1] < stats[0] and stats[3] > 10000
    B = sim_tree(v, f)
    PC.check_exact(lambda o_, n_, c: planes_sim.walk(B, o_, n_, cut=c, frontier_entries=2), v, f, o, nr, "host walk, cube4")
    # the icosphere rounded to the grid, planes through every seventh of its vertices
    iv, i_f = PC.mesh("icosphere80")
    iv = PC.snap(iv)
    io, inr = PC.vertex_planes(iv)
    PC.check_exact(lambda o_, n_, c: planes_sim.brute(iv, i_f, o_, n_, cut=c), iv, i_f, io, inr, "brute force, snapped icosphere")


def test_the_signed_value_is_monotone_and_bounds_every_box():
    """the culling claim on the host: for boxes around hashed points, s at the corner m is <= s of every point of the box <= s
    at the corner M, in computed values"""
    import planes_sim
    rng = np.random.default_rng(7)
    lo = rng.uniform(-2, 2, (60, 3)).astype(np.float32)
    hi = (lo + rng.uniform(0, 1, (60, 3)).astype(np.float32)).astype(np.float32)
    lo[::7, 0] = hi[::7, 0]                                     # flat boxes
    o, nr = PC.hashed_planes(np.float32([[-2, -2, -2], [3, 3, 3]]), 50, seed=3)
    nr[::9, 1] = 0.0
    one = np.int32([[0, 1, 2]])
    checked = 0
    for i in range(len(lo)):
        pts = np.clip((lo[i] + (hi[i] - lo[i]) * rng.uniform(0, 1, (31, 3)).astype(np.float32)).astype(np.float32), lo[i], hi[i])
        pts = np.concatenate([pts, lo[i:i + 1], hi[i:i + 1]])           # 33 points of the box, its own corners included
        s = planes_sim.signed(pts, np.arange(33, dtype=np.int32).reshape(-1, 3), o, nr).reshape(len(o), -1)
        for k in range(len(o)):
            m = np.where(nr[k] >= 0, lo[i], hi[i]).astype(np.float32)
            M_ = np.where(nr[k] >= 0, hi[i], lo[i]).astype(np.float32)
            sm = planes_sim.signed(np.stack([m] * 3), one, o[k:k + 1], nr[k:k + 1])[0, 0, 0]
            sM = planes_sim.signed(np.stack([M_] * 3), one, o[k:k + 1], nr[k:k + 1])[0, 0, 0]
            assert (sm <= s[k]).all() and (s[k] <= sM).all()
            checked += 1
    assert checked == 3000


# ---- 5. closed loops, known answers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere80", "icosphere320", "cube4", "cube16"])
def test_segments_of_a_closed_mesh_pair_up_end_for_end(name):
    import planes_sim
    v, f = PC.mesh(name)
    rows = 0
    for label, (o, nr) in (("200 hashed planes", PC.hashed_planes(v, 200, seed=17)), ("vertex planes", PC.vertex_planes(v)),
                           ("lattice planes", PC.lattice_planes())):
        res = planes_sim.brute(v, f, o, nr, cut=True)
        assert np.isfinite(res.segments).all()
        rows += PC.loops_close(res, f"{name}, {label}")
    assert rows > 1000


def test_a_crossing_interpolated_from_the_faces_own_vertex_order_would_not_close():
    """the identity is sharp: a crossing interpolated in float32 along the face's own edge direction (from the positive vertex where
    the walk leaves the arc) instead of from negative to positive in float64 gives two neighbours different bits on the icosphere.
    (The same interpolation carried out in float64 and rounded once differs from the contract's in far fewer than one row in a
    million: it is the common rule, not the precision alone, that makes the identity exact.)"""
    import planes_sim
    v, f = PC.mesh("icosphere320")
    o, nr = PC.hashed_planes(v, 200, seed=17)
    res = planes_sim.brute(v, f, o, nr, cut=True)
    s = planes_sim.signed(v, f, o, nr)
    plane = np.repeat(np.arange(len(o)), res.count)
    sv = s[plane, res.faces].astype(np.float32)                         # [h, 3]
    tv = v[f[res.faces]]                                                 # [h, 3, 3] float32
    seg = res.segments.copy()
    for e in range(3):                                                   # leaving edge e -> e + 1 with a strictly negative end
        a, b = e, (e + 1) % 3
        rows = np.flatnonzero((sv[:, a] > 0) & (sv[:, b] < 0))
        t = (sv[rows, a] / (sv[rows, a] - sv[rows, b])).astype(np.float32)
        seg[rows, 1] = (tv[rows, a] + t[:, None] * (tv[rows, b] - tv[rows, a])).astype(np.float32)
    assert not np.array_equal(PC.bits(seg), PC.bits(res.segments))
    with pytest.raises(AssertionError):
        PC.loops_close(res._replace(segments=seg), "own vertex order")


def test_known_answers_on_the_four_cell_cube():
    import planes_sim
    v, f = PC.mesh("cube4")
    assert len(f) == 192
    B = sim_tree(v, f)
    PC.check_known(lambda o, nr, c: planes_sim.brute(v, f, o, nr, cut=c), "brute force")
    PC.check_known(lambda o, nr, c: planes_sim.walk(B, o, nr, cut=c, frontier_entries=2), "host walk")


def test_segment_ends_and_directions():
    """each end lies in the plane to rounding and on an edge of its face; the direction is (face normal) x (plane normal)"""
    import planes_sim
    v, f = PC.mesh("icosphere320")
    o, nr = PC.hashed_planes(v, 100, seed=23)
    res = planes_sim.brute(v, f, o, nr, cut=True)
    plane = np.repeat(np.arange(len(o)), res.count)
    seg = res.segments.astype(np.float64)
    n64, o64 = nr.astype(np.float64)[plane], o.astype(np.float64)[plane]
    for e in (0, 1):
        dist = np.abs(((seg[:, e] - o64) * n64).sum(1)) / np.linalg.norm(n64, axis=1)
        assert dist.max() < 1e-6
    tv = v[f[res.faces]].astype(np.float64)
    fn = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    want_dir = np.cross(fn, n64)
    d = seg[:, 1] - seg[:, 0]
    long_enough = np.linalg.norm(d, axis=1) > 1e-4
    cos = (d * want_dir).sum(1) / (np.linalg.norm(d, axis=1) * np.linalg.norm(want_dir, axis=1) + 1e-300)
    assert long_enough.sum() > 1000 and cos[long_enough].min() > 0.999


# ---- 6. the ordering network alone -----------------------------------------------------------------------------------------
def test_the_ordering_network_equals_numpy_sort_and_stays_below_m():
    import planes_sim
    parts, count, offsets, size = PC.order_case()
    keys = np.full(size, -1515870811, np.int32)
    for p, off in zip(parts, offsets):
        keys[off:off + len(p)] = p
    got = planes_sim.order(keys, count, offsets)
    want = keys.copy()
    inside = np.zeros(size, bool)
    for p, off in zip(parts, offsets):
        want[off:off + len(p)] = np.sort(p)
        inside[off:off + len(p)] = True
    assert np.array_equal(got, want)
    assert (got[~inside] == -1515870811).all() and (~inside).sum() >= 5 * len(parts)
    # a total that cuts the last segment short: the rows beyond it are not touched
    total = int(offsets[-1]) + 1
    got = planes_sim.order(keys, count, offsets, total=total)
    assert np.array_equal(got[total:], keys[total:]) and np.array_equal(got[:offsets[-1]], want[:offsets[-1]])
    for m in PC.ORDER_LENGTHS + (5, 6, 7, 100, 1023, 1025, 4096):
        pairs, largest = planes_sim.network_pairs(m)
        assert largest < max(m, 1), m
        if m >= 2:
            assert 0 < pairs <= (m * (int(np.ceil(np.log2(m))) * (int(np.ceil(np.log2(m))) + 1))) // 4 + m, m


# ---- 7. row limits and misdirected fills -----------------------------------------------------------------------------------
def test_misdirected_fills_stay_inside_their_rows():
    """counts that are too small, too large or negative, offsets outside and a total cut short never write outside [0, total);
    correct counts give the exact list"""
    import planes_sim
    v, f = PC.mesh("icosphere320")
    B = sim_tree(v, f)
    o, nr = PC.hashed_planes(v, 40, seed=31)
    want = planes_sim.brute(v, f, o, nr, cut=True)
    total = int(want.offsets[-1])
    assert total > 500
    G = 64
    POISON_I, POISON_F = np.int32(-1515870811), np.float32(np.nan)

    def run(count, offsets, tot, entries):
        face = np.full(G + total + G, POISON_I, np.int32)
        seg = np.full((G + total + G, 2, 3), POISON_F, np.float32)
        planes_sim.fill(B, o, nr, count, offsets, tot, face[G:], seg[G:], cut=True, frontier_entries=entries)
        assert (face[:G] == POISON_I).all() and (face[G + max(tot, 0):] == POISON_I).all()
        assert np.isnan(seg[:G]).all() and np.isnan(seg[G + max(tot, 0):]).all()
        return face[G:G + tot], seg[G:G + tot]
    for entries in (0, 1):
        face, seg = run(want.count, want.offsets[:-1], total, entries)
        assert np.array_equal(face, want.faces) and np.array_equal(PC.bits(seg), PC.bits(want.segments))
        small = np.maximum(want.count - 3, 0).astype(np.int32)
        face, _ = run(small, want.offsets[:-1], total, entries)
        for i in (0, 1, 20, 39):
            a = int(want.offsets[i])
            mine = want.faces[want.offsets[i]:want.offsets[i + 1]]
            assert (np.diff(face[a:a + small[i]]) > 0).all() and np.isin(face[a:a + small[i]], mine).all()
        run(want.count + 5, want.offsets[:-1], total, entries)                      # too large: into the neighbour's rows, not beyond
        run(-want.count - 1, want.offsets[:-1], total, entries)                     # negative: nothing
        run(want.count, want.offsets[:-1] + total - 7, total, entries)              # offsets outside
        run(want.count, want.offsets[:-1] - 11, total, entries)                     # negative offsets
        run(want.count, want.offsets[:-1], total - 37, entries)                     # total cut short
        run(want.count, want.offsets[:-1], 0, entries)
