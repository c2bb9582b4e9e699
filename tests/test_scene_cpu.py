"""CPU checks of libtriro_scene.so (include/triro_scene.h, csrc/scene.hip, csrc/tr_scene.h): the library is built and exports
what its header declares, the ctypes table covers the header, bad arguments are refused without a device, its code object
holds exactly the two instantiations of k_scene_query without scratch or spills, and the core built for the host
(tests/host_sim/scene_sim.cpp):
  * the brute force -- tr_range_tri on every triangle of every instance, reduced by (t, instance, face) -- agrees bit for bit
    with a second computation in numpy: the range brute force per instance on the transformed rays, reduced in numpy;
  * the per-lane instance loop over the members' hierarchies returns the brute force's bits at every stack limit, for the
    instances listed in both orders and visited in both orders;
  * one instance at M = I is the range query on that mesh;
  * on members and placements that are exact in float32 the scene EQUALS the integer-arithmetic reference on the baked mesh,
    ray by ray; rays through an edge or a vertex -- where the owner depends on the projected frame -- EQUAL the same integer
    rule evaluated in each instance's frame;
  * the written fmaf order of the transform is the order evaluated in exact rationals with one rounding per operation;
  * the inverse of every placement is the float32 rounding of numpy's float64 inverse to a few units in the last place."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import range_cases as RC
import scene_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "triro_scene.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# one row per kernel of libtriro_scene.so: the GPU tests that launch it and compare it with the brute force
_TESTS = ("test_gpu_scene.py::test_scenes_at_every_stack_limit",
          "test_gpu_scene.py::test_tails_of_the_lane_and_block_indexing",
          "test_gpu_scene.py::test_a_wave_whose_lanes_split_between_instances",
          "test_gpu_scene.py::test_exact_transforms_against_the_integer_reference")
INVENTORY = {
    "void k_scene_query<0>": _TESTS,      # TR_Q_ANY
    "void k_scene_query<2>": _TESTS,      # TR_Q_CLOSEST
}
SYMBOLS = ["tr_scene_abi_version", "tr_scene_any", "tr_scene_closest", "tr_scene_commit", "tr_scene_create", "tr_scene_destroy",
           "tr_scene_info"]


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tr_[a-z_0-9]+)\s*\(", src)))


# ---- 1. plumbing -------------------------------------------------------------------------------------------------------
def test_the_library_exists_and_exports_every_declared_symbol():
    import triro.backend.ops as hops
    path = hops.scene_library_path()
    assert os.path.exists(path), "build with __graft_entry__.build()"
    ctypes.CDLL(hops.library_path(), mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert syms == SYMBOLS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/triro_scene.h but not exported"
    assert set(hops.SCENE_ABI) == set(syms)
    hip = ctypes.CDLL(hops.library_path())
    for s in syms:
        assert not hasattr(hip, s), f"libtriro_hip.so gained {s}"


def test_abi_version_argument_counts_and_the_public_class():
    import triro.backend.ops as hops
    want = int(re.search(r"#define\s+TR_SCENE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert hops.SCENE_ABI_VERSION == want
    lib = hops.get_scene_module()
    assert lib.tr_scene_abi_version() == want
    assert len(hops.SCENE_ABI["tr_scene_any"][1]) == 7 and len(hops.SCENE_ABI["tr_scene_closest"][1]) == 13
    assert len(hops.SCENE_ABI["tr_scene_commit"][1]) == 7
    import triro.ray
    from triro.ray.scene import RaySceneIntersector
    assert triro.ray.RaySceneIntersector is RaySceneIntersector
    for name in ("set_transforms", "commit", "intersects_any", "intersects_closest", "segments_any", "segments_closest"):
        assert callable(getattr(RaySceneIntersector, name))


def test_the_header_is_strict_c99():
    src = '#include "triro_scene.h"\nint main(void) { tr_scene_info_t i; i.device = 0; return TR_SCENE_ABI_VERSION - 1 + i.device; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_invalid_arguments_are_refused_without_a_device():
    """every refusal comes before any device work: blocks of zeros stand in for member handles (their first word, the
    device ordinal, is all that is read before a refusal), and a scene that was never committed has no member to compare"""
    import triro.backend.ops as hops
    lib = hops.get_scene_module()
    err = hops.get_module().tr_last_error
    scene = ctypes.c_void_p()
    assert lib.tr_scene_create(0, ctypes.byref(scene)) == 0 and scene.value
    assert lib.tr_scene_create(0, None) == 1
    inf = hops.TrSceneInfo()
    assert lib.tr_scene_info(scene, ctypes.byref(inf)) == 0
    assert (inf.device, inf.num_members, inf.num_instances, inf.table_bytes, inf.commits, inf.stack_capacity) == (0, 0, 0, 0, 0, 32)
    here, there = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    ctypes.cast(there, ctypes.POINTER(ctypes.c_int))[0] = 1                      # a member on device 1
    members = lambda *bufs: (ctypes.c_void_p * len(bufs))(*(ctypes.addressof(b) if b is not None else None for b in bufs))  # noqa: E731
    mesh_of = np.zeros(4, np.int32)
    M = np.tile(np.eye(3, 4, dtype=np.float32).reshape(-1), (4, 1))
    mp, Mp = mesh_of.ctypes.data, M.ctypes.data
    for args, word in (((None, members(here), 1, mp, Mp, 1), b"scene == NULL"), ((scene, members(here), -1, mp, Mp, 1), b"negative"),
                       ((scene, members(here), 1, mp, Mp, -1), b"negative"), ((scene, None, 1, mp, Mp, 1), b"members == NULL"),
                       ((scene, members(here), 1, None, Mp, 1), b"== NULL"), ((scene, members(here), 1, mp, None, 1), b"== NULL"),
                       ((scene, members(here, None), 2, mp, Mp, 1), b"member 1 == NULL"),
                       ((scene, members(here, there), 2, mp, Mp, 1), b"member 1 lives on device 1"),
                       ((scene, members(here), 0, mp, Mp, 1), b"names member 0 outside")):
        assert lib.tr_scene_commit(*args, None) == 1 and word in err(), (word, err())
    mesh_of[2] = 1
    assert lib.tr_scene_commit(scene, members(here), 1, mp, Mp, 4, None) == 1 and b"instance 2 names member 1" in err()
    mesh_of[2] = -1
    assert lib.tr_scene_commit(scene, members(here), 1, mp, Mp, 4, None) == 1 and b"instance 2 names member -1" in err()
    assert lib.tr_scene_info(scene, ctypes.byref(inf)) == 0 and inf.commits == 0      # a refused commit changes nothing
    # the empty scene is a scene: committed without a device, since there is nothing to upload
    assert lib.tr_scene_commit(scene, None, 0, None, None, 0, None) == 0
    assert lib.tr_scene_info(scene, ctypes.byref(inf)) == 0 and (inf.commits, inf.num_instances) == (1, 0)
    # the queries: the argument checks of tr_range_*
    out = ctypes.addressof(ctypes.create_string_buffer(64))

    def rays(n, shape=None, o=out, d=out):
        r = hops.TrRays()
        r.d_origins, r.d_directions, r.nray = o, d, n
        r.shape = (ctypes.c_int64 * 4)(*(shape or [hops._INT64_MAX, hops._INT64_MAX, n, 3]))
        r.ostride = (ctypes.c_int64 * 4)(0, 0, 3, 1)
        r.dstride = (ctypes.c_int64 * 4)(0, 0, 3, 1)
        return ctypes.byref(r)

    def both(s, r, required, entries):
        a = lib.tr_scene_any(s, r, None, None, required, entries, None)
        ea = err()
        c = lib.tr_scene_closest(s, r, None, None, out, required, out, out, out, out, out, entries, None)
        return a, c, ea + b" | " + err()

    for args, word in (((None, rays(1), out, 0), b"scene"), ((scene, None, out, 0), b"rays"), ((scene, rays(-1), out, 0), b"nray < 0"),
                       ((scene, rays(1, [hops._INT64_MAX, hops._INT64_MAX, 2, 3]), out, 0), b"product"),
                       ((scene, rays(1, o=None), out, 0), b"null"), ((scene, rays(1, d=None), out, 0), b"null"),
                       ((scene, rays(1), None, 0), b"null"), ((scene, rays(1), out, 33), b"stack_entries"), ((scene, rays(1), out, -1), b"stack_entries"),
                       ((scene, rays((1 << 31) * 128), out, 0), b"too many")):
        a, c, msg = both(*args)
        assert a == 1 and c == 1 and msg.count(word) == 2, (word, a, c, msg)
    assert both(scene, rays(0, o=None, d=None), None, 32)[:2] == (0, 0)
    assert lib.tr_scene_closest(scene, rays(0), None, None, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.tr_scene_destroy(scene) == 0 and lib.tr_scene_destroy(None) == 0


def test_the_code_object_holds_exactly_the_shipped_kernels_without_scratch():
    import code_object_notes as con
    import triro.backend.ops as hops
    if not os.path.exists(con.READELF):
        pytest.skip("llvm-readelf not available")
    kernels = {k["name"]: k for k in con.kernels(hops.scene_library_path())}
    assert set(kernels) == set(INVENTORY)
    for name, row in INVENTORY.items():
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{name}: {test_id} does not exist"
            assert "pytest.mark.gpu" in src
        k = kernels[name]
        print(name, k)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert k["lds"] == 32 * 8 * 128, k       # the far-child stack of k_range_query, and nothing else
        assert k["vgpr"] <= 168, k                # 32 KB of LDS allow ten waves per CU: registers must not limit it further


# ---- 2. brute force == the second computation; walk == brute force -------------------------------------------------------
@pytest.fixture(scope="module")
def brutes():
    """(scene, bounds kind) -> (lo, hi, brute force), computed once"""
    import scene_sim
    mem = SC.members()
    out = {}
    for name, s in SC.scenes().items():
        free = scene_sim.brute(mem, s["mesh_of"], s["M"], s["o"], s["d"])
        out[name, "none"] = (None, None, free)
        out[name, "hash"] = (s["lo"], s["hi"], scene_sim.brute(mem, s["mesh_of"], s["M"], s["o"], s["d"], s["lo"], s["hi"]))
        lo, hi = SC.exact_bounds(free, s["lo"], s["hi"])
        out[name, "exact"] = (lo, hi, scene_sim.brute(mem, s["mesh_of"], s["M"], s["o"], s["d"], lo, hi))
    return out


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


def test_the_scenes_are_what_they_claim(brutes):
    s = SC.scenes()
    import scene_sim
    _, valid, flip = scene_sim.record(s["odd"]["M"])
    assert valid.tolist() == [True, True, True, False, False, True, True, True] and flip.tolist()[:3] == [True, False, False] and flip[7]
    free = brutes["odd", "none"][2]
    hit_inst = set(free["instance"][free["hit"]].tolist())
    assert hit_inst >= {0, 1, 2} and not hit_inst & {3, 4, 5, 6}, hit_inst      # the mirror, the tiny and the huge copy are hit; invalid ones never
    for name in ("one_affine", "two_same", "three", "odd", "many65"):
        for kind in ("none", "hash", "exact"):
            w = brutes[name, kind][2]
            assert w["hit"].sum() > 100 and (~w["hit"]).sum() > 100, (name, kind)
    assert set(brutes["two_same", "none"][2]["instance"].tolist()) == {-1, 0}          # equal placements: the lower index wins every tie
    assert (brutes["two_same", "none"][2]["count"] % 2 == 0).all()
    assert len(set(brutes["three", "hash"][2]["instance"].tolist())) == 4
    assert len(set(brutes["many65", "none"][2]["instance"].tolist())) > 30
    assert not brutes["none", "none"][2]["any"].any()
    # bounds placed on hits: the float32 distance lies in the band of the bound, so the float64-derived distance decides and
    # is the distance reported -- on either side of the bound, within the 2^-11 of a float32 distance
    for name in ("three", "odd"):
        free, (lo, hi, ex) = brutes[name, "none"][2], brutes[name, "exact"]
        for on in (free["hit"] & (hi == free["t"]), free["hit"] & (lo == free["t"])):
            same = on & ex["hit"] & (ex["instance"] == free["instance"]) & (ex["tri"] == free["tri"])
            assert on.sum() > 50 and same.sum() > 20, (name, int(on.sum()), int(same.sum()))
            assert (np.abs(ex["t"][same].astype(np.float64) - free["t"][same]) <= free["t"][same] * 2.0 ** -11).all()
            assert ((ex["t"][same] >= lo[same]) & (ex["t"][same] <= hi[same])).all()
    RC.check_miss_rule(brutes["three", "hash"][2], s["three"]["bad"], "brute force")
    assert (brutes["three", "hash"][2]["instance"][s["three"]["bad"]] == -1).all()


@pytest.mark.parametrize("name", list(SC.scenes()))
def test_brute_force_matches_the_numpy_reduction_of_per_instance_range_queries(name, brutes):
    s = SC.scenes()[name]
    for kind in ("none", "hash", "exact"):
        lo, hi, want = brutes[name, kind]
        got = SC.numpy_brute(SC.members(), s["mesh_of"], s["M"], s["o"], s["d"], lo, hi)
        RC.assert_same_bits(got, want, f"{name}, bounds {kind}", keys=SC.KEYS)


@pytest.mark.parametrize("name", list(SC.scenes()))
def test_host_walk_matches_the_brute_force_bit_for_bit(name, brutes, trees):
    import scene_sim
    s = SC.scenes()[name]
    r = SC.reversed_scene(s)
    n = len(s["mesh_of"])
    for kind in ("none", "hash", "exact"):
        lo, hi, want = brutes[name, kind]
        want_r = scene_sim.brute(SC.members(), r["mesh_of"], r["M"], s["o"], s["d"], lo, hi)
        if name != "two_same":      # (equal placements tie, and the lower index wins in either listing)
            back = dict(want_r)
            back["instance"] = np.where(want_r["hit"], n - 1 - want_r["instance"], -1).astype(np.int32)
            RC.assert_same_bits(back, want, f"{name}, {kind}: the reversed listing, renumbered", keys=SC.KEYS)
        for entries in (1, 2, 0):
            got = scene_sim.walk(trees, s["mesh_of"], s["M"], s["o"], s["d"], lo, hi, entries)
            RC.assert_same_bits(got, want, f"{name}, {kind}, stack_entries {entries}", keys=SC.KEYS)
            if entries == 1 and n and name != "none":
                assert got["lost"].any() and got["lost_any"].any(), f"{name}: a stack of one entry never overflowed"
            if entries == 0:
                assert not got["lost"].any() and not got["lost_any"].any()
            got = scene_sim.walk(trees, r["mesh_of"], r["M"], s["o"], s["d"], lo, hi, entries)
            RC.assert_same_bits(got, want_r, f"{name}, {kind}, reversed listing, stack_entries {entries}", keys=SC.KEYS)
            # the same listing VISITED in reverse: the answer does not depend on the visiting order
            got = scene_sim.walk(trees, s["mesh_of"], s["M"], s["o"], s["d"], lo, hi, entries, order=np.arange(n)[::-1])
            RC.assert_same_bits(got, want, f"{name}, {kind}, visited in reverse, stack_entries {entries}", keys=SC.KEYS)


# ---- 4. identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("member", [SC.ICO, SC.SHELLS, SC.TRI])
def test_one_instance_at_the_identity_is_the_range_query(member):
    import range_sim
    import scene_sim
    v, f = SC.members()[member]
    make = (RC.icosphere, RC.shells5, RC.icosphere)[member]
    o, d, lo, hi = make()[2:6]
    ho, hd, hlo, hhi, _ = RC.hostile_rays(o, d, lo, hi)
    o, d, lo, hi = (np.concatenate(x) for x in ((o[:6000], ho), (d[:6000], hd), (lo[:6000], hlo), (hi[:6000], hhi)))
    keep = ~(np.signbit(o) & (o == 0)).any(1) & ~(np.signbit(d) & (d == 0)).any(1)      # rays without a negative-zero component
    assert keep.sum() > 6000
    o, d, lo, hi = o[keep], d[keep], lo[keep], hi[keep]
    I = np.eye(3, 4, dtype=np.float32)[None]
    W_, valid, flip = scene_sim.record(I)
    assert np.array_equal(W_, I.reshape(1, 12)) and valid[0] and not flip[0]
    o2, d2, ok = scene_sim.transform(I[0], o, d)
    fin = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    assert np.array_equal(RC.bits(o2[fin]), RC.bits(o[fin])) and np.array_equal(RC.bits(d2[fin]), RC.bits(d[fin])) and np.array_equal(ok, fin)
    for blo, bhi in ((None, None), (lo, hi)):
        want = range_sim.brute(v, f, o, d, blo, bhi)
        got = scene_sim.brute(SC.members(), [member], I, o, d, blo, bhi)
        assert want["hit"].sum() > (20 if member == SC.TRI else 500)
        RC.assert_same_bits(got, want, f"member {member} at the identity", keys=RC.KEYS_ANY + RC.KEYS_CLOSEST)
        assert np.array_equal(got["instance"], np.where(want["hit"], 0, -1))


# ---- 5. the integer-arithmetic reference ---------------------------------------------------------------------------------
def test_exact_transforms_against_the_integer_reference():
    import scene_sim
    from sim import SimBVH
    L = SC.lattice_scene()
    # the transforms and their inverses are exact: M W = I in integers / dyadic rationals, and the object-space rays are integers
    W_, valid, flip = scene_sim.record(L["M"])
    assert valid.all() and flip.tolist() == [True, False, True, False, True]
    for k in range(len(L["M"])):
        M4, W4 = np.eye(4), np.eye(4)
        M4[:3], W4[:3] = L["M"][k].astype(np.float64), W_[k].reshape(3, 4).astype(np.float64)
        assert np.array_equal(M4 @ W4, np.eye(4)) and np.array_equal(W4 @ M4, np.eye(4)), k
        o2, d2, ok = scene_sim.transform(L["M"][k], L["o"], L["d"])
        # (dyadic: integers over the scale, a power of two; float64 holds W o + w and W d without rounding)
        assert ok.all() and np.array_equal(o2 * 8, np.rint(o2 * 8)) and np.array_equal(d2 * 8, np.rint(d2 * 8))
        assert np.array_equal((W4[:3, :3] @ L["o"].astype(np.float64).T).T + W4[:3, 3], o2.astype(np.float64))
        assert np.abs(d2).max() < exact_ref_max() and np.array_equal((W4[:3, :3] @ L["d"].astype(np.float64).T).T, d2.astype(np.float64))
        # the baked vertices ARE the placed member vertices, by the contract's own point transform
        v, f = L["members"][L["mesh_of"][k]]
        lo = L["face_base"][k]
        baked = L["v"][L["f"][lo:lo + len(f)]].reshape(-1, 3)
        assert np.array_equal(scene_sim.points(L["M"][k], v[f].reshape(-1, 3)).astype(np.float64), baked.astype(np.float64))
    pairs, worst = SC.check_lattice_separation(L)
    print(f"lattice scene: {len(L['o'])} rays, {pairs} pairs of hits in different instances, the nearest {worst:.4g} relative apart")
    got = scene_sim.brute(L["members"], L["mesh_of"], L["M"], L["o"], L["d"])
    ties, other, mask = SC.check_against_ideal(L, got, "brute force")
    print(f"lattice scene: {ties} rays run through an edge or a vertex; held to the integer rule in each instance's frame, where {other} of them "
          f"name another face and {mask} have another hit mask than the rule on the baked mesh gives in the world frame")
    assert ties > 2000 and 0 < mask < other < ties // 4
    trees = [SimBVH(v, f) for v, f in L["members"]]
    for entries in (1, 0):
        RC.assert_same_bits(scene_sim.walk(trees, L["mesh_of"], L["M"], L["o"], L["d"], None, None, entries), got, f"lattice, stack_entries {entries}",
                            keys=SC.KEYS)


def exact_ref_max():
    import exact_ref
    return exact_ref.LATTICE_MAX


# ---- 5b. the written order of the transform ---------------------------------------------------------------------------------
def _round32(x):
    """the float32 nearest to the rational x, ties to even (x within the normal range)"""
    from fractions import Fraction
    if x == 0:
        return np.float32(0)
    c = np.float32(float(x))                      # a neighbour of the answer (the double rounding can be one step off)
    cands = sorted({c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))}, key=float)
    err = [abs(Fraction(float(y)) - x) for y in cands]
    best = min(err)
    win = [y for y, e in zip(cands, err) if e == best]
    if len(win) > 1:                              # a tie: the even mantissa
        win = [y for y in win if (y.view(np.uint32) & 1) == 0]
    return win[0]


def test_the_transform_is_the_written_fmaf_order_in_exact_rationals():
    """contract 3, restated without the header: o'x = fmaf(W00, ox, fmaf(W01, oy, fmaf(W02, oz, W03))) and
    d'x = fmaf(W00, dx, fmaf(W01, dy, W02 * dz)), every operation exact in rationals and rounded ONCE to float32.  On the
    general placements another association or an unfused multiply-add gives other bits on most rays (asserted)."""
    import scene_sim
    from fractions import Fraction
    F = lambda x: Fraction(float(x))      # noqa: E731
    fma = lambda a, b, c: _round32(F(a) * F(b) + F(c))      # noqa: E731
    s = SC.scenes()["many65"]
    W_, valid, _ = scene_sim.record(s["M"])
    fin = np.isfinite(s["o"]).all(1) & np.isfinite(s["d"]).all(1) & (np.abs(s["o"]).max(1) < 1e30) & (np.abs(s["d"]).max(1) < 1e30) & \
        (np.abs(s["d"]).min(1) > 1e-30) & (np.abs(s["o"]).min(1) > 1e-30)
    rays = np.flatnonzero(fin)[:40]
    other = total = 0
    for k in np.flatnonzero(valid)[:12]:
        Wk = W_[k].reshape(3, 4)
        o2, d2, ok = scene_sim.transform(s["M"][k], s["o"][rays], s["d"][rays])
        assert ok.all()
        for j, i in enumerate(rays):
            o, d = s["o"][i], s["d"][i]
            for r in range(3):
                want_o = fma(Wk[r, 0], o[0], fma(Wk[r, 1], o[1], fma(Wk[r, 2], o[2], Wk[r, 3])))
                want_d = fma(Wk[r, 0], d[0], fma(Wk[r, 1], d[1], _round32(F(Wk[r, 2]) * F(d[2]))))
                assert o2[j, r].view(np.uint32) == want_o.view(np.uint32) and d2[j, r].view(np.uint32) == want_d.view(np.uint32), (k, i, r)
                # what the unfused left-to-right sum of products would give
                plain = np.float32(np.float32(np.float32(Wk[r, 0] * o[0]) + np.float32(Wk[r, 1] * o[1])) + np.float32(Wk[r, 2] * o[2])) + Wk[r, 3]
                other += int(np.float32(plain).view(np.uint32) != want_o.view(np.uint32))
                total += 1
    assert total >= 1000 and other > total // 4, (other, total)      # the check can tell the orders apart
    # the point transform of the outputs (M applied to the object-space location) is the same chain
    M0 = s["M"][int(np.flatnonzero(valid)[0])]
    p = s["o"][rays]
    got = scene_sim.points(M0, p)
    for j in range(len(p)):
        for r in range(3):
            want = fma(M0[r, 0], p[j, 0], fma(M0[r, 1], p[j, 1], fma(M0[r, 2], p[j, 2], M0[r, 3])))
            assert got[j, r].view(np.uint32) == want.view(np.uint32)


# ---- 6. the inverse --------------------------------------------------------------------------------------------------------
def test_the_inverse_is_the_rounded_float64_inverse():
    import scene_sim
    Ms = np.concatenate([s["M"] for s in SC.scenes().values()] + [SC.lattice_scene()["M"]])
    W_, valid, flip = scene_sim.record(Ms)
    checked = 0
    for M, Wk, ok, fl in zip(Ms, W_.reshape(-1, 3, 4), valid, flip):
        M4 = np.eye(4)
        M4[:3] = M.astype(np.float64)
        det = np.linalg.det(M4[:3, :3]) if np.isfinite(M).all() else np.nan
        if not np.isfinite(M).all() or abs(det) < 1e-12 * np.abs(M4[:3, :3]).max() ** 3:
            assert not ok      # the NaN and the singular placements
            continue
        assert ok and fl == (det < 0)
        want = np.linalg.inv(M4)[:3].astype(np.float32)
        for row in range(3):
            ulp = np.spacing(np.abs(want[row]).max())
            assert (np.abs(Wk[row].astype(np.float64) - want[row].astype(np.float64)) <= 4 * float(ulp)).all(), (M, Wk, want)
        checked += 1
    assert checked >= 70
    # exact transforms give exact inverses
    L = SC.lattice_scene()
    Wl = scene_sim.record(L["M"])[0].reshape(-1, 3, 4)
    for M, Wk in zip(L["M"], Wl):
        M4, W4 = np.eye(4), np.eye(4)
        M4[:3], W4[:3] = M.astype(np.float64), Wk.astype(np.float64)
        assert np.array_equal(W4 @ M4, np.eye(4)) and np.array_equal(M4 @ W4, np.eye(4))      # (every product is exact in float64)
    for s in (2.0 ** -20, 2.0 ** 20, -0.5):
        Wk = scene_sim.record(SC.placement(np.eye(3) * s, [3, -5, 7])[None])[0].reshape(3, 4)
        assert np.array_equal(Wk[:, :3], np.eye(3, dtype=np.float32) / np.float32(s)) and np.array_equal(Wk[:, 3], np.float32([-3, 5, -7]) / np.float32(s))
