"""Shared by tests/test_scene_cross_cpu.py and tests/test_gpu_scene_cross.py (not a test module): the bit-for-bit comparison
of two scene_cross_sim.Result, the brute force of every scene of scene_cases computed once, the facts the fixtures must
meet, the stack of quads placed three times (long lists whose rows interleave between instances), and the lattice scene of
scene_cases against its integer-arithmetic ideal."""
import functools

import numpy as np

import cross_cases as CC
import range_cases as RC
import scene_cases as SC

KEYS = ("count", "offsets", "instance", "faces", "t", "front", "loc", "uv", "ray")
F32 = np.float32


def assert_same(got, want, what, keys=KEYS):
    """two scene_cross_sim.Result, bit for bit (cross_cases.assert_same with the instance column)"""
    CC.assert_same(got, want, what, keys=keys)


def rows_of(res, i):
    return slice(int(res.offsets[i]), int(res.offsets[i + 1]))


def instances_per_ray(res):
    """[n]: in how many different instances ray i has a crossing"""
    ray = np.repeat(np.arange(len(res.count)), res.count)
    pairs = np.unique(np.stack([ray, res.instance.astype(np.int64)], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=len(res.count))


def bounds_of(name, kind):
    """(tmin, tmax) of scenes()[name]: 'none', 'hash' (the scene's own) or 'exact' (placed on the hits of the unbounded scene
    brute force: scene_cases.exact_bounds)"""
    s = SC.scenes()[name]
    if kind == "none":
        return None, None
    if kind == "hash":
        return s["lo"], s["hi"]
    return SC.brute_of(name, "exact")[:2]


@functools.lru_cache(maxsize=None)
def brute_of(name, kind):
    """scene_cross_sim.brute of scenes()[name] under the bounds `kind`, computed once"""
    import scene_cross_sim
    s = SC.scenes()[name]
    lo, hi = bounds_of(name, kind)
    return scene_cross_sim.brute(SC.members(), s["mesh_of"], s["M"], s["o"], s["d"], lo, hi)


def renumbered(res, ninst):
    """the Result of the REVERSED listing of a scene in the numbering of the original one: instance k -> ninst - 1 - k, and
    the rows of each ray ordered again by (t, instance, face) -- rows with equal t swap places"""
    inst = (ninst - 1 - res.instance).astype(np.int32)
    ray = np.repeat(np.arange(len(res.count)), res.count)
    order = np.lexsort((res.faces, inst, res.t, ray))
    return res._replace(instance=inst[order], faces=res.faces[order], t=res.t[order], front=res.front[order], loc=res.loc[order], uv=res.uv[order])


# ---- what the fixtures must be: asserted from the brute force -------------------------------------------------------------
def check_fixture_conditions():
    """the facts the comparisons rest on, from the brute force alone (other rays, not weaker asserts, if one fails)"""
    two = brute_of("two_same", "none")
    per = instances_per_ray(two)
    assert len(two.count) == 2210 and len(two.t) == 2892 and (per >= 2).sum() == 1216
    # equal placements: every crossing appears in both instances with identical t bits -- the (t, instance) tie
    a, b = two.instance == 0, two.instance == 1
    assert a.sum() == b.sum() == 1446 and np.array_equal(two.faces[a], two.faces[b]) and np.array_equal(RC.bits(two.t[a]), RC.bits(two.t[b]))
    assert np.array_equal(two.instance.reshape(-1, 2), np.tile(np.int32([0, 1]), (1446, 1)))
    three = brute_of("three", "none")
    per = instances_per_ray(three)
    assert (per >= 2).sum() == 337 and (per >= 3).sum() == 126 and three.count.max() == 13
    assert (instances_per_ray(brute_of("three", "hash")) >= 2).sum() == 90
    many = brute_of("many65", "none")
    per = instances_per_ray(many)
    assert (per >= 2).sum() == 574 and (per >= 3).sum() == 231 and per.max() == 6 and many.count.max() == 16
    for kind in ("none", "hash", "exact"):
        none = brute_of("none", kind)
        assert len(none.t) == 0 and not none.count.any()
    for name, s in SC.scenes().items():      # hostile rays and bounds (`bad` is about the scene's own bounds) cross nothing
        w = brute_of(name, "hash")
        assert s["bad"].sum() > 20 and not w.count[s["bad"]].any() and not np.isnan(w.t).any(), name
        assert name == "none" or (w.count[~s["bad"]] > 0).sum() > 100, name


# ---- long, interleaved lists: the stack of quads placed three times ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quad_scene():
    """dict(members, mesh_of, M, o, d, expected): cross_cases.quad_stack() as ONE member placed at the identity, at the
    identity again and translated by (0, 0, 0.25).  A ray that reaches m squares crosses 3 m placed squares: copies 0 and 1
    at t = k - 1/2 (a tie, broken by the instance), copy 2 at t = k - 1/4, so the rows of the three instances interleave
    0 1 2 0 1 2 ..."""
    v, f, o, d, expected = CC.quad_stack()
    M = np.array([SC.placement(np.eye(3), [0, 0, 0]), SC.placement(np.eye(3), [0, 0, 0]), SC.placement(np.eye(3), [0, 0, 0.25])], F32)
    return dict(members=[(v, f)], mesh_of=np.zeros(3, np.int32), M=M, o=o, d=d, expected=expected)


def check_quad_scene(res, what):
    """a Result on quad_scene() (default bounds) against what the scene says"""
    q = quad_scene()
    # a ray of `expected` squares crosses them in the copies 0 and 1; the copy 0.25 higher is left sideways no later
    assert np.array_equal(res.count[q["expected"] == 0], np.zeros((q["expected"] == 0).sum(), np.int32)), what
    wave = res.count[:64]
    assert (wave == 0).any() and (wave >= 100).any(), f"{what}: the first wave holds lists of {sorted(set(wave.tolist()))} rows"
    i = int(np.flatnonzero(res.count >= 100)[0])
    rows = rows_of(res, i)
    inst, t = res.instance[rows], res.t[rows]
    assert np.array_equal(inst[:99], np.tile(np.int32([0, 1, 2]), 33)), f"{what}: ray {i} does not interleave the instances: {inst[:12]}"
    assert np.array_equal(RC.bits(t[0:99:3]), RC.bits(t[1:99:3])) and (t[2:99:3] > t[1:99:3]).all() and (t[3:99:3] > t[2:96:3]).all()
    assert np.array_equal(res.faces[rows][0:99:3], res.faces[rows][1:99:3])


# ---- the lattice scene of scene_cases against integer arithmetic ------------------------------------------------------------
def check_lattice(res, what):
    """a Result on SC.lattice_scene() (default bounds, every ray) against exact_ref.lattice on the baked mesh.
    Rays without a tie (~ideal.tie): the count is len(ideal.sets[i]), the set of (instance, tri) mapped through face_base is
    the ideal's, and consecutive rows follow the exact order of scene_cases.exact_distances wherever those distances differ by
    at least 2^-8 relative (four times the 2^-11 bound on a float32 distance).  Tie rays: count > 0 equals the hit mask of
    lattice_frame_ideal().  -> (rays compared in full, pairs of consecutive rows whose order was checked)"""
    L = SC.lattice_scene()
    ideal = L["ideal"]
    vi, fi = L["v"], L["f"]
    oi, di = L["o"].astype(np.int64), L["d"].astype(np.int64)
    baked = L["face_base"][res.instance] + res.faces
    assert len(res.count) == len(L["o"])
    full = pairs = 0
    for i in np.flatnonzero(~ideal.tie):
        rows = rows_of(res, i)
        want = ideal.sets[i] if ideal.sets[i] is not None else np.zeros(0, np.int32)
        assert res.count[i] == len(want), f"{what}: ray {i} has {res.count[i]} rows, the ideal {len(want)}"
        got = baked[rows]
        assert np.array_equal(np.sort(got), np.sort(want)), f"{what}: ray {i} lists the baked faces {np.sort(got)}, the ideal {np.sort(want)}"
        full += 1
        if len(got) >= 2:
            t = SC.exact_distances(vi, fi, oi[i], di[i], got)
            apart = np.abs(t[1:] - t[:-1]) >= 2.0 ** -8 * np.maximum(t[1:], t[:-1])
            assert (t[1:] > t[:-1])[apart].all(), f"{what}: ray {i} is out of the exact order: {t}"
            pairs += int(apart.sum())
    rays, fhit = SC.lattice_frame_ideal()[:2]
    assert np.array_equal(rays, np.flatnonzero(ideal.tie))
    bad = (res.count[rays] > 0) != fhit
    assert not bad.any(), f"{what}: count > 0 differs from the rule in the instances' frames on {int(bad.sum())} tie rays, first {rays[bad][:8]}"
    return full, pairs
