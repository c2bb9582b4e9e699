"""Shared by tests/test_scene_nearest_cpu.py and tests/test_gpu_scene_nearest.py (not a test module): the query points of every
scene of scene_cases for closest_point on scenes (csrc/tr_scene_nearest.h), the max_distance arrays, the brute force of each
computed once, the bit-for-bit comparison of two scene_nearest_sim.Result, the facts the fixtures must meet, the scene whose
placement overflows, a wave whose lanes have their winners in different instances, and the lattice scene of scene_cases with
its integer-baked mesh."""
import functools

import numpy as np

import nearest_cases as NC
import scene_cases as SC
import scene_points_cases as PC

F32 = np.float32
KEYS = ("closest", "distance", "instance", "tri")
KINDS = ("none", "hash", "exact", "below")      # the max_distance arrays of a scene: see max_distance_of


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_same(got, want, what, keys=KEYS):
    """two scene_nearest_sim.Result (or tuples in its order), bit for bit (NaN == NaN, -0 != +0); an output that `got` left
    out (None) is skipped"""
    for k in keys:
        g, w = got[KEYS.index(k)], want[KEYS.index(k)]
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        bad = (bits(g) != bits(w)).reshape(len(g), int(np.prod(g.shape[1:]))).any(1)
        assert not bad.any(), f"{what}: {k} differs at {np.flatnonzero(bad)[:8]}: {g[bad][:4]} != {w[bad][:4]}"


def usable(s):
    """the instances of a scene that can offer a candidate"""
    mem = SC.members()
    return [k for k, (m, M) in enumerate(zip(s["mesh_of"], s["M"]))
            if len(mem[m][1]) and m != SC.INACTIVE and np.isfinite(M).all() and abs(np.linalg.det(M[:, :3].astype(np.float64))) > 0]


@functools.lru_cache(maxsize=None)
def points_of(name):
    """float32 [n, 3] of scenes()[name]: hashed inside the world boxes of the instances grown by a tenth, the exact placed
    centres (the translation of every placement), placed vertices themselves -- distance 0, exact ties between the faces of a
    fan and between the two copies of two_same -- and a block of 60 hostile points (scene_points_cases.hostile_points)"""
    import scene_sim
    s = SC.scenes()[name]
    mem = SC.members()
    use = usable(s)
    parts = []
    for j, k in enumerate(use):
        lo, hi = SC.world_box(mem[s["mesh_of"][k]][0], s["M"][k])
        grow = PC.MARGIN * (hi - lo)
        big = len(mem[s["mesh_of"][k]][1]) > 1
        few = len(s["mesh_of"]) <= 8
        m = (max(120, 1500 // len(use)) if few else 50) if big else (60 if few else 8)
        parts.append(NC.hash_points(m, 900 + 17 * j, lo - grow, hi + grow))
    if len(s["M"]):
        centres = s["M"][:, :, 3].astype(F32)
        parts.append(centres[np.isfinite(centres).all(1)])
        for k in use:
            v = mem[s["mesh_of"][k]][0]
            parts.append(scene_sim.points(s["M"][k], v[::max(1, len(v) // (24 if len(s["mesh_of"]) <= 8 else 3))]))
    else:
        parts.append(NC.hash_points(300, 899, -np.ones(3), np.ones(3)))
    p = np.concatenate(parts)
    return np.ascontiguousarray(np.concatenate([p, PC.hostile_points(p[:60])]), F32)


def valid_points(p):
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(1)


@functools.lru_cache(maxsize=None)
def max_distance_of(name, kind):
    """None ('none': unbounded) or float32 [n] for points_of(name).  'hash': the unbounded answer's distance times a hashed factor in
    [0.25, 1.75] -- about half the points keep their answer --, with +Inf, NaN, a negative number, -0.0 and 0 sprinkled in;
    'exact': exactly the float32 distance of the unbounded answer (the float64 part decides: a d2 slightly above R2 can round
    to it); 'below': one float32 step below that"""
    if kind == "none":
        return None
    d = brute_of(name, "none").distance
    n = len(d)
    base = np.where(np.isfinite(d), d, F32(1))
    if kind == "hash":
        u = NC.hash_points(n, 4242, [0.25] * 3, [1.75] * 3)[:, 0]
        with np.errstate(over="ignore"):
            r = (base * u).astype(F32)
        r[3::41], r[5::43], r[7::47], r[11::53], r[13::59] = np.inf, np.nan, -1.0, -0.0, 0.0
        return r
    r = base.astype(F32)
    return r if kind == "exact" else np.nextafter(r, F32(-np.inf)).astype(F32)


@functools.lru_cache(maxsize=None)
def brute_of(name, kind="none"):
    """scene_nearest_sim.brute of scenes()[name] on points_of(name) under max_distance_of(name, kind), computed once"""
    import scene_nearest_sim
    s = SC.scenes()[name]
    return scene_nearest_sim.brute(SC.members(), s["mesh_of"], s["M"], points_of(name), max_distance_of(name, kind))


def renumbered(res, ninst):
    """the Result of the REVERSED listing of a scene in the numbering of the original one: instance k -> ninst - 1 - k"""
    return res._replace(instance=np.where(res.instance >= 0, ninst - 1 - res.instance, -1).astype(np.int32))


# ---- what the fixtures must be: asserted from the brute force, computed once and written down ------------------------------
# name -> (points, valid points, points with an answer, different instances that win somewhere, points at distance 0,
#          valid points with an exact tie in d2 between two different instances)
FACTS = {
    "none": (360, 324, 0, 0, 0, 0),
    "one_affine": (1586, 1550, 1550, 1, 25, 0),
    "two_same": (1612, 1576, 1576, 1, 50, 1576),
    "three": (1176, 1140, 1140, 3, 53, 24),
    "odd": (1330, 1294, 1294, 4, 79, 24),
    "many65": (1311, 1275, 1275, 62, 186, 24),
}


@functools.lru_cache(maxsize=None)
def cross_instance_ties(name):
    """bool [n]: the points with exactly the same float64 d2 to their winner and to a triangle of ANOTHER instance: the brute
    force of every usable instance on its own, compared in d2"""
    import scene_nearest_sim
    s = SC.scenes()[name]
    p = points_of(name)
    best = np.full(len(p), np.inf)
    times = np.zeros(len(p), np.int32)
    for k in usable(s):
        _, d2 = scene_nearest_sim.brute(SC.members(), s["mesh_of"][k:k + 1], s["M"][k:k + 1], p, None, want_d2=True)
        times = np.where(d2 < best, 1, times + (d2 == best))
        best = np.minimum(best, d2)
    return (times >= 2) & np.isfinite(best)


def facts_of(name):
    p, w = points_of(name), brute_of(name)
    ok = valid_points(p)
    return (len(p), int(ok.sum()), int((w.instance >= 0).sum()), len(set(w.instance[w.instance >= 0].tolist())),
            int((w.distance == 0).sum()), int(cross_instance_ties(name).sum()))


def check_fixture_conditions():
    """the facts the comparisons rest on, from the brute force alone (other points, not weaker asserts, if one fails)"""
    for name in SC.scenes():
        assert facts_of(name) == FACTS[name], f"{name}: {facts_of(name)}"
        p, w = points_of(name), brute_of(name)
        ok = valid_points(p)
        assert (~ok).sum() >= 30 and (w.instance[~ok] == -1).all() and (w.tri[~ok] == -1).all() and np.isinf(w.distance[~ok]).all() \
            and np.isnan(w.closest[~ok]).all(), name
        if name != "none":
            near = ok & (np.abs(np.where(ok[:, None], p, 0)) < 1e38).all(1)      # (at 3e38 the distance itself leaves the float32 range: +Inf)
            assert (w.instance[ok] >= 0).all() and np.isfinite(w.closest[ok]).all() and np.isfinite(w.distance[near]).all(), name
            assert np.isinf(w.distance[ok & ~near]).any(), name
    none = brute_of("none")
    assert (none.instance == -1).all() and np.isnan(none.closest).all()
    # two_same: equal placements, every point ties between the two copies, and the earlier one is named
    assert (brute_of("two_same").instance[valid_points(points_of("two_same"))] == 0).all() and FACTS["two_same"][5] == FACTS["two_same"][1]
    assert FACTS["three"][3] >= 3 and FACTS["many65"][3] >= 20
    # odd: the mirrored (0), tiny (1) and huge (2) copies each win somewhere; the singular (3), NaN (4), inactive (5) and
    # faceless (6) instances never do
    odd = brute_of("odd").instance
    assert all((odd == k).sum() > 20 for k in (0, 1, 2)) and not np.isin(odd, (3, 4, 5, 6)).any()
    # the bounded arrays decide something: some points keep their answer, some lose it, and the float64 part of an exact
    # bound goes both ways somewhere
    for name in SC.scenes():
        if name == "none":
            continue
        free, h, e, b = (brute_of(name, kind).instance >= 0 for kind in KINDS)
        assert (free & h).sum() > 100 and (free & ~h).sum() > 100, name
        assert (free & e).sum() > 100 and (free & ~b).sum() > 100, name
    kept = sum(int(((brute_of(n, "none").instance >= 0) & (brute_of(n, "exact").instance < 0)).sum()) for n in SC.scenes())
    assert kept > 0, "no point whose float32 distance equals max_distance while its d2 exceeds max_distance^2"


# ---- a placement that overflows ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def overflow_scene():
    """dict(members, mesh_of, M, p, want): ONE member that holds the sphere of scene_cases twice -- scaled to an extent of 1e10,
    and to 1e-3 -- placed by a full matrix of entries around 1e30 with both signs: the large copy's placed coordinates leave
    the float32 range (+-Inf; never NaN: the product inside an fmaf is exact, so an infinite partial sum meets a finite one),
    its triangles are inactive, its boxes place to infinite corners; the small copy lands around 1e27 and answers.  A second instance
    places the same member by a modest matrix: both copies answer there.  Nothing is NaN in an answer."""
    import scene_nearest_sim
    iv, if_ = SC.members()[SC.ICO]
    v = np.concatenate([iv * F32(1e10), iv * F32(1e-3)]).astype(F32)
    f = np.concatenate([if_, if_ + len(iv)]).astype(np.int32)
    big = SC.placement([[1e30, -1e30, 1e29], [1e29, 1e30, -1e30], [-1e30, 1e29, 1e30]], [0, 1e27, -1e27])
    small = SC.placement([[0, -2e-10, 0], [2e-10, 0, 0], [0, 0, -2e-10]], [5, 0, 0])
    members = [(v, f)]
    mesh_of, M = np.array([0, 0], np.int32), np.array([big, small], F32)
    p = np.concatenate([NC.hash_points(500, 31, [-4e27] * 3, [4e27] * 3), NC.hash_points(300, 32, [-1.5e38] * 3, [1.5e38] * 3),
                        NC.hash_points(400, 33, [2, -3, -3], [8, 3, 3]), PC.hostile_points(NC.hash_points(30, 34, [-1e27] * 3, [1e27] * 3))])
    want = scene_nearest_sim.brute(members, mesh_of, M, p)
    bv, bf, inst_of, tri_of = scene_nearest_sim.bake(members, mesh_of, M)
    act = NC.active(bv, bf)
    assert not act[(inst_of == 0) & (tri_of < len(if_))].any() and act[(inst_of == 0) & (tri_of >= len(if_))].all() and act[inst_of == 1].all()
    placed = bv[bf[(inst_of == 0) & (tri_of < len(if_))]]
    assert np.isinf(placed).any(axis=(1, 2)).all() and (placed == np.inf).any() and (placed == -np.inf).any() and not np.isnan(placed).any()
    ok = valid_points(p)
    assert (want.instance[ok] >= 0).all() and not np.isnan(want.closest[ok]).any() and not np.isnan(want.distance).any()
    assert ((want.instance == 0) & (want.tri >= len(if_))).sum() > 300 and (want.instance == 1).sum() > 300
    assert not ((want.instance == 0) & (want.tri < len(if_))).any()
    assert (want.instance[~ok] == -1).all()
    return dict(members=members, mesh_of=mesh_of, M=M, p=p, want=want)


# ---- waves whose lanes part ways --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def split_waves():
    """(mesh_of, M, points, the brute force): three spheres in a row, 10 apart.  Points 0 .. 63: even lanes next to the first
    instance, odd lanes next to the third.  64 .. 127: every lane invalid.  128 .. 255: a whole block of invalid points
    follows in 256 .. 383.  Then: lanes in turn next to the first, second and third, and 1 500 points hashed around all"""
    import scene_nearest_sim
    rng = np.random.default_rng(3)
    M = np.array([SC.placement(SC.general(rng, 0.9), [-10, 0, 0]), SC.placement(np.eye(3), [0, 0, 0]), SC.placement(SC.general(rng, 0.9), [10, 0, 0])])
    mesh_of = np.array([SC.ICO, SC.SHELLS, SC.ICO], np.int32)
    jitter = NC.hash_points(64, 5, [-0.3] * 3, [0.3] * 3)
    w0 = jitter.copy()
    w0[0::2, 0] -= 10
    w0[1::2, 0] += 10
    w1 = PC.hostile_points(NC.hash_points(64, 6, [-1] * 3, [1] * 3))
    w1[(np.isfinite(w1).all(1))] = np.nan      # (3e38 is finite: here every lane is to be invalid)
    w2 = NC.hash_points(128, 7, [-12, -2, -2], [12, 2, 2])
    w3 = np.full((128, 3), np.inf, F32)
    w4 = (np.array([[-10, 0, 0], [0, 0, 0], [10, 0, 0]], F32)[np.arange(64) % 3] + jitter).astype(F32)
    rest = NC.hash_points(1500, 8, [-13, -3, -3], [13, 3, 3])
    p = np.ascontiguousarray(np.concatenate([w0, w1, w2, w3, w4, rest]), F32)
    want = scene_nearest_sim.brute(SC.members(), mesh_of, M, p)
    assert np.array_equal(want.instance[:64], np.tile(np.int32([0, 2]), 32))
    assert (want.instance[64:128] == -1).all() and (want.instance[256:384] == -1).all() and (want.instance[128:256] >= 0).all()
    assert np.array_equal(want.instance[384:448], (np.arange(64) % 3).astype(np.int32))
    assert all((want.instance[448:] == k).sum() > 200 for k in range(3))
    return mesh_of, M, p, want


# ---- the lattice scene of scene_cases: placements that are exact in float32 ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice():
    """dict(members, mesh_of, M, p, want): SC.lattice_scene() -- signed permutations with power-of-two scales and integer
    translations, so the float32 chain places every vertex EXACTLY -- and integer and half-integer points in and around it.
    want: nearest_sim.brute on the INTEGER-baked mesh (L["v"], computed in int64 without the chain) with the baked face index
    mapped back by face_base"""
    import nearest_sim
    L = SC.lattice_scene()
    rng = np.random.default_rng(9)
    parts = []
    for lo, hi in L["boxes"]:
        parts.append(rng.integers(2 * lo - 6, 2 * hi + 7, (220, 3)) / 2)
    parts.append(rng.integers(-10, 75, (400, 3)).astype(np.float64))
    parts.append(L["v"][::7].astype(np.float64))      # placed vertices themselves: distance 0, ties around a vertex
    p = np.ascontiguousarray(np.concatenate(parts), F32)
    closest, distance, t = nearest_sim.brute(L["v"].astype(F32), L["f"].astype(np.int32), p)
    inst = (np.searchsorted(L["face_base"], t, "right") - 1).astype(np.int32)
    tri = (t - L["face_base"][inst]).astype(np.int32)
    assert (t >= 0).all() and (distance == 0).sum() > 50 and all((inst == k).sum() > 50 for k in range(len(L["mesh_of"])))
    return dict(members=L["members"], mesh_of=L["mesh_of"], M=L["M"], p=p, want=(closest, distance, inst, tri))
