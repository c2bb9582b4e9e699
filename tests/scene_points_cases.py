"""Shared by tests/test_scene_points_cpu.py and tests/test_gpu_scene_points.py (not a test module): the query points of every
scene of scene_cases for contains_points on scenes (csrc/tr_scene_points.h), the brute force of each computed once, the
bit-for-bit comparison of two scene_points_sim.Result, the facts the fixtures must meet, and the lattice scene of scene_cases
against integer parity."""
import functools

import numpy as np

import exact_ref
import nearest_cases as NC
import scene_cases as SC

F32 = np.float32
DEFAULT = np.array([0.4395064455, 0.617598629942, 0.652231566745], F32)      # RayMeshIntersector._DEFAULT_DIRECTION
OTHER = np.array([-0.3, 0.8, 0.52], F32)                                      # another direction (the misdirected fill)
MARGIN = 0.1                                                                  # of the box's size, on every side
CLOSED = (SC.ICO, SC.SHELLS)


def assert_same(got, want, what, keys=None):
    """two scene_points_sim.Result, bit for bit"""
    for k in keys or want._fields:
        g, w = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        assert np.array_equal(g, w), f"{what}: {k} differs at {np.flatnonzero((g != w).reshape(len(g), -1).any(1))[:8]}"


def hostile_points(base):
    """copies of the points `base` with NaN, +Inf, -Inf and 3e38 put into one, two or all three components in turn.  A
    non-finite component makes the point invalid; 3e38 is finite, and leaves the float32 range in any instance's frame that
    scales it up: inside nothing either way"""
    p = np.array(base, F32)
    values = (np.nan, np.inf, -np.inf, 3e38, -3e38)
    masks = ((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2))
    for i in range(len(p)):
        for axis in masks[(i // len(values)) % len(masks)]:
            p[i, axis] = values[i % len(values)]
    return p


def regions(s):
    """[(lo, hi, points)] of a scene: the world box of every instance that can hold or be crossed by something, grown by
    MARGIN on every side; closed members get most of the points"""
    mem = SC.members()
    out = []
    usable = [k for k, (m, M) in enumerate(zip(s["mesh_of"], s["M"]))
              if len(mem[m][1]) and m != SC.INACTIVE and np.isfinite(M).all() and abs(np.linalg.det(M[:, :3].astype(np.float64))) > 0]
    nclosed = sum(int(s["mesh_of"][k]) in CLOSED for k in usable)
    for k in usable:
        lo, hi = SC.world_box(mem[s["mesh_of"][k]][0], s["M"][k])
        grow = MARGIN * (hi - lo)
        closed = int(s["mesh_of"][k]) in CLOSED
        out.append((lo - grow, hi + grow, max(250, 2400 // max(nclosed, 1)) if closed else (60 if len(s["mesh_of"]) <= 8 else 12)))
    return out


@functools.lru_cache(maxsize=None)
def points_of(name):
    """float32 [n, 3] of scenes()[name]: hashed inside the grown world boxes of the instances, the exact placed centres (the
    translation of every placement), and a block of 60 hostile points"""
    s = SC.scenes()[name]
    parts = [NC.hash_points(m, 500 + 13 * j, lo, hi) for j, (lo, hi, m) in enumerate(regions(s))]
    if len(s["M"]):
        centres = s["M"][:, :, 3].astype(F32)
        parts.append(centres[np.isfinite(centres).all(1)])
    else:
        parts.append(NC.hash_points(300, 499, -np.ones(3), np.ones(3)))
    p = np.concatenate(parts)
    return np.ascontiguousarray(np.concatenate([p, hostile_points(p[:60])]), F32)


def valid_points(p):
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(1) & (np.abs(p) < 1e38).all(1)


@functools.lru_cache(maxsize=None)
def counts_of(name, which="default"):
    import scene_points_sim
    s = SC.scenes()[name]
    return scene_points_sim.counts(SC.members(), s["mesh_of"], s["M"], points_of(name), DEFAULT if which == "default" else OTHER)


@functools.lru_cache(maxsize=None)
def brute_of(name, which="default"):
    """scene_points_sim.brute of scenes()[name] on points_of(name) along DEFAULT (or OTHER), computed once"""
    import scene_points_sim
    return scene_points_sim.reduce(*counts_of(name, which))


def renumbered(res, ninst):
    """the Result of the REVERSED listing of a scene in the numbering of the original one: instance k -> ninst - 1 - k, the
    rows of each point ascending again"""
    pt = np.repeat(np.arange(len(res.count)), res.count)
    inst = (ninst - 1 - res.instance).astype(np.int32)
    return res._replace(instance=inst[np.lexsort((inst, pt))])


def rows_of(res, i):
    return res.instance[int(res.offsets[i]):int(res.offsets[i + 1])]


# ---- what the fixtures must be: asserted from the brute force -------------------------------------------------------------
# name -> (points, valid points, valid points inside some instance, rows, points inside two or more DIFFERENT instances)
FACTS = {}


def facts_of(name):
    s = SC.scenes()[name]
    p, w = points_of(name), brute_of(name)
    ok = valid_points(p)
    distinct = np.array([len(set(rows_of(w, i).tolist())) for i in range(len(p))])
    if name == "two_same":      # (equal placements: one and the same solid twice)
        distinct = np.minimum(distinct, 1)
    return (len(p), int(ok.sum()), int((w.count[ok] > 0).sum()), int(w.offsets[-1]), int((distinct >= 2).sum())), s


def check_fixture_conditions():
    """the facts the comparisons rest on, from the brute force alone (other points, not weaker asserts, if one fails)"""
    for name in SC.scenes():
        got, s = facts_of(name)
        assert got == FACTS[name], f"{name}: {got}"
        p, w = points_of(name), brute_of(name)
        ok = valid_points(p)
        assert (~ok).sum() >= 50 and not w.count[~ok].any() and not w.any[~ok].any(), name
        assert np.array_equal(w.any, w.count > 0)
        if name != "none":
            assert 5 * got[2] >= got[1], f"{name}: {got[2]} of {got[1]} valid points are inside some instance"
            centres = s["M"][:, :, 3][np.isfinite(s["M"][:, :, 3]).all(1)]
            assert np.array_equal(p[len(p) - 60 - len(centres):len(p) - 60], centres), f"{name}: the exact placed centres"
    assert not brute_of("none").any.any() and len(brute_of("none").instance) == 0
    two = brute_of("two_same")
    assert set(two.count.tolist()) == {0, 2} and np.array_equal(two.instance.reshape(-1, 2), np.tile(np.int32([0, 1]), (len(two.instance) // 2, 1)))
    assert FACTS["three"][4] > 100 and FACTS["many65"][4] > 0      # (the closed copies of many65 sit 1.6 apart: few overlaps)
    # the open triangle: crossed by exactly one of a point's two rays for some points, and holding none
    for name, k in (("three", 2), ("odd", 7)):
        assert SC.scenes()[name]["mesh_of"][k] == SC.TRI
        cp, cm = counts_of(name)
        assert ((cp[k] + cm[k]) == 1).sum() > 20 and not ((cp[k] & 1) & (cm[k] & 1)).any(), name
        assert not (brute_of(name).instance == k).any()
    # the shortcut has something to skip and something to walk: first counts of both parities, odd first counts that the
    # second pass turns down
    cp, cm = counts_of("three")
    assert ((cp & 1) == 0).any() and ((cp & 1) == 1).any() and (((cp & 1) == 1) & ((cm & 1) == 0)).sum() > 20


FACTS.update({
    "none": (360, 300, 0, 0, 0),
    "one_affine": (2461, 2401, 562, 562, 0),
    "two_same": (2462, 2402, 711, 1422, 0),
    "three": (2523, 2463, 1024, 1228, 204),
    "odd": (2527, 2467, 1918, 3215, 1049),
    "many65": (3725, 3665, 884, 890, 6),
})


# ---- open members: where the answer depends on the direction ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def open_scene():
    """dict(members, mesh_of, M, p, mine, theirs): the sphere of scene_cases with its cap (face centroids above z = 0.6)
    taken off, placed twice, and the whole sphere once, interpenetrating.  A point inside a capless copy is held by it only
    when neither of its two rays leaves through the hole, so the counts along DEFAULT (mine) and along OTHER (theirs)
    differ -- which they never do on closed members: these are the counts a caller can misdirect."""
    import scene_points_sim
    iv, if_ = SC.members()[SC.ICO]
    keep = iv[if_].mean(1)[:, 2] <= 0.6
    members = [(iv, np.ascontiguousarray(if_[keep])), (iv, if_)]
    rng = np.random.default_rng(8)
    M = np.array([SC.placement(SC.rotation([1, 0, 0], 0.9), [-0.5, 0, 0]), SC.placement(np.eye(3) * 0.8, [0.3, 0.2, 0]),
                  SC.placement(SC.general(rng), [0.2, -0.3, 0.4])], F32)
    mesh_of = np.array([0, 1, 0], np.int32)
    p = NC.hash_points(2500, 61, [-1.8] * 3, [1.8] * 3)
    mine = scene_points_sim.brute(members, mesh_of, M, p, DEFAULT)
    theirs = scene_points_sim.brute(members, mesh_of, M, p, OTHER)
    assert 1.0 > keep.mean() > 0.7 and (mine.count > theirs.count).sum() > 20 and (mine.count < theirs.count).sum() > 20 and (mine.count >= 2).sum() > 100
    return dict(members=members, mesh_of=mesh_of, M=M, p=p, mine=mine, theirs=theirs)


def check_misdirected_rows(rows, mine, theirs, total, written, what, in_order=True):
    """rows [total] of a fill that was handed theirs.count / theirs.offsets and `total` on the query of `mine`; written
    [total] bool: which rows the fill wrote.  At the rows of point i: as many of the instances that hold it as fit, ascending
    (in_order: the first ones), and nothing after them"""
    for i in range(len(mine.count)):
        lo, hi = int(theirs.offsets[i]), min(int(theirs.offsets[i + 1]), total)
        full = rows_of(mine, i)
        k = min(len(full), hi - lo) if hi > lo else 0
        mine_i = rows[lo:lo + k]
        assert written[lo:lo + k].all() and not written[lo + k:hi].any(), f"{what}: point {i} wrote {written[lo:hi]}, holds {full}"
        assert np.isin(mine_i, full).all() and (np.diff(mine_i) > 0).all(), f"{what}: point {i} has the rows {mine_i}, holds {full}"
        assert not in_order or np.array_equal(mine_i, full[:k]), f"{what}: point {i} has the rows {mine_i}, holds {full}"


# ---- waves whose lanes part ways ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def split_waves():
    """(mesh_of, M, points, the brute force): three closed members in a row, 10 apart.  Points 0 .. 63: even lanes inside the
    first instance, odd lanes inside the third.  64 .. 127: far off to the side, no ray crosses anything.  128 .. 191: inside
    the second instance alone.  192 .. 255: outside everything, behind a copy along -d, so that the +d ray passes through
    it (first counts even, and not zero).  Then 2 100 points hashed around the three copies."""
    import scene_points_sim
    rng = np.random.default_rng(3)
    M = np.array([SC.placement(SC.general(rng, 0.9), [-10, 0, 0]), SC.placement(np.eye(3), [0, 0, 0]), SC.placement(SC.general(rng, 0.9), [10, 0, 0])])
    mesh_of = np.array([SC.ICO, SC.ICO, SC.ICO], np.int32)
    jitter = NC.hash_points(64, 5, [-0.05] * 3, [0.05] * 3)
    w0 = jitter.copy()
    w0[0::2, 0] -= 10
    w0[1::2, 0] += 10
    w1 = NC.hash_points(64, 6, [-1, 40, -1], [1, 60, 1])
    w2 = jitter
    w3 = (np.array([[-10, 0, 0], [0, 0, 0], [10, 0, 0]], F32)[np.arange(64) % 3] - 4 * DEFAULT + jitter).astype(F32)
    rest = np.concatenate([NC.hash_points(700, 7 + k, [c - 1.3, -1.3, -1.3], [c + 1.3, 1.3, 1.3]) for k, c in enumerate((-10, 0, 10))])
    p = np.ascontiguousarray(np.concatenate([w0, w1, w2, w3, rest]), F32)
    want = scene_points_sim.brute(SC.members(), mesh_of, M, p, DEFAULT)
    cp, cm = scene_points_sim.counts(SC.members(), mesh_of, M, p, DEFAULT)
    assert np.array_equal(want.instance[:64], np.tile(np.int32([0, 2]), 32)) and (want.count[:64] == 1).all()
    assert not want.any[64:128].any() and not cp[:, 64:128].any() and not cm[:, 64:128].any()
    assert (want.count[128:192] == 1).all() and (rows_of(want, 128) == 1).all() and (want.instance[64:128] == 1).all()
    assert not want.any[192:256].any() and (cp[:, 192:256] % 2 == 0).all() and (cp[:, 192:256] > 0).any(0).sum() > 40
    assert (want.count[256:] > 0).sum() > 300 and (want.count[256:] == 0).sum() > 300
    return mesh_of, M, p, want


# ---- the lattice scene of scene_cases against integer parity -----------------------------------------------------------------
LATTICE_DIRECTIONS = (DEFAULT, np.array([1, 0, 0], F32), np.array([1, 1, 1], F32), np.array([2, -1, 3], F32), np.array([0, -1, 0], F32))


@functools.lru_cache(maxsize=None)
def lattice_points():
    """dict(p float32 [n, 3]: integer points and points at odd multiples of 1/2 in and around every instance of
    SC.lattice_scene(), those on a placed surface left out; inside bool [ninst, n]: exact_ref.axis_parity on each instance's
    baked integer cube (False for the open heightfield, which is left to the brute force); closed [ninst]; ties [ndir - 1]:
    for each lattice direction, from how many of every fourth point d or -d runs exactly through an edge or a vertex of a
    placed cube)"""
    L = SC.lattice_scene()
    v, f, base = L["v"], L["f"], list(L["face_base"]) + [len(L["f"])]
    rng = np.random.default_rng(5)
    parts = []
    for lo, hi in L["boxes"]:
        parts.append(rng.integers(2 * lo - 4, 2 * hi + 5, (260, 3)))                       # doubled coordinates: both parities
        parts.append(rng.integers(lo - 1, hi + 2, (140, 3)) * 2)                           # integer points
    p2 = np.concatenate(parts).astype(np.int64)
    ninst = len(L["mesh_of"])
    names = [name for name, *_ in SC._LATTICE_INSTANCES]
    closed = np.array([n != "heightfield" for n in names])
    on = np.zeros(len(p2), bool)
    for k in range(ninst):
        on |= exact_ref.on_surface(v, f[base[k]:base[k + 1]], p2)
    p2 = p2[~on]
    inside = np.zeros((ninst, len(p2)), bool)
    for k in np.flatnonzero(closed):
        inside[k] = exact_ref.axis_parity(v, f[base[k]:base[k + 1]], p2)
    ties = []
    for d in LATTICE_DIRECTIONS[1:]:
        di = d.astype(np.int64)
        n = 0
        for i in range(0, len(p2), 4):      # (every fourth point: the count only shows that such points are there)
            for s in (1, -1):
                for k in np.flatnonzero(closed):
                    if SC.met_faces(v * 2, f[base[k]:base[k + 1]], p2[i], s * di)["edge"].any():
                        n += 1
                        break
                else:
                    continue
                break
        ties.append(n)
    return dict(p=(p2 / 2).astype(F32), inside=inside, closed=closed, ties=ties)


def check_lattice(res_of_direction, what):
    """res_of_direction: LATTICE_DIRECTIONS index -> a Result on lattice_points()["p"].  Every closed instance against the integer parity,
    along every direction"""
    P = lattice_points()
    n = P["p"].shape[0]
    assert n > 1500 and (P["inside"].sum(1)[P["closed"]] > 40).all() and min(P["ties"]) > 25, (n, P["inside"].sum(1), P["ties"])
    for j in range(len(LATTICE_DIRECTIONS)):
        res = res_of_direction(j)
        pt = np.repeat(np.arange(n), res.count)
        got = np.zeros_like(P["inside"])
        got[res.instance, pt] = True
        for k in np.flatnonzero(P["closed"]):
            bad = np.flatnonzero(got[k] != P["inside"][k])
            assert len(bad) == 0, f"{what}, direction {LATTICE_DIRECTIONS[j]}: instance {k} differs from the integer parity at points {P['p'][bad][:6]}"
