"""Shared by tests/test_cross_cpu.py and tests/test_gpu_cross.py (not a test module): the bit-for-bit comparison of two
cross_sim.Result, the scenes with analytically known lists (the sheet scene of range_cases, a stack of 40 quads), the
narrower bounds of the misuse checks, and the lattice scenes of exact_ref against their integer-arithmetic ideal."""
import functools
from fractions import Fraction

import numpy as np

import exact_ref as X
import range_cases as RC

KEYS = ("count", "offsets", "faces", "t", "front", "loc", "uv", "ray")


def assert_same(got, want, what, keys=KEYS):
    """two cross_sim.Result, bit for bit (NaN == NaN, -0 != +0); a field that is None in `got` was not asked for"""
    for k in keys:
        g, w = getattr(got, k), getattr(want, k)
        if g is None:
            continue
        g = np.asarray(g)
        assert g.shape == w.shape, f"{what}: {k} has shape {g.shape}, expected {w.shape}"
        same = RC.bits(g) == RC.bits(w)
        if not same.all():
            rows = np.flatnonzero(~same.reshape(len(w), -1).all(1))
            raise AssertionError(f"{what}: {k} differs on {len(rows)} of {len(w)} rows, first {rows[:8]}: {g[rows[:4]]} != {w[rows[:4]]}")


def rows_of(res, i):
    return slice(int(res.offsets[i]), int(res.offsets[i + 1]))


def narrower(lo, hi):
    """bounds inside [lo, hi]: the middle half of each interval"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    w = hi - lo
    return (lo + np.float32(0.25) * w).astype(np.float32), (hi - np.float32(0.25) * w).astype(np.float32)


# ---- the sheet scene: one row per sheet in range, at even integers ------------------------------------------------------------
def check_sheets(res, lo, hi, count, what):
    """a Result on RC.sheet_cases against what the scene says: the listed count, one row per sheet in range in order, every t
    the exact even integer, front everywhere"""
    assert np.array_equal(res.count, count), f"{what}: count {res.count[res.count != count][:8]} != {count[res.count != count][:8]}"
    assert res.offsets[-1] == count.sum() == len(res.faces)
    assert res.front.all(), what
    sheet = res.faces // RC.TRIS_PER_SHEET + 1
    assert np.array_equal(res.t, (2 * sheet).astype(np.float32)), f"{what}: a distance is not the even integer of its sheet"
    with np.errstate(invalid="ignore"):
        lo2, hi2 = np.maximum(lo, 0), np.minimum(hi, np.float32(1e7))
    for i in np.flatnonzero(count > 0):
        want = np.array([k for k in range(1, RC.SHEETS + 1) if lo2[i] <= 2 * k <= hi2[i]])
        assert np.array_equal(sheet[rows_of(res, i)], want), f"{what}: ray {i} lists the sheets {sheet[rows_of(res, i)]}, in range are {want}"
    assert np.array_equal(res.loc[:, 2], sheet.astype(np.float32)), what


# ---- a stack of parallel quads: lists of very different lengths side by side -------------------------------------------------
QUADS = 40
QUAD_CROSSINGS = (0, 1, 2, 3, 33, 40)


def quad_stack():
    """(v, f, o, d, expected): 40 squares [0, 10]^2 at z = 1 .. 40 (80 triangles) and 300 rays from z = 1/2 that drift along x
    and leave the stack sideways after 0, 1, 2, 3, 33 or 40 of them, interleaved so that every block holds every length.
    Square k is met at t = k - 1/2."""
    vs, fs = [], []
    for k in range(1, QUADS + 1):
        b = len(vs)
        vs += [(0, 0, k), (10, 0, k), (10, 10, k), (0, 10, k)]
        fs += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    n = 300
    expected = np.tile(np.array(QUAD_CROSSINGS, np.int32), n // len(QUAD_CROSSINGS))
    y = (0.7 + 8.5 * ((np.arange(n) * 0.6180339887) % 1.0)).astype(np.float32)
    o = np.stack([np.full(n, 0.3, np.float32), y, np.full(n, 0.5, np.float32)], 1)
    # x(z) = 0.3 + dx (z - 1/2): inside [0, 10] at z = m, outside at z = m + 1
    dx = np.where(expected > 0, 9.7 / np.maximum(expected, 1), 0.0).astype(np.float32)
    d = np.stack([dx, np.full(n, 0.003, np.float32), np.ones(n, np.float32)], 1)
    o[expected == 0, 0] = 20.0          # beside the stack
    return np.array(vs, np.float32), np.array(fs, np.int32), np.ascontiguousarray(o), np.ascontiguousarray(d), expected


def check_quad_stack(res, expected, tmax, what):
    """square k is crossed at t = k - 1/2 (within float32 rounding of the hit distance): a ray lists min(expected, those
    with k - 1/2 <= tmax) squares, in order, one triangle of each"""
    reach = QUADS if tmax is None else int(np.floor(tmax + 0.5))
    want = np.minimum(expected, reach)
    assert np.array_equal(res.count, want), f"{what}: count {res.count[res.count != want][:8]} != {want[res.count != want][:8]}"
    for i in range(len(expected)):
        rows = rows_of(res, i)
        assert np.array_equal(res.faces[rows] // 2, np.arange(want[i])), f"{what}: ray {i}"
        assert np.allclose(res.t[rows], np.arange(want[i]) + 0.5, rtol=2.0 ** -11, atol=0), f"{what}: ray {i}"


# ---- the lattice scenes of exact_ref: the list against integer arithmetic -------------------------------------------------
LATTICE_SCENES = ("cube1", "cube2", "cube5", "cube8", "nested3", "heightfield", "fan3", "fan8", "fan64")
@functools.lru_cache(maxsize=None)
def lattice_lists(name):
    """(scene, ideal, t): t[i] = the exact distances (Fractions) of ideal.sets[i], face by face"""
    s = next(s for s in X.lattice_scenes() if s["name"] == name)
    ideal = X.lattice_ideal(name)
    ray = np.repeat(np.arange(len(s["o"])), ideal.count)
    tri = np.concatenate([x for x in ideal.sets] + [np.zeros(0, np.int32)])
    c = X.pairs(s["v"], s["f"], s["o"][ray], s["d"][ray], tri)
    assert np.asarray(c["hit"], bool).all()
    flat = [Fraction(int(a), int(b)) for a, b in zip(c["tn"], c["td"])]
    off = np.concatenate([[0], np.cumsum(ideal.count)])
    return s, ideal, [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def check_lattice(name, res, what):
    """count and ordered face list of a Result (default bounds, every ray of the scene) against the ideal, ray by ray: the
    faces by (exact distance, face index) ascending.  Returns (rays with two or more crossings, rays with two faces at exactly
    the same distance)"""
    s, ideal, exact = lattice_lists(name)
    bad = np.flatnonzero(res.count != ideal.count)
    assert len(bad) == 0, f"{what}: count differs from the ideal on {len(bad)} rays, the first: o {s['o'][bad[0]]} d {s['d'][bad[0]]}: {res.count[bad[0]]} != {ideal.count[bad[0]]}"
    lists = ties = 0
    for i in range(len(ideal.count)):
        got = res.faces[rows_of(res, i)]
        faces, ts = ideal.sets[i], exact[i]
        order = sorted(range(len(faces)), key=lambda k: (ts[k], int(faces[k])))
        assert np.array_equal(got, faces[order]), f"{what}: ray {i} (o {s['o'][i]} d {s['d'][i]}) lists {got}, the ideal order is {faces[order]}"
        lists += len(faces) >= 2
        ties += any(ts[a] == ts[b] for a, b in zip(order, order[1:]))
    return lists, ties
