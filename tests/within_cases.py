"""Shared by tests/test_within_cpu.py and tests/test_gpu_within.py (not a test module): the meshes and points of the radius
queries -- those of tests/nearest_cases.py --, their radii, the bit-for-bit comparison of two within_sim.Result, an exact
reference in fractions.Fraction for the cube lattice, and the tolerance check against nearest_cases.numpy_distances.

The exact reference shares no formulation with csrc/tr_nearest.h: the in-plane candidate comes from the 2x2 Gram system of
(b - a, c - a) and its barycentric coordinates, the edges are clamped segments, nothing is clamped into a coordinate range
and every operation is exact rational arithmetic."""
from fractions import Fraction

import numpy as np

import nearest_cases as NC

CASES = NC.HIERARCHICAL                        # cube, icosphere, soup, deep
FRACTIONS = (0.0, 1 / 32, 1 / 8, 1 / 4, 1 / 2)
TOLERANCE_FRACTIONS = (1 / 32, 1 / 8, 1 / 4, 1 / 2)


def extent(v):
    """the longest side of the box of the finite vertices"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    return float((v.max(0) - v.min(0)).max()) if len(v) else 1.0


def hashed_radii(n, ext, seed=0):
    """[n] float32: a radius per point in [0, ext / 2), with exact zeros and +Inf sprinkled in"""
    k = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(2654435761) % np.uint64(1 << 32)
    with np.errstate(over="ignore"):              # (an extent near the end of the float range: +Inf radii)
        r = (k.astype(np.float64) / float(1 << 32) * 0.5 * ext).astype(np.float32)
    r[3::7] = 0.0
    r[5::11] = np.inf
    return r


def radii(v, n):
    """[(label, radius)]: the fractions of the extent as float32 scalars, +Inf, and one per-point array"""
    ext = extent(v)
    out = [(f"{fr:g} of the extent", np.float32(fr * ext)) for fr in FRACTIONS]
    out.append(("+Inf", np.float32(np.inf)))
    out.append(("per point", hashed_radii(n, ext)))
    return out


def assert_same(got, want, what, nearest=True):
    """two within_sim.Result (or tuples laid out like one; None entries of `got` are skipped), bit for bit"""
    names = ("any", "count", "offsets", "faces", "distance", "closest")
    for name, g, w in zip(names, got[:6], want[:6]):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, expected {w.shape}"
        if g.dtype == np.float32:
            g, w = NC.bits(g), NC.bits(w)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
            raise AssertionError(f"{what}: {name} differs at {bad[:8]} ({len(bad)} of {len(g)}): {g[bad[:4]]} != {w[bad[:4]]}")
    if nearest and got[6] is not None:
        NC.assert_same_bits(tuple(got[6][:3]), tuple(want[6][:3]), f"{what}: bounded nearest")


def check_identities(res, what):
    """what holds for any Result whatever the mesh: any == (count > 0) == (bounded nearest found), count == diff(offsets),
    lists strictly ascending"""
    assert np.array_equal(res.any, res.count > 0), what
    assert np.array_equal(res.count, np.diff(res.offsets)), what
    assert len(res.faces) == res.offsets[-1] and res.offsets[0] == 0, what
    if len(res.faces) > 1:
        inner = np.ones(len(res.faces) - 1, bool)
        starts = res.offsets[1:-1]
        inner[starts[(starts > 0) & (starts < len(res.faces))] - 1] = False        # (a pair that straddles two points' lists)
        assert (np.diff(res.faces)[inner] > 0).all(), f"{what}: a list is not strictly ascending"
    assert np.array_equal(res.any, res.nearest[2] >= 0), f"{what}: any against the bounded nearest"


# ---- the exact reference (cube lattice) ---------------------------------------------------------------------------------
def _fr(x):
    return [Fraction(float(c)) for c in x]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _segment_d2(w, e):
    ee = _dot(e, e)
    t = min(max(_dot(w, e) / ee, Fraction(0)), Fraction(1)) if ee > 0 else Fraction(0)
    q = [w[k] - t * e[k] for k in range(3)]
    return _dot(q, q)


def exact_d2(p, a, b, c):
    """the exact squared distance (a Fraction) from point p to triangle (a, b, c), all sequences of three floats"""
    p, a, b, c = _fr(p), _fr(a), _fr(b), _fr(c)
    e1, e2, w = _sub(b, a), _sub(c, a), _sub(p, a)
    g11, g12, g22, r1, r2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(w, e1), _dot(w, e2)
    det = g11 * g22 - g12 * g12
    if det > 0:
        s, t = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
        if s >= 0 and t >= 0 and s + t <= 1:
            q = [w[k] - s * e1[k] - t * e2[k] for k in range(3)]
            return _dot(q, q)
    return min(_segment_d2(w, e1), _segment_d2(_sub(p, b), _sub(c, b)), _segment_d2(_sub(p, c), _sub(a, c)))


def exact_d2_table(v, f, p):
    """[n][F] Fractions"""
    return [[exact_d2(pt, v[t[0]], v[t[1]], v[t[2]]) for t in f] for pt in p]


LATTICE_RADII = (0.0, 0.25, 0.5, 1.0)          # dyadic: with vertices at +-1 and points on a 1/4 grid every d2 is exact


def check_cube_lattice(run, what):
    """run(points, radius) -> Result on the cube; sets and counts against the exact table at the dyadic radii and just below
    them.  Returns the number of (point, face) pairs at distance exactly r, per radius."""
    v, f, p = NC.cube()
    assert set(np.unique(v)) == {-1.0, 1.0} and np.array_equal(p * 4, np.round(p * 4))
    table = exact_d2_table(v, f, p)
    at = []
    for r in LATTICE_RADII:
        below = np.nextafter(np.float32(r), np.float32(0)) if r > 0 else None
        on = np.array([[d == Fraction(r) ** 2 for d in row] for row in table])
        at.append(int(on.sum()))
        for rr in (np.float32(r),) + (() if below is None else (below,)):
            want = np.array([[d <= Fraction(float(rr)) ** 2 for d in row] for row in table])
            res = run(p, rr)
            got = np.zeros_like(want)
            rows = np.repeat(np.arange(len(p)), res.count)
            got[rows, res.faces] = True
            assert np.array_equal(res.count, want.sum(1)), f"{what}: counts at r = {float(rr)!r}"
            assert np.array_equal(got, want), f"{what}: sets at r = {float(rr)!r}"
            assert np.array_equal(res.any, want.any(1)), f"{what}: any at r = {float(rr)!r}"
            if rr == np.float32(r):
                assert got[on].all(), f"{what}: a face at exactly r = {r} is not within"
            else:
                assert not got[on].any(), f"{what}: a face at exactly r = {r} is within nextafter(r, 0)"
    return at


# ---- the independent tolerance check --------------------------------------------------------------------------------------
def check_tolerance(v, f, p, r, res, what):
    """every pair with numpy distance D <= r - tol is listed, none with D >= r + tol is; tol = one float32 spacing of r + two
    float32 spacings of the coordinate scale S + 2^-40 S.  Pairs inside the band are left out and must be at most 0.1 % of
    the pairs within r.  Prints each figure before it asserts."""
    v, f, p = np.asarray(v, np.float32), np.asarray(f, np.int32), np.asarray(p, np.float32)
    S = float(max(np.abs(v[f[NC.active(v, f)].reshape(-1)]).max(), np.abs(p).max()))
    r = float(np.float32(r))
    tol = float(NC.u32(r)) + 2 * float(NC.u32(S)) + 2.0 ** -40 * S
    D = NC.numpy_distances(v, f, p)
    listed = np.zeros(D.shape, bool)
    listed[np.repeat(np.arange(len(p)), res.count), res.faces] = True
    inside, outside = D <= r - tol, D >= r + tol
    band = ~inside & ~outside
    within = int((D <= r).sum())
    print(f"{what}: r = {r:g}, S = {S:g}, tol = {tol:.3g}: {within} pairs within r, {int(band.sum())} in the band, "
          f"{int((inside & ~listed).sum())} missing, {int((outside & listed).sum())} listed beyond")
    assert not (inside & ~listed).any(), f"{what}: {int((inside & ~listed).sum())} pairs well within r are not listed"
    assert not (outside & listed).any(), f"{what}: {int((outside & listed).sum())} pairs well beyond r are listed"
    assert band.sum() <= 0.001 * within, f"{what}: {int(band.sum())} pairs in the band of {within} within r"
    return within, int(band.sum())
