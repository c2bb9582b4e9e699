"""Shared by tests/test_boxes_cpu.py and tests/test_gpu_boxes.py (not a test module): the meshes of the box queries -- those of
tests/nearest_cases.py --, their boxes, the comparison of two boxes_sim.Result, an exact integer reference on snapped inputs
and the reference of surface_voxels.

The exact reference is no separating-axis test and shares nothing with csrc/tr_boxes.h: a closed triangle and a closed box
share a point iff a vertex of the triangle lies in the box, or an edge of the triangle meets the box (clipped against the
three slabs in fractions.Fraction), or one of the twelve edges of the box meets the triangle (the crossing with the
triangle's plane, then three edge functions, in Python integers).  Proof that the three cases are complete: the common part
is a convex polygon in the triangle's plane; take one of its corners.  It is a vertex of the triangle, or lies on an edge of
the triangle (and in the box), or on two face planes of the box, that is on an edge of the box (and in the triangle)."""
from fractions import Fraction

import numpy as np

import nearest_cases as NC

CASES = NC.HIERARCHICAL                        # cube, icosphere, soup, deep
FLT_MAX = np.float32(np.finfo(np.float32).max)
HALVES = (1 / 32, 1 / 8, 1 / 2)


def extent(v):
    """the longest side of the box of the finite vertices"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    return float((v.max(0) - v.min(0)).max()) if len(v) else 1.0


def _hash01(n, seed):
    k = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(2654435761) % np.uint64(1 << 32)
    return k.astype(np.float64) / float(1 << 32)


def hashed_boxes(p, ext, seed=0):
    """(lo, hi) float32 [n, 3] around the points p: a half size per box and axis in [0, ext / 4), with flat boxes (one axis of
    zero size), lines (two) and points (three) sprinkled in"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n = len(p)
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.stack([_hash01(n, seed + 7919 * a) for a in range(3)], 1) * 0.25 * ext
        h[3::7, 0] = 0.0
        h[5::11, :2] = 0.0
        h[6::13, :] = 0.0
        h = h.astype(np.float32)
        return (p - h).astype(np.float32), (p + h).astype(np.float32)


def box_sets(v, p):
    """[(label, lo, hi)]: the points themselves, cubes of three half sizes around them, hashed boxes, and one box that holds
    the whole mesh (for every point)"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    ext = extent(v)
    out = [("points", p.copy(), p.copy())]
    for fr in HALVES:
        h = np.float32(fr * ext)
        out.append((f"half size {fr:g} of the extent", (p - h).astype(np.float32), (p + h).astype(np.float32)))
    out.append(("hashed",) + hashed_boxes(p, ext))
    fin = np.asarray(v, np.float32)[np.isfinite(v).all(1)]
    out.append(("the whole mesh", np.tile(fin.min(0), (len(p), 1)), np.tile(fin.max(0), (len(p), 1))))
    return out


def assert_same(got, want, what):
    """two boxes_sim.Result (or tuples laid out like one; None entries of `got` are skipped), element for element"""
    for name, g, w in zip(("any", "count", "offsets", "faces", "inside"), got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, expected {w.shape}"
        assert g.dtype == w.dtype, f"{what}: {name} has type {g.dtype}, expected {w.dtype}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {name} differs at {bad[:8]} ({len(bad)} of {len(g)}): {g[bad[:4]]} != {w[bad[:4]]}")


def check_identities(res, what):
    """what holds for any Result whatever the mesh: any == (count > 0), count == diff(offsets), lists strictly ascending"""
    assert np.array_equal(res.any, res.count > 0), what
    assert np.array_equal(res.count, np.diff(res.offsets)), what
    assert len(res.faces) == res.offsets[-1] == len(res.inside) and res.offsets[0] == 0, what
    if len(res.faces) > 1:
        inner = np.ones(len(res.faces) - 1, bool)
        starts = res.offsets[1:-1]
        inner[starts[(starts > 0) & (starts < len(res.faces))] - 1] = False        # (a pair that straddles two boxes' lists)
        assert (np.diff(res.faces)[inner] > 0).all(), f"{what}: a list is not strictly ascending"


def listed(res, n, nf):
    """[n, nf] bool: face f is in the list of box i"""
    got = np.zeros((n, nf), bool)
    got[np.repeat(np.arange(n), res.count), res.faces] = True
    return got


# ---- hostile boxes ------------------------------------------------------------------------------------------------------
def hostile_boxes(ordinary_lo, ordinary_hi):
    """(lo, hi, valid, whole): the first rows of ordinary boxes replaced by hostile ones.  valid [n]: finite and lo <= hi;
    whole [n]: the box is [-FLT_MAX, FLT_MAX]^3 or holds the unit-sized meshes anyway (meets every active face)"""
    lo, hi = np.array(ordinary_lo, np.float32), np.array(ordinary_hi, np.float32)
    whole = np.zeros(len(lo), bool)
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for corner in (lo, hi):
            for axis in range(3):
                corner[k, axis] = bad
                k += 1
    for axis in range(3):                                  # lo > hi on one axis, by one float32 step and by a lot
        lo[k, axis] = np.nextafter(hi[k, axis], np.float32(np.inf)); k += 1
        lo[k, axis] = hi[k, axis] + np.float32(2.0); k += 1
    lo[k] = -FLT_MAX; hi[k] = FLT_MAX; whole[k] = True; k += 1
    lo[k] = [-FLT_MAX, -3e38, -2.0 ** 100]; hi[k] = [3e38, FLT_MAX, 2.0 ** 100]; whole[k] = True; k += 1
    lo[k] = [-FLT_MAX, -4, -4]; hi[k] = [FLT_MAX, 4, 4]; whole[k] = True; k += 1          # a slab
    lo[k] = FLT_MAX; hi[k] = FLT_MAX; k += 1                                              # a point at the end of the range
    lo[k] = [-FLT_MAX, 0, 0]; hi[k] = [FLT_MAX, 0, 0]; k += 1                              # a line through everything
    lo[k] = [0, 0, 0]; hi[k] = [1e-45, 1e-45, 1e-45]; k += 1                               # a denormal box
    lo[k] = [-0.0, -0.0, -0.0]; hi[k] = [0.0, 0.0, 0.0]; k += 1                            # -0 <= +0: a valid point
    assert k <= len(lo)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(lo).all(1) & np.isfinite(hi).all(1) & (lo <= hi).all(1)
    return lo, hi, valid, whole


# ---- the exact reference (snapped inputs) -------------------------------------------------------------------------------
GRID = 1024                                     # coordinates are k / GRID, |k| <= 4 * GRID


def snapped(x):
    """the integers k of coordinates k * 2^-10, asserting that the input is on the grid and |k| <= 2^12"""
    x = np.asarray(x, np.float64)
    k = x * GRID
    assert np.array_equal(k, np.round(k)) and (np.abs(k) <= 4 * GRID).all(), "input is not snapped to k * 2^-10, |k| <= 2^12"
    return k.astype(np.int64)


def snap(x):
    """float32 coordinates rounded to the grid (|x| <= 4)"""
    return (np.round(np.asarray(x, np.float64) * GRID) / GRID).astype(np.float32)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _segment_meets_box(p, q, lo, hi):
    """the segment p .. q clipped against the three slabs (Liang-Barsky in exact fractions)"""
    t0, t1 = Fraction(0), Fraction(1)
    for k in range(3):
        d = q[k] - p[k]
        if d == 0:
            if p[k] < lo[k] or p[k] > hi[k]:
                return False
            continue
        ta, tb = Fraction(lo[k] - p[k], d), Fraction(hi[k] - p[k], d)
        if ta > tb:
            ta, tb = tb, ta
        t0, t1 = max(t0, ta), min(t1, tb)
        if t0 > t1:
            return False
    return True


def _in_triangle_scaled(x, s, tri, n):
    """the point x / s (s != 0, in the triangle's plane) lies in the closed triangle: three edge functions, in integers"""
    sign = 1 if s > 0 else -1
    for v, w in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
        rel = (x[0] - v[0] * s, x[1] - v[1] * s, x[2] - v[2] * s)
        if _dot(_cross(_sub(w, v), rel), n) * sign < 0:
            return False
    return True


def _segment_meets_triangle(p, q, tri, n):
    """a segment (an edge of the box) against a triangle with the normal n != 0.  A segment in the triangle's plane counts only
    through its end points: where it crosses an edge of the triangle, that edge meets the box, which is its own case"""
    dp, dq = _dot(n, _sub(p, tri[0])), _dot(n, _sub(q, tri[0]))
    if (dp > 0 and dq > 0) or (dp < 0 and dq < 0):
        return False
    if dp == 0 and dq == 0:
        return _in_triangle_scaled(p, 1, tri, n) or _in_triangle_scaled(q, 1, tri, n)
    s = dp - dq                                      # the crossing is p + (dp / s) (q - p) = (p s + dp (q - p)) / s
    x = tuple(p[k] * s + dp * (q[k] - p[k]) for k in range(3))
    return _in_triangle_scaled(x, s, tri, n)


def exact_meets(lo, hi, tri):
    """closed box [lo, hi] (lo <= hi) against the closed triangle tri = (a, b, c); everything tuples of Python integers"""
    if any(all(lo[k] <= v[k] <= hi[k] for k in range(3)) for v in tri):
        return True
    if any(_segment_meets_box(tri[j], tri[(j + 1) % 3], lo, hi) for j in range(3)):
        return True
    n = _cross(_sub(tri[1], tri[0]), _sub(tri[2], tri[0]))
    if n == (0, 0, 0):
        return False                                 # a segment or a point: its edges were all of it
    for axis in range(3):                            # the four edges of the box along `axis`
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for cu in (lo[u], hi[u]):
            for cw in (lo[w], hi[w]):
                p, q = [0, 0, 0], [0, 0, 0]
                p[axis], q[axis], p[u], q[u], p[w], q[w] = lo[axis], hi[axis], cu, cu, cw, cw
                if _segment_meets_triangle(tuple(p), tuple(q), tri, n):
                    return True
    return False


def exact_table(v, f, lo, hi, shrink=0):
    """[n, F] bool by exact_meets on snapped inputs (asserted); shrink: grid steps taken off every side of every box -- a box
    that this empties meets nothing"""
    V, LO, HI = snapped(v), snapped(lo) + shrink, snapped(hi) - shrink
    tris = [tuple(tuple(int(c) for c in V[i]) for i in t) for t in np.asarray(f)]
    out = np.zeros((len(LO), len(tris)), bool)
    for i in range(len(LO)):
        l, h = tuple(int(c) for c in LO[i]), tuple(int(c) for c in HI[i])
        if any(l[k] > h[k] for k in range(3)):
            continue
        for j, t in enumerate(tris):
            out[i, j] = exact_meets(l, h, t)
    return out


def lattice_boxes(v, n, seed, extra=(-1.5, 1.5)):
    """(lo, hi) [n, 3] float32 with every bound taken from the lattice of the vertices' own coordinates (plus `extra`): boxes
    whose faces pass through vertices.  Every seventh box is flat on one axis, every eleventh a point at a vertex."""
    v = np.asarray(v, np.float32)
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for a in range(3):
        values = np.unique(np.concatenate([v[:, a], np.asarray(extra, np.float32)]))
        i = (_hash01(n, seed + 31 * a) * len(values)).astype(int)
        j = (_hash01(n, seed + 31 * a + 17) * len(values)).astype(int)
        lo[:, a], hi[:, a] = values[np.minimum(i, j)], values[np.maximum(i, j)]
    flat = np.arange(n) % 7 == 3
    hi[flat, 0] = lo[flat, 0]
    point = np.arange(n) % 11 == 5
    at = v[(_hash01(n, seed + 5) * len(v)).astype(int)]
    lo[point], hi[point] = at[point], at[point]
    return lo, hi


def snapped_meshes():
    """{name: (v, f)} on the grid: the cube, the icosphere rounded to it, and the soup's six zero-area triangles (segments and
    points) beside two proper ones"""
    cv, cf, _ = NC.cube()
    iv, i_f, _ = NC.icosphere()
    sv, sf, _ = NC.soup_with_degenerates()
    dv = sv[sf[-6:].reshape(-1)]
    dv = np.concatenate([dv, np.float32([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0.25], [-0.5, -0.5, -0.5], [0.5, -0.5, 0.5], [0.25, 0.75, 0]])])
    return {"cube": (cv, cf), "icosphere": (snap(iv), i_f), "degenerate": (snap(dv), np.arange(len(dv), dtype=np.int32).reshape(-1, 3))}


SNAPPED_BOXES = {"cube": 260, "icosphere": 90, "degenerate": 260}


def check_snapped(run, what):
    """run(v, f, lo, hi) -> Result; on every snapped mesh the sets must EQUAL the exact reference, pairs that only touch
    included.  Returns {mesh: (pairs, met, touching)}"""
    stats = {}
    for k, (name, (v, f)) in enumerate(snapped_meshes().items()):
        lo, hi = lattice_boxes(v, SNAPPED_BOXES[name], seed=100 * k)
        want = exact_table(v, f, lo, hi)
        shrunk = exact_table(v, f, lo, hi, shrink=1)
        assert not (shrunk & ~want).any()
        touching = want & ~shrunk
        res = run(v, f, lo, hi)
        got = listed(res, len(lo), len(f))
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{what}, {name}: {len(bad)} of {want.size} pairs differ from the exact reference, the first (box, face) {bad[:4].tolist()}"
        assert np.array_equal(res.count, want.sum(1)) and np.array_equal(res.any, want.any(1)), f"{what}, {name}"
        assert touching.sum() > 0 and got[touching].all(), f"{what}, {name}: pairs that only touch"
        # inside: all three vertices in the box, in integers
        V, LO, HI = snapped(v), snapped(lo), snapped(hi)
        tv = V[np.asarray(f)]                                                  # [F, 3, 3]
        inside = ((tv[None] >= LO[:, None, None, :]) & (tv[None] <= HI[:, None, None, :])).all(axis=(2, 3))
        assert np.array_equal(res.inside, inside[got]), f"{what}, {name}: inside"
        stats[name] = (int(want.size), int(want.sum()), int(touching.sum()))
    return stats


# ---- surface_voxels -------------------------------------------------------------------------------------------------------
def voxel_planes(origin, pitch, first, count):
    """[count] float32: the planes first .. first + count - 1 of one axis, float32(origin + i * pitch) evaluated in float64"""
    return np.float32(np.float64(origin) + np.arange(first, first + count, dtype=np.float64) * np.float64(pitch))


def voxel_cells(v, f, pitch, origin, brute_any, margin=2):
    """int64 [m, 3]: every integer cell whose closed box meets the surface, lexicographic, by `brute_any(lo, hi) -> bool [n]` over
    a grid that overshoots the mesh's box by `margin` cells on every side (all of them must come out empty)"""
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    origin = lo if origin is None else np.asarray(origin, np.float64)
    first = np.floor((lo - origin) / pitch).astype(np.int64) - margin
    last = np.floor((hi - origin) / pitch).astype(np.int64) + margin
    planes = [voxel_planes(origin[a], pitch, first[a], last[a] - first[a] + 2) for a in range(3)]
    idx = np.stack(np.meshgrid(*[np.arange(len(p) - 1) for p in planes], indexing="ij"), -1).reshape(-1, 3)
    blo = np.stack([planes[a][idx[:, a]] for a in range(3)], 1)
    bhi = np.stack([planes[a][idx[:, a] + 1] for a in range(3)], 1)
    met = np.asarray(brute_any(blo, bhi), bool)
    cells = idx + first
    edge = ((idx == 0) | (idx == np.array([len(p) - 2 for p in planes]))).any(1)
    assert not met[edge].any(), "the reference grid does not overshoot the surface"
    return cells[met].astype(np.int64)
