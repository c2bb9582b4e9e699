"""Shared by tests/test_planes_cpu.py and tests/test_gpu_planes.py (not a test module): the meshes of the plane queries, their
planes, the comparison of two planes_sim.Result, an exact integer reference on snapped inputs, the closed-loop identity, the known
answers on the 4-cell cube and the keys of the ordering network.

The exact reference shares nothing with csrc/tr_planes.h: on inputs k * 2^-10, |k| <= 2^12, with small integer normals the signed
value of a vertex is the integer sum n . (v - o) in grid units (|d| <= 2^13, |n| <= 2^3: below 2^18, exact in float64 as well), and
the classification is restated on Python / numpy integers (exact_tables)."""
import numpy as np

import hostile_meshes as M
import nearest_cases as NC
import workloads as W

FLT_MAX = np.float32(np.finfo(np.float32).max)
FRONTIERS = (1, 2, 63, 64, 0)                  # frontier_entries of every walk comparison; 0 = the whole capacity
BATCHES = (1, 63, 64, 65, 257)
GRID = 1024                                    # snapped coordinates are k / GRID, |k| <= 4 * GRID


# ---- meshes -------------------------------------------------------------------------------------------------------------
def _patch(p0, du, dv, k, flip):
    """(k + 1)^2 vertices p0 + i/k du + j/k dv and 2 k^2 triangles wound counter-clockwise seen from du x dv; the diagonal of a
    cell runs along du + dv, with `flip` along du - dv"""
    iu, iv = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij")
    v = np.asarray(p0, np.float64) + (iu / k)[..., None] * np.asarray(du, np.float64) + (iv / k)[..., None] * np.asarray(dv, np.float64)
    idx = iu * (k + 1) + iv
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    first, second = ((a, b, d), (b, c, d)) if flip else ((a, b, c), (a, c, d))
    f = np.concatenate([np.stack(first, -1).reshape(-1, 3), np.stack(second, -1).reshape(-1, 3)], 0)
    return v.reshape(-1, 3), f


def unit_cube(k):
    """the unit cube [0, 1]^3, outward-wound, k x k cells per side, 12 k^2 triangles; every side has its own vertices (the
    coordinates of a shared edge are the same bits).  The cell diagonals of the three sides through the corner (0, 0, 0) run
    along (1, 1) in the side's two coordinates, those of the three sides through (1, 1, 1) along (1, -1): the triangulation on
    which the known answers below hold (the face counts of a diagonal plane depend on it, the areas do not)."""
    ex, ey, ez = np.eye(3)
    o = np.zeros(3)
    sides = ((o, ey, ex, 0), (ez, ex, ey, 1), (o, ez, ey, 0), (ex, ey, ez, 1), (o, ex, ez, 0), (ey, ez, ex, 1))
    vs, fs, base = [], [], 0
    for p0, du, dv, flip in sides:
        v, f = _patch(p0, du, dv, k, flip)
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def few_triangles(nt):
    """0 .. 3 triangles: no hierarchy below two"""
    v, f = W.two_triangles()
    v = np.concatenate([v, np.float32([[0.25, -0.75, -0.5], [0.25, 0.75, -0.5], [0.25, 0.0, 0.75]])])
    f = np.concatenate([f, np.int32([[6, 7, 8]])])
    return np.ascontiguousarray(v[:3 * nt]), np.ascontiguousarray(f[:nt])


def hostile_mesh():
    """a mesh of tests/hostile_meshes.py with NaN / +-Inf vertices and triangles displaced to +-FLT_MAX"""
    c = M.case("faraway_nonfinite", 0)
    return np.array(c.v), np.array(c.f)


def comb(n=6000):
    """n thin triangles side by side along x, every one of them from z = -1 up to z = 1 and alternately wound: the plane z = 0
    cuts them all -- more rows for one plane than the ordering pass holds in its tile"""
    x = (np.arange(n, dtype=np.float64) / n).astype(np.float32)
    w = np.float32(0.5 / n)
    a = np.stack([x, np.zeros(n, np.float32), np.full(n, -1, np.float32)], 1)
    b = np.stack([x + w, np.full(n, 0.25, np.float32), np.full(n, 1, np.float32)], 1)
    c = np.stack([x, np.ones(n, np.float32), np.full(n, -1, np.float32) + (np.arange(n) % 5).astype(np.float32) * np.float32(0.125)], 1)
    v = np.stack([a, b, c], 1).reshape(-1, 3)
    f = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    f[1::2] = f[1::2, ::-1]
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f)


COMB_PLANES = (np.float32([[0, 0, 0], [0.5, 0.5, 0.5], [0.25, 0, -0.5], [0, 0, -1], [0, 0, 1]]),
               np.float32([[0, 0, 1], [0.125, -0.25, 1], [1, 0, 0.001], [0, 0, 1], [0, 0, -2]]))


MESHES = {
    "0 triangles": lambda: few_triangles(0), "1 triangle": lambda: few_triangles(1), "2 triangles": lambda: few_triangles(2),
    "3 triangles": lambda: few_triangles(3),
    "icosphere80": lambda: W.icosphere(1), "icosphere1280": lambda: W.icosphere(3),
    "cube4": lambda: unit_cube(4), "cube16": lambda: unit_cube(16),
    "hostile": hostile_mesh,
}
CLOSED = ("icosphere80", "icosphere320", "icosphere1280", "cube4", "cube16")      # closed and consistently wound
CLOSED_MESHES = dict({k: MESHES[k] for k in CLOSED if k in MESHES}, icosphere320=lambda: W.icosphere(2))


def mesh(name):
    v, f = (CLOSED_MESHES.get(name) or MESHES[name])()
    return np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)


def finite_box(v):
    v = np.asarray(v, np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1) & (np.abs(v) < 1e6).all(1)]
    if len(v) == 0:
        return np.full(3, -1.0), np.full(3, 1.0)
    return v.min(0), v.max(0)


# ---- planes -------------------------------------------------------------------------------------------------------------
INTEGER_NORMALS = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [1, -1, 2], [-2, 1, 1]])


def hashed_planes(v, n, seed):
    """(origins, normals) float32 [n, 3]: origins hashed over the mesh's box grown by a quarter, normals hashed in [-1, 1]^3;
    every fifth plane has an axis normal and every seventh passes through a vertex"""
    lo, hi = finite_box(v)
    pad = 0.25 * (hi - lo).max()
    o = NC.hash_points(n, seed, lo - pad, hi + pad)
    nr = NC.hash_points(n, seed + 1000, [-1.0] * 3, [1.0] * 3)
    axis = np.arange(n) % 5 == 2
    nr[axis] = np.eye(3, dtype=np.float32)[np.arange(n)[axis] % 3] * np.float32(-1.5)
    fin = np.asarray(v, np.float32).reshape(-1, 3)
    fin = fin[np.isfinite(fin).all(1)]
    if len(fin):
        at = np.arange(n) % 7 == 3
        o[at] = fin[(np.arange(n)[at] * 31 + seed) % len(fin)]
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(nr, np.float32)


def vertex_planes(v, every=7):
    """planes through every `every`-th vertex with axis and integer normals"""
    at = np.asarray(v, np.float32)[::every]
    o = np.repeat(at, len(INTEGER_NORMALS), 0)
    nr = np.tile(INTEGER_NORMALS, (len(at), 1))
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(nr, np.float32)


def lattice_planes():
    """1 512 planes on the cube's lattice: origins in {0, 1/4, 1/2, 1} x {0, 1/2} x {0, 1/4, 3/4}, normals in {-1, 0, 1, 2}^3
    without the zero normal -- through vertices, along edges, coplanar with faces"""
    os_ = np.stack(np.meshgrid([0, 0.25, 0.5, 1], [0, 0.5], [0, 0.25, 0.75], indexing="ij"), -1).reshape(-1, 3)
    ns = np.stack(np.meshgrid(*[[-1, 0, 1, 2]] * 3, indexing="ij"), -1).reshape(-1, 3)
    ns = ns[(ns != 0).any(1)]
    o, nr = np.repeat(os_, len(ns), 0), np.tile(ns, (len(os_), 1))
    assert len(o) == 1512
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(nr, np.float32)


def hostile_planes(origins, normals):
    """(origins, normals, valid, empty): the first rows of ordinary planes replaced by hostile ones.  valid [n]: finite with a
    non-zero normal; empty [n]: the plane must yield nothing on a mesh of unit size (invalid, or valid and far away)"""
    o, nr = np.array(origins, np.float32), np.array(normals, np.float32)
    empty = np.zeros(len(o), bool)
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for part in (o, nr):
            for axis in range(3):
                part[k, axis] = bad
                k += 1
    nr[k] = 0.0; k += 1
    nr[k] = [0.0, -0.0, 0.0]; k += 1
    first_far = k
    for far in (FLT_MAX, -FLT_MAX, np.float32(2.0 ** 60)):
        o[k] = far; nr[k] = [1, 1, 1]; k += 1
        o[k] = [far, 0, 0]; nr[k] = [1, 0, 0]; k += 1
        o[k] = [far, 0, 0]; nr[k] = [FLT_MAX, 0, 0]; k += 1
    empty[first_far:k] = True
    o[k] = 0.0; nr[k] = [1e-45, 0, 0]; k += 1                      # denormal normals: valid planes through the origin
    o[k] = 0.0; nr[k] = [1e-40, -1e-42, 1e-45]; k += 1
    o[k] = [0.125, 0, 0]; nr[k] = [0, 1e-45, 0]; k += 1
    o[k] = 0.0; nr[k] = [FLT_MAX, FLT_MAX, -FLT_MAX]; k += 1       # the largest normal: |s| stays finite
    assert k <= len(o)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(o).all(1) & np.isfinite(nr).all(1) & (nr != 0).any(1)
    empty |= ~valid
    return o, nr, valid, empty


# ---- comparison -----------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same(got, want, what):
    """two planes_sim.Result (or tuples laid out like one; None entries of `got` are skipped), element for element; segments as
    bits"""
    for name, g, w in zip(("any", "count", "offsets", "faces", "segments"), got, want):
        if g is None:
            continue
        assert w is not None, f"{what}: {name} given but not expected"
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, expected {w.shape}"
        assert g.dtype == w.dtype, f"{what}: {name} has type {g.dtype}, expected {w.dtype}"
        if name == "segments":
            g, w = bits(g), bits(w)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {name} differs at {bad[:4].tolist()} ({len(bad)} of {g.size}): "
                                 f"{g[tuple(bad[0])]} != {w[tuple(bad[0])]}")


def check_identities(res, what):
    """what holds for any Result whatever the mesh: any == (count > 0), count == diff(offsets), lists strictly ascending"""
    assert np.array_equal(res.any, res.count > 0), what
    assert np.array_equal(res.count, np.diff(res.offsets)), what
    assert len(res.faces) == res.offsets[-1] and res.offsets[0] == 0, what
    assert res.segments is None or res.segments.shape == (len(res.faces), 2, 3), what
    if len(res.faces) > 1:
        inner = np.ones(len(res.faces) - 1, bool)
        starts = res.offsets[1:-1]
        inner[starts[(starts > 0) & (starts < len(res.faces))] - 1] = False        # (a pair that straddles two planes' lists)
        assert (np.diff(res.faces)[inner] > 0).all(), f"{what}: a list is not strictly ascending"


def listed(res, n, nf):
    """[n, nf] bool: face f is in the list of plane i"""
    got = np.zeros((n, nf), bool)
    got[np.repeat(np.arange(n), res.count), res.faces] = True
    return got


# ---- the exact reference (snapped inputs) -------------------------------------------------------------------------------
def snapped(x):
    """the integers k of coordinates k * 2^-10, asserting that the input is on the grid and |k| <= 2^12"""
    x = np.asarray(x, np.float64)
    k = x * GRID
    assert np.array_equal(k, np.round(k)) and (np.abs(k) <= 4 * GRID).all(), "input is not snapped to k * 2^-10, |k| <= 2^12"
    return k.astype(np.int64)


def snap(x):
    return (np.round(np.asarray(x, np.float64) * GRID) / GRID).astype(np.float32)


def exact_tables(v, f, origins, normals):
    """(meets, cut) [n, F] bool in integers: s = n . (v - o) in grid units, pos / neg / zero counted per face"""
    V, O = snapped(v), snapped(origins)
    N = np.asarray(normals, np.float64)
    assert np.array_equal(N, np.round(N)) and (np.abs(N) <= 8).all() and (N != 0).any(1).all(), "normals must be small non-zero integers"
    N = N.astype(np.int64)
    tv = V[np.asarray(f)]                                                        # [F, 3, 3]
    s = ((tv[None] - O[:, None, None, :]) * N[:, None, None, :]).sum(-1)         # [n, F, 3] int64, exact
    pos, neg, zero = (s > 0).sum(-1), (s < 0).sum(-1), (s == 0).sum(-1)
    meets = ~((pos == 3) | (neg == 3))
    cut = (pos >= 1) & ((neg >= 1) | (zero == 2))
    return meets, cut


def check_exact(run, v, f, origins, normals, what):
    """run(origins, normals, cut) -> Result; the lists must EQUAL the integer reference for both predicates.  Returns (pairs,
    met, cut, met with a vertex in the plane)"""
    meets, cut = exact_tables(v, f, origins, normals)
    assert not (cut & ~meets).any()
    for want, c in ((meets, False), (cut, True)):
        res = run(origins, normals, c)
        got = listed(res, len(origins), len(f))
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{what}, cut={c}: {len(bad)} of {want.size} pairs differ from the exact reference, the first (plane, face) {bad[:4].tolist()}"
        assert np.array_equal(res.count, want.sum(1)) and np.array_equal(res.any, want.any(1)), f"{what}, cut={c}"
    V, O, N = snapped(v), snapped(origins), np.asarray(normals, np.int64)
    s = ((V[np.asarray(f)][None] - O[:, None, None, :]) * N[:, None, None, :]).sum(-1)
    return int(meets.size), int(meets.sum()), int(cut.sum()), int((meets & (s == 0).any(-1)).sum())


# ---- closed loops ---------------------------------------------------------------------------------------------------------
def loops_close(res, what):
    """for every plane the multiset of p0 (three float32 as bits) must EQUAL the multiset of p1; returns the number of rows"""
    seg = bits(res.segments).reshape(-1, 2, 3).astype(np.int64)
    plane = np.repeat(np.arange(len(res.count), dtype=np.int64), res.count)
    ends = []
    for e in (0, 1):
        rows = np.concatenate([plane[:, None], seg[:, e, :]], 1)
        ends.append(rows[np.lexsort(rows.T[::-1])])
    if not np.array_equal(ends[0], ends[1]):
        bad = np.flatnonzero((ends[0] != ends[1]).any(1))
        raise AssertionError(f"{what}: the ends of the segments do not pair up: {len(bad)} of {len(plane)} rows, first in plane {ends[0][bad[0], 0]}")
    return len(plane)


# ---- known answers on the 4-cell cube ------------------------------------------------------------------------------------
# (origin, normal, faces met, rows, A = 1/2 sum n . (p0 x p1) in float64 = -|n| * area of the section; None: no rows)
KNOWN = [
    ((0, 0, .375), (0, 0, 1), 32, 32, -1.0),
    ((0, 0, .5), (0, 0, 1), 64, 16, -1.0),
    ((0, 0, 0), (0, 0, 1), 64, 16, -1.0),
    ((0, 0, 1), (0, 0, 1), 64, 0, None),
    ((.5, .5, .5), (1, 1, 0), 66, 20, -2.0),
    ((.5, .5, .5), (1, 1, 1), 60, 18, -2.25),
    ((0, 0, 0), (1, 1, 0), 19, 8, 0.0),
]


def check_known(run, what):
    """run(origins, normals, cut) -> Result on unit_cube(4)"""
    o, nr = np.float32([k[0] for k in KNOWN]), np.float32([k[1] for k in KNOWN])
    met, cut = run(o, nr, False), run(o, nr, True)
    for i, (_, _, want_met, want_rows, want_a) in enumerate(KNOWN):
        assert met.count[i] == want_met, f"{what}: plane {KNOWN[i][:2]} meets {met.count[i]} faces, expected {want_met}"
        assert cut.count[i] == want_rows, f"{what}: plane {KNOWN[i][:2]} has {cut.count[i]} rows, expected {want_rows}"
        seg = cut.segments[cut.offsets[i]:cut.offsets[i + 1]].astype(np.float64)
        a = 0.5 * float((np.cross(seg[:, 0], seg[:, 1]) @ nr[i].astype(np.float64)).sum())
        assert a == (0.0 if want_a is None else want_a), f"{what}: plane {KNOWN[i][:2]} has A = {a!r}, expected {want_a}"
    # the last plane touches the cube along one edge: that edge once per adjacent face, in opposite directions
    seg = bits(cut.segments[cut.offsets[6]:cut.offsets[7]]).reshape(-1, 2, 3)
    there = sorted(map(bytes, seg.reshape(len(seg), -1)))
    back = sorted(map(bytes, seg[:, ::-1, :].reshape(len(seg), -1)))
    assert there == back and len(set(there)) == 8
    loops_close(cut, what)


# ---- the ordering network -----------------------------------------------------------------------------------------------
ORDER_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 1000, 4097)
INT32_MIN, INT32_MAX = np.int32(-2 ** 31), np.int32(2 ** 31 - 1)


def order_keys(m, seed):
    """m int32 keys: hashed with duplicates, both ends of the range, and already-sorted runs (ascending and descending)"""
    k = ((np.arange(m, dtype=np.uint64) + np.uint64(seed * 7919 + 1)) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32).view(np.int32).copy()
    k[::3] >>= 20                                      # duplicates
    if m >= 8:
        k[1], k[m // 2], k[m - 2], k[m - 1] = INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN
    if m >= 64:
        k[8:40] = np.sort(k[8:40])
        k[40:60] = np.sort(k[40:60])[::-1]
    if seed % 3 == 1:
        k = np.sort(k)                                 # a whole segment that is sorted already
    if seed % 3 == 2:
        k = np.sort(k)[::-1].copy()
    return k


def order_case(guard=5):
    """(keys with `guard` words between the segments, count, offsets): one segment per length of ORDER_LENGTHS, twice"""
    parts, count, offsets, at = [], [], [], guard
    for seed, m in enumerate(ORDER_LENGTHS + ORDER_LENGTHS[::-1]):
        offsets.append(at)
        count.append(m)
        parts.append(order_keys(m, seed))
        at += m + guard
    return parts, np.int32(count), np.int64(offsets), at
