"""Shared by tests/test_tris_cpu.py and tests/test_gpu_tris.py (not a test module): the meshes of the triangle queries -- those
of tests/nearest_cases.py --, their query triangles, the comparison of two tris_sim.Result and an exact integer reference on
snapped inputs.

The exact reference is no separating-axis test and shares nothing with csrc/tr_tris.h: two closed triangles WITH AREA share a
point iff an edge of one meets the other closed triangle.  Proof: the common part is convex; if the triangles are not
coplanar it is a point or a segment on the line where the planes cross, and an end of it lies on the boundary of one of the
triangles, that is on an edge of it (and in the other triangle); if they are coplanar and no edge of one meets an edge of the
other, one of them lies in the other with all its edges, or they are apart.
A segment against a closed triangle (segment_meets_triangle), in Python integers: the signs of the two ends against the
triangle's plane; a segment that crosses the plane meets it at one point x / s, tested with three scaled edge functions; a
segment IN the plane is projected with the triangle onto the coordinate plane where the normal is largest, and meets it iff
an end lies in the triangle or it crosses one of the triangle's edges (2-D orientation tests, collinear overlap included)."""
import functools

import numpy as np

import nearest_cases as NC
from boxes_cases import _cross, _dot, _hash01, _in_triangle_scaled, _sub, extent  # noqa: F401  (extent: for the tests)

CASES = NC.HIERARCHICAL                        # cube, icosphere, soup, deep
FLT_MAX = np.float32(np.finfo(np.float32).max)
SHIFTS = (1 / 32, 1 / 8, 1 / 2)
MAX_OWN = 128                                  # own faces taken as queries, evenly spread


# ---- query triangles ----------------------------------------------------------------------------------------------------
def own_faces(v, f, limit=MAX_OWN):
    """[m, 3, 3] float32: up to `limit` faces of the mesh, evenly spread, as query triangles"""
    f = np.asarray(f)
    pick = np.unique(np.linspace(0, len(f) - 1, min(limit, len(f))).astype(int)) if len(f) else np.zeros(0, int)
    return np.ascontiguousarray(np.asarray(v, np.float32)[f[pick]], np.float32)


def hashed_triangles(n, lo, hi, ext, seed=0):
    """[n, 3, 3] float32: centres hashed in [lo, hi], vertices hashed within size / 2 of them, size = ext / 16, ext / 4 and ext
    in turn"""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float32), (3,)), np.broadcast_to(np.asarray(hi, np.float32), (3,))
    c = NC.hash_points(n, seed, lo, hi).astype(np.float64)
    size = np.array([ext / 16, ext / 4, ext])[np.arange(n) % 3]
    d = np.stack([NC.hash_points(n, seed + 1 + k, [-0.5] * 3, [0.5] * 3) for k in range(3)], 1).astype(np.float64)
    return (c[:, None, :] + d * size[:, None, None]).astype(np.float32)


def larger_than(v):
    """[4, 3, 3] float32: triangles whose boxes hold the whole mesh (every walk visits the whole tree); the first two cut through
    it, the others pass it by"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    c, e = (v.max(0) + v.min(0)) / 2, 3 * max(float((v.max(0) - v.min(0)).max()), 1e-3)
    t = np.array([[[-1, -1, -1], [1, -1, 1], [0, 1, 0]], [[-1, 1, 1], [1, 1, -1], [0, -1, 0.25]],
                  [[-1, -1, 1], [1, -1, 1], [-1, 1, -1]], [[1, -1, -1], [1, 1, -1], [-1, 1, 1]]], np.float64)
    return (c + e * t).astype(np.float32)


def query_sets(v, f):
    """[(label, triangles [n, 3, 3])]: the mesh's own faces, those displaced by three fractions of the extent, hashed triangles
    of three sizes, and triangles larger than the mesh"""
    ext = extent(v)
    own = own_faces(v, f)
    fin = np.asarray(v, np.float32)[np.isfinite(v).all(1)]
    out = [("own faces", own)]
    for fr in SHIFTS:
        d = (np.float64(fr * ext) * np.array([2, -1, 2]) / 3).astype(np.float32)
        out.append((f"own faces displaced by {fr:g} of the extent", (own + d).astype(np.float32)))
    out.append(("hashed", hashed_triangles(150, fin.min(0) - 0.1 * ext, fin.max(0) + 0.1 * ext, ext, seed=5)))
    out.append(("larger than the mesh", larger_than(v)))
    return out


def assert_same(got, want, what):
    """two tris_sim.Result (or tuples laid out like one; None entries of `got` are skipped), element for element"""
    for name, g, w in zip(("any", "count", "offsets", "faces"), got, want):
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
    assert len(res.faces) == res.offsets[-1] and res.offsets[0] == 0, what
    if len(res.faces) > 1:
        inner = np.ones(len(res.faces) - 1, bool)
        starts = res.offsets[1:-1]
        inner[starts[(starts > 0) & (starts < len(res.faces))] - 1] = False        # (a pair that straddles two queries' lists)
        assert (np.diff(res.faces)[inner] > 0).all(), f"{what}: a list is not strictly ascending"


def listed(res, n, nf):
    """[n, nf] bool: face f is in the list of query i"""
    got = np.zeros((n, nf), bool)
    got[np.repeat(np.arange(n), res.count), res.faces] = True
    return got


# ---- hostile queries ------------------------------------------------------------------------------------------------------
def hostile_triangles(ordinary):
    """(triangles, valid, degenerate): the first rows of ordinary triangles replaced by hostile ones.  valid [n]: all nine values
    finite; degenerate [n]: valid but exactly without area (these rows only)"""
    t = np.array(ordinary, np.float32).reshape(-1, 3, 3)
    degenerate = np.zeros(len(t), bool)
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for vertex in range(3):
            for axis in range(3):
                t[k, vertex, axis] = bad
                k += 1
    t[k] = [[0.25, 0.25, 0.25], [-0.5, -0.5, -0.5], [0.75, 0.75, 0.75]]; degenerate[k] = True; k += 1      # collinear
    t[k] = [[-0.75, 0.5, 0.0], [0.25, 0.5, 0.0], [-0.25, 0.5, 0.0]]; degenerate[k] = True; k += 1
    t[k] = [[0.5, -0.25, 0.75], [0.5, -0.25, 0.75], [0.5, 0.5, -0.75]]; degenerate[k] = True; k += 1      # a doubled vertex
    t[k] = [[0.0, 0.0, 0.0]] * 3; degenerate[k] = True; k += 1                                             # a point
    t[k] = [[1e-45, 0, 0], [2e-45, 0, 0], [4e-45, 0, 0]]; degenerate[k] = True; k += 1                     # denormal, collinear
    t[k] = [[-FLT_MAX, -FLT_MAX, -FLT_MAX], [FLT_MAX, -FLT_MAX, FLT_MAX], [0, FLT_MAX, 0]]; k += 1         # through everything near 0
    t[k] = [[-FLT_MAX, -FLT_MAX, 0.25], [FLT_MAX, -FLT_MAX, 0.25], [0, FLT_MAX, 0.25]]; k += 1             # the plane z = 1/4
    t[k] = [[FLT_MAX, FLT_MAX, FLT_MAX], [FLT_MAX, -FLT_MAX, FLT_MAX], [FLT_MAX, 0, -FLT_MAX]]; k += 1     # the plane x = FLT_MAX
    t[k] = [[-FLT_MAX, 0, 0], [FLT_MAX, 1e-30, 0], [0, 0, 1e-38]]; k += 1                                  # a sliver across the range
    t[k] = [[0, 0, 0], [1e-45, 0, 0], [0, 1e-45, 0]]; k += 1                                               # the smallest triangle
    assert k <= len(t)
    return t, np.isfinite(t).all(axis=(1, 2)), degenerate


def hostile_mesh_triangles(c, fa):
    """[triangles] for a hostile mesh: hashed triangles around its points, and triangles larger than its active part"""
    av = c.v[np.unique(fa)] if len(fa) else np.zeros((1, 3), np.float32)
    ext = extent(av) if len(fa) else 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(c.p, np.float64)
        p = p[np.isfinite(p).all(1)][:150]
        near = (p[:, None, :] + (hashed_triangles(len(p), [0, 0, 0], [0, 0, 0], 2 * ext, seed=3))).astype(np.float32)
        return [near, larger_than(av)]


# ---- the exact reference (snapped inputs) -------------------------------------------------------------------------------
GRID = 1024                                     # coordinates are k / GRID, |k| <= 2 * GRID


def snapped(x):
    """the integers k of coordinates k * 2^-10, asserting that the input is on the grid and |k| <= 2^11"""
    x = np.asarray(x, np.float64)
    k = x * GRID
    assert np.array_equal(k, np.round(k)) and (np.abs(k) <= 2 * GRID).all(), "input is not snapped to k * 2^-10, |k| <= 2^11"
    return k.astype(np.int64)


def snap_even(x, bound=0.25):
    """float32 coordinates scaled into [-bound, bound] and rounded to EVEN grid steps: midpoints of two of them are on the grid"""
    x = np.asarray(x, np.float64)
    x = x * (bound / np.abs(x).max())
    return (np.round(x * (GRID / 2)) / (GRID / 2)).astype(np.float32)


def _orient2(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _between2(a, b, c):
    """c (collinear with a, b) lies on the closed segment a .. b"""
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _segments_meet2(a, b, c, d):
    """closed segments a .. b and c .. d in the plane"""
    d1, d2, d3, d4 = _orient2(c, d, a), _orient2(c, d, b), _orient2(a, b, c), _orient2(a, b, d)
    if ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0)):
        return True
    return (d1 == 0 and _between2(c, d, a)) or (d2 == 0 and _between2(c, d, b)) or \
           (d3 == 0 and _between2(a, b, c)) or (d4 == 0 and _between2(a, b, d))


def _in_triangle2(x, t):
    s = [_orient2(t[k], t[(k + 1) % 3], x) for k in range(3)]
    return all(v >= 0 for v in s) or all(v <= 0 for v in s)


def segment_meets_triangle(p, q, tri, n):
    """the closed segment p .. q against the closed triangle tri with the normal n != 0; tuples of Python integers"""
    dp, dq = _dot(n, _sub(p, tri[0])), _dot(n, _sub(q, tri[0]))
    if (dp > 0 and dq > 0) or (dp < 0 and dq < 0):
        return False
    if dp == 0 and dq == 0:
        # in the plane: project onto the coordinate plane where the normal is largest (the triangle keeps its area there)
        drop = max(range(3), key=lambda k: abs(n[k]))
        u, w = (drop + 1) % 3, (drop + 2) % 3
        p2, q2, t2 = (p[u], p[w]), (q[u], q[w]), [(v[u], v[w]) for v in tri]
        if _in_triangle2(p2, t2) or _in_triangle2(q2, t2):
            return True
        return any(_segments_meet2(p2, q2, t2[k], t2[(k + 1) % 3]) for k in range(3))
    s = dp - dq                                      # the crossing is p + (dp / s) (q - p) = (p s + dp (q - p)) / s
    x = tuple(p[k] * s + dp * (q[k] - p[k]) for k in range(3))
    return _in_triangle_scaled(x, s, tri, n)


def _normal(t):
    return _cross(_sub(t[1], t[0]), _sub(t[2], t[0]))


def exact_meets(t, q):
    """closed triangles t and q (tuples of three integer points): both with area and sharing a point"""
    nt, nq = _normal(t), _normal(q)
    if nt == (0, 0, 0) or nq == (0, 0, 0):
        return False
    return any(segment_meets_triangle(q[k], q[(k + 1) % 3], t, nt) for k in range(3)) or \
        any(segment_meets_triangle(t[k], t[(k + 1) % 3], q, nq) for k in range(3))


def coplanar(t, q):
    """both with area and in one plane"""
    nt, nq = _normal(t), _normal(q)
    return nt != (0, 0, 0) and nq != (0, 0, 0) and _cross(nt, nq) == (0, 0, 0) and _dot(nt, _sub(q[0], t[0])) == 0


def only_touching(t, q):
    """for a pair that meets: the triangles ONLY TOUCH -- on one of the seventeen axes, in integers, the two spans share
    exactly an end, so a predicate that separated on equality would call them apart.  A shared vertex, a vertex on an edge,
    an edge across an edge with the triangles on either side, and coplanar triangles that share boundary only are all of this
    kind; triangles whose interiors cross are not.  Used to COUNT the coverage, never as the reference."""
    e = [_sub(t[1], t[0]), _sub(t[2], t[1]), _sub(t[0], t[2])]
    f = [_sub(q[1], q[0]), _sub(q[2], q[1]), _sub(q[0], q[2])]
    nt, nq = _cross(e[0], e[1]), _cross(f[0], f[1])
    axes = [nt, nq] + [_cross(a, b) for a in e for b in f] + [_cross(nt, a) for a in e] + [_cross(nq, b) for b in f]
    for L in axes:
        if L == (0, 0, 0):
            continue
        ts = [_dot(L, _sub(v, t[0])) for v in t]
        qs = [_dot(L, _sub(v, t[0])) for v in q]
        if min(qs) >= max(ts) or max(qs) <= min(ts):
            return True
    return False


def _as_int_triangles(x):
    return [tuple(tuple(int(c) for c in p) for p in t) for t in snapped(x).reshape(-1, 3, 3)]


def exact_tables(v, f, tri):
    """(met, touching, coplanar) [n, F] bool each, by the functions above on snapped inputs (asserted)"""
    T, Q = _as_int_triangles(np.asarray(v, np.float32)[np.asarray(f)]), _as_int_triangles(tri)
    met, touch, cop = (np.zeros((len(Q), len(T)), bool) for _ in range(3))
    for i, q in enumerate(Q):
        for j, t in enumerate(T):
            cop[i, j] = coplanar(t, q)
            met[i, j] = exact_meets(t, q)
            touch[i, j] = met[i, j] and only_touching(t, q)
    return met, touch, cop


def flat_mesh():
    """a mesh with coplanar and degenerate faces mixed in, on even grid steps: a 3 x 3 patch of squares in the plane z = 0
    (18 faces), a 2 x 2 patch in the tilted plane x + z = 1/4 (8 faces), and the six zero-area triangles of the soup"""
    vs, fs = [], []

    def patch(p0, du, dv, nu, nv):
        base = len(vs)
        for i in range(nu + 1):
            for j in range(nv + 1):
                vs.append([p0[k] + i * du[k] + j * dv[k] for k in range(3)])
        for i in range(nu):
            for j in range(nv):
                a, b, c, d = (base + i * (nv + 1) + j, base + (i + 1) * (nv + 1) + j, base + (i + 1) * (nv + 1) + j + 1, base + i * (nv + 1) + j + 1)
                fs.extend([[a, b, c], [a, c, d]])
    patch([-0.375, -0.375, 0.0], [0.25, 0, 0], [0, 0.25, 0], 3, 3)
    patch([0.0, -0.25, 0.25], [0.125, 0, -0.125], [0, 0.25, 0], 2, 2)
    sv, sf, _ = NC.soup_with_degenerates()
    deg = (sv[sf[-6:].reshape(-1)] * np.float32(0.5)).tolist()
    for k in range(6):
        fs.append([len(vs) + 3 * k, len(vs) + 3 * k + 1, len(vs) + 3 * k + 2])
    return np.array(vs + deg, np.float32), np.array(fs, np.int32)


def snapped_meshes():
    """{name: (v, f)} on EVEN grid steps: the cube and the icosphere within [-1/4, 1/4], and flat_mesh()"""
    cv, cf, _ = NC.cube()
    iv, i_f, _ = NC.icosphere()
    fv, ff = flat_mesh()
    out = {"cube": (snap_even(cv), cf), "icosphere": (snap_even(iv), i_f), "flat": (fv, ff)}
    for v, _ in out.values():
        assert (snapped(v) % 2 == 0).all()
    return out


SNAPPED_QUERIES = {"cube": 280, "icosphere": 48, "flat": 260}
SNAPPED_KINDS = {"cube": (0, 1, 2, 3), "icosphere": (0, 1, 2, 3), "flat": (0, 2, 1, 2, 3, 2)}      # the flat mesh: half in a face's plane
_STEPS = np.array([0, 0, 0, 32, -32, 64, -64, 128, 256, -256]) / GRID      # small offsets, in grid steps (0 three times as likely)


def lattice_triangles(v, f, n, seed, kinds=(0, 1, 2, 3)):
    """[n, 3, 3] float32 on the grid, drawn from the mesh's own vertices so that they touch it in every way; query i is of the
    kind kinds[i % len(kinds)]:
      0: three vertices of the mesh (a query that shares vertices, edges or a whole face with it);
      1: three vertices of the mesh, each moved by small steps along the axes;
      2: IN THE PLANE of a face (a, b, c): the points a + i (b - a) / 2 + j (c - a) / 2 for small i, j -- coplanar with it,
         across it, beside it with a shared edge or a shared vertex, or apart;
      3: a face of the mesh moved as a whole by small steps (often along its own plane).
    Degenerate picks stay in: they must meet nothing."""
    v, f = np.asarray(v, np.float64), np.asarray(f)
    fa = f[[not np.array_equal(np.cross(v[t[1]] - v[t[0]], v[t[2]] - v[t[0]]), np.zeros(3)) for t in f]]
    h = [_hash01(n, seed + 977 * k) for k in range(12)]
    out = np.zeros((n, 3, 3))
    halves = np.array([-1, 0, 0, 1, 1, 2, 2, 3]) / 2
    for i in range(n):
        kind = kinds[i % len(kinds)]
        if kind in (0, 1):
            out[i] = v[[int(h[k][i] * len(v)) for k in range(3)]]
            if kind == 1:
                out[i] += _STEPS[[int(h[3 + k][i] * len(_STEPS)) for k in range(9)]].reshape(3, 3)
        elif kind == 2:
            a, b, c = v[fa[int(h[0][i] * len(fa))]]
            for k in range(3):
                ci, cj = halves[int(h[1 + 2 * k][i] * len(halves))], halves[int(h[2 + 2 * k][i] * len(halves))]
                out[i, k] = a + ci * (b - a) + cj * (c - a)
        else:
            out[i] = v[fa[int(h[0][i] * len(fa))]] + _STEPS[[int(h[1 + k][i] * len(_STEPS)) for k in range(3)]]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def snapped_reference():
    """{mesh: (v, f, queries, met, touching, coplanar)}: computed once per process and never changed"""
    out = {}
    for k, (name, (v, f)) in enumerate(snapped_meshes().items()):
        tri = lattice_triangles(v, f, SNAPPED_QUERIES[name], seed=100 * k, kinds=SNAPPED_KINDS[name])
        met, touch, cop = exact_tables(v, f, tri)
        for a in (tri, met, touch, cop):
            a.setflags(write=False)
        out[name] = (v, f, tri, met, touch, cop)
    return out


def check_snapped(run, what):
    """run(v, f, triangles) -> Result; on every snapped mesh the sets must EQUAL the exact reference pair for pair, pairs that
    only touch and coplanar pairs included.  Returns {mesh: (pairs, met, only touching, coplanar)}"""
    stats = {}
    for name, (v, f, tri, want, touching, cop) in snapped_reference().items():
        res = run(v, f, tri)
        got = listed(res, len(tri), len(f))
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{what}, {name}: {len(bad)} of {want.size} pairs differ from the exact reference, the first (query, face) {bad[:4].tolist()}"
        assert np.array_equal(res.count, want.sum(1)) and np.array_equal(res.any, want.any(1)), f"{what}, {name}"
        check_identities(res, f"{what}, {name}")
        stats[name] = (int(want.size), int(want.sum()), int(touching.sum()), int(cop.sum()))
    return stats


def check_coverage(stats):
    """the floors on what the snapped set covers: of the meeting pairs at least a fifth only touch, of all pairs at least a
    tenth are coplanar"""
    pairs, met, touching, cop = (sum(s[k] for s in stats.values()) for k in range(4))
    assert 0 < met < pairs
    assert 5 * touching >= met, f"only {touching} of {met} meeting pairs only touch"
    assert 10 * cop >= pairs, f"only {cop} of {pairs} pairs are coplanar"
    return pairs, met, touching, cop
