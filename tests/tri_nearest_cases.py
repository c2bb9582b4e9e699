"""Shared by tests/test_tri_nearest_cpu.py and tests/test_gpu_tri_nearest.py (not a test module): the meshes of the
triangles_nearest checks -- those of tests/nearest_cases.py --, their query triangles, the bit-for-bit comparison of two results,
a numpy model of mesh_distance's chunked reduction, and two independent evaluations of the distance of two triangles.

1. EXACT, on snapped inputs (tests/tris_cases.py: coordinates k * 2^-10, |k| <= 2^11), in Python integers and fractions.  It
   shares nothing with csrc/tr_tri_nearest.h: the squared distance of a point and a triangle is that of its projection where
   the projection falls inside (three integer edge functions), else the least over the three edges as segments; the squared
   distance of two segments is taken at the critical point of the quadratic where that lies in the unit square (its ends are
   ends of one segment against the other and are covered by the point-triangle terms).  The distance of a pair is the least of
   six point-triangle and nine segment-segment terms, and 0 where tris_cases.exact_meets says the pair meets.
2. NUMPY FLOAT64, off the grid: nearest_cases' point-triangle distance applied to the witness points and to densely
   parametrised edge points -- an upper bound of the true distance, so the comparison with it is one-sided."""
import functools
from fractions import Fraction

import numpy as np

import nearest_cases as NC
import tris_cases as TC

CASES = NC.HIERARCHICAL                        # cube, icosphere, soup, deep
NAMES = ("tri", "distance", "closest_mesh", "closest_query")


# ---- query triangles ----------------------------------------------------------------------------------------------------
def sized_triangles(n, centre, ext, seed=0):
    """[n, 3, 3] float32: centres hashed within 1.5 extents of `centre`, vertices hashed within size / 2 of them, size = a tenth
    of the extent, half of it and three times it in turn"""
    centre = np.asarray(centre, np.float64)
    c = NC.hash_points(n, seed, centre - 1.5 * ext, centre + 1.5 * ext).astype(np.float64)
    size = np.array([ext / 10, ext / 2, 3 * ext])[np.arange(n) % 3]
    d = np.stack([NC.hash_points(n, seed + 1 + k, [-0.5] * 3, [0.5] * 3) for k in range(3)], 1).astype(np.float64)
    return (c[:, None, :] + d * size[:, None, None]).astype(np.float32)


def query_sets(v, f):
    """[(label, triangles [n, 3, 3])]: the mesh's own faces (distance 0), those displaced by 1 / 32 of the extent and by two
    extents, 200 hashed triangles of three sizes, and degenerate queries (a doubled vertex, three equal vertices)"""
    ext = TC.extent(v)
    own = TC.own_faces(v, f)
    fin = np.asarray(v, np.float64)[np.isfinite(v).all(1)]
    out = [("own faces", own)]
    for fr in (1 / 32, 2.0):
        d = (np.float64(fr * ext) * np.array([2, -1, 2]) / 3).astype(np.float32)
        out.append((f"own faces displaced by {fr:g} of the extent", (own + d).astype(np.float32)))
    hashed = sized_triangles(200, (fin.max(0) + fin.min(0)) / 2, ext, seed=7)
    out.append(("hashed", hashed))
    deg = hashed[:24].copy()
    deg[:12, 2] = deg[:12, 1]              # a doubled vertex: a segment
    deg[12:] = deg[12:, :1]                # three equal vertices: a point
    out.append(("degenerate", deg))
    return out


def all_queries(v, f):
    """the query sets of a mesh as one array"""
    return np.concatenate([tri for _, tri in query_sets(v, f)])


def half_bound(distance):
    """a max_distance that admits roughly half of the queries: the median of the positive finite unbounded distances"""
    d = np.asarray(distance, np.float32)
    d = d[np.isfinite(d) & (d > 0)]
    return np.float32(np.median(d)) if len(d) else np.float32(0)


def assert_same(got, want, what):
    """(tri, distance, closest_mesh, closest_query) against the same: tri equal, the three float arrays bit for bit (NaN == NaN);
    None entries of `got` are skipped"""
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, expected {w.shape}"
        assert g.dtype == w.dtype, f"{what}: {name} has type {g.dtype}, expected {w.dtype}"
        same = (g == w) if name == "tri" else (NC.bits(g) == NC.bits(w))
        if not same.all():
            bad = np.flatnonzero(~same.reshape(len(g), -1).all(1))
            raise AssertionError(f"{what}: {name} differs at {bad[:8]} ({len(bad)} of {len(g)}): {g[bad[:4]]} != {w[bad[:4]]}")


def check_no_result(got, rows, what):
    """the rows of a result that must be (-1, +Inf, NaN, NaN)"""
    tri, distance, on_mesh, on_query = got
    assert (tri[rows] == -1).all() and np.isposinf(distance[rows]).all(), what
    assert np.isnan(on_mesh[rows]).all() and np.isnan(on_query[rows]).all(), what


# ---- mesh_distance's reduction --------------------------------------------------------------------------------------------
def reduce_rows(rows, chunk=None, max_distance=None):
    """a numpy model of RayMeshIntersector.mesh_distance on the unbounded per-face rows (tri, distance, closest_mesh,
    closest_query) of the other mesh's faces: chunks ascend, each after the first bounded by the best float32 distance so far (a
    row is dropped where its float32 distance exceeds the bound -- the kernel may also drop one that rounds to exactly the bound,
    which cannot win), ties go to the earlier row.  -> (distance, other face, face, point on other, point on self)"""
    tri, distance, on_mesh, on_query = rows
    n = len(tri)
    chunk = n if chunk is None else chunk
    nan3 = np.full(3, np.nan, np.float32)
    best = (np.float32(np.inf), -1, -1, nan3, nan3)
    bound = np.float32(np.inf) if max_distance is None else np.float32(max_distance)
    for start in range(0, n, max(chunk, 1)):
        d = distance[start:start + chunk].copy()
        d[~(d <= bound) | (tri[start:start + chunk] < 0)] = np.inf
        if len(d) == 0 or not d.min() < best[0]:
            continue
        k = start + int(np.flatnonzero(d == d.min())[0])
        best = (distance[k], k, int(tri[k]), on_query[k], on_mesh[k])
        bound = distance[k]
    return best


def assert_same_pair(got, want, what):
    """two results of mesh_distance / reduce_rows, bit for bit"""
    assert np.float32(got[0]).view(np.uint32) == np.float32(want[0]).view(np.uint32), f"{what}: distance {got[0]} != {want[0]}"
    assert int(got[1]) == int(want[1]) and int(got[2]) == int(want[2]), f"{what}: faces ({got[1]}, {got[2]}) != ({want[1]}, {want[2]})"
    for k in (3, 4):
        assert np.array_equal(NC.bits(got[k]), NC.bits(want[k])), f"{what}: point {k - 3} {got[k]} != {want[k]}"


# ---- independent evaluation 1: exact --------------------------------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def exact_point_segment(p, a, b):
    """squared distance of the point p and the closed segment a .. b (integer points) as a Fraction"""
    e, w = _sub(b, a), _sub(p, a)
    ee, we = _dot(e, e), _dot(w, e)
    if ee == 0 or we <= 0:
        return Fraction(_dot(w, w))
    if we >= ee:
        u = _sub(p, b)
        return Fraction(_dot(u, u))
    return Fraction(_dot(w, w) * ee - we * we, ee)


def exact_point_triangle(p, t):
    """squared distance of the point p and the closed triangle t"""
    a, b, c = t
    n = _cross(_sub(b, a), _sub(c, a))
    nn = _dot(n, n)
    if nn != 0:
        # p projects inside iff it is on the inner side of the three edge planes (the component along n drops out)
        inside = all(_dot(_cross(_sub(y, x), _sub(p, x)), n) >= 0 for x, y in ((a, b), (b, c), (c, a)))
        if inside:
            h = _dot(_sub(p, a), n)
            return Fraction(h * h, nn)
    return min(exact_point_segment(p, a, b), exact_point_segment(p, b, c), exact_point_segment(p, c, a))


def exact_segments_inside(v, v2, w, w2):
    """squared distance of the lines through the segments v .. v2 and w .. w2 where the nearest points lie on both segments,
    else None (the minimum is then at an end of one of them: a point-segment term)"""
    e, f, r = _sub(v2, v), _sub(w2, w), _sub(v, w)
    A, B, C, D, G = _dot(e, e), _dot(e, f), _dot(f, f), _dot(e, r), _dot(f, r)
    det = A * C - B * B
    if det <= 0:
        return None
    sn, tn = B * G - C * D, A * G - B * D              # s = sn / det, t = tn / det
    if sn < 0 or sn > det or tn < 0 or tn > det:
        return None
    n = _cross(e, f)                                    # |n|^2 = det; the distance of the lines is |r . n| / |n|
    h = _dot(r, n)
    return Fraction(h * h, det)


def exact_candidates(q, t):
    """the least of the six point-triangle and nine segment-segment terms of two triangles (tuples of three integer points)"""
    best = min(min(exact_point_triangle(p, t) for p in q), min(exact_point_triangle(p, q) for p in t))
    for i in range(3):
        for j in range(3):
            d = exact_segments_inside(q[i], q[(i + 1) % 3], t[j], t[(j + 1) % 3])
            if d is not None and d < best:
                best = d
    return best


def _has_area(t):
    return _cross(_sub(t[1], t[0]), _sub(t[2], t[0])) != (0, 0, 0)


@functools.lru_cache(maxsize=None)
def exact_reference():
    """{mesh: (v, f, queries, met [n, F] bool, area_q [n] bool, area_t [F] bool, d2 [n, F] float64)} on the snapped meshes and
    queries of tris_cases.snapped_reference: d2 is the exact squared distance (0 where the pair meets) in coordinate units,
    rounded once to float64.  Computed once per process and never changed"""
    out = {}
    unit = Fraction(1, TC.GRID * TC.GRID)
    for name, (v, f, tri, met, _, _) in TC.snapped_reference().items():
        T, Q = TC._as_int_triangles(np.asarray(v, np.float32)[np.asarray(f)]), TC._as_int_triangles(tri)
        d2 = np.zeros((len(Q), len(T)))
        for i, q in enumerate(Q):
            for j, t in enumerate(T):
                d2[i, j] = 0.0 if met[i, j] else float(exact_candidates(q, t) * unit)
        area_q, area_t = np.array([_has_area(q) for q in Q]), np.array([_has_area(t) for t in T])
        for a in (d2, area_q, area_t):
            a.setflags(write=False)
        out[name] = (v, f, tri, met, area_q, area_t, d2)
    return out


def eps_of(value, S):
    """the tolerance form of nearest_cases.check_against_numpy: one float32 spacing of the value plus 2^-40 of the scale"""
    return NC.u32(value) + 2.0 ** -40 * S


def check_exact_winner(name, got, what):
    """a result on the snapped mesh `name` and its snapped queries against the exact reference: the distance within eps, 0
    exactly where a pair with area meets, the winner an exact minimiser within eps.  Prints the worst excess before it asserts"""
    v, f, tri, met, area_q, area_t, d2 = exact_reference()[name]
    face, distance = got[0], got[1].astype(np.float64)
    S = float(max(np.abs(v).max(), np.abs(tri).max()))
    rows = np.arange(len(tri))
    assert ((face >= 0) & (face < len(f))).all(), what
    d_min = np.sqrt(d2.min(1))
    e_dist = np.abs(distance - d_min) - eps_of(d_min, S)
    e_win = np.sqrt(d2[rows, face]) - (d_min + eps_of(d_min, S))
    print(f"{what}, {name}: worst excess over the bound (<= 0 passes): distance {e_dist.max():.3g}, winner {e_win.max():.3g}")
    assert (e_dist <= 0).all(), f"{what}, {name}: distance, {int((e_dist > 0).sum())} queries, worst excess {e_dist.max()}"
    assert (e_win <= 0).all(), f"{what}, {name}: the returned face is not an exact minimiser, worst excess {e_win.max()}"
    meets = met.any(1)
    assert meets.any() and not meets.all()
    assert (got[1][meets] == 0).all() and (got[1][d_min > 0] > 0).all(), f"{what}, {name}: 0 exactly where a pair with area meets"
    # the smallest meeting face wins a query that meets
    assert np.array_equal(face[meets], met.argmax(1)[meets]), f"{what}, {name}: the smallest meeting face wins"


# ---- independent evaluation 2: numpy float64 -------------------------------------------------------------------------------
def edge_points(tri, k=9):
    """[n, 3 k, 3] float64: k points on each edge of the triangles, both ends included"""
    tri = np.asarray(tri, np.float64)
    s = np.linspace(0.0, 1.0, k)[None, :, None]
    return np.concatenate([tri[:, e, None, :] * (1 - s) + tri[:, (e + 1) % 3, None, :] * s for e in range(3)], 1)


def numpy_upper_bound(v, f, tri):
    """[n, F] float64: an upper bound of the distance of query i and face j -- the least point-triangle distance over edge
    points of the query against the face and over the face's vertices against the query; +Inf to an inactive face"""
    v, tri = np.asarray(v, np.float64), np.asarray(tri, np.float64)
    ok = NC.active(v, f)
    vv = np.where(np.isfinite(v), v, 0.0)
    a, b, c = (vv[f[:, k]] for k in range(3))
    pts = edge_points(tri)
    ub = np.full((len(tri), len(f)), np.inf)
    for k in range(pts.shape[1]):
        ub = np.minimum(ub, NC._distance(pts[:, k, None, :], a[None], b[None], c[None]))
    for p in (a, b, c):
        ub = np.minimum(ub, NC._distance(p[None, :, :], tri[:, None, 0], tri[:, None, 1], tri[:, None, 2]))
    return np.where(ok[None, :], ub, np.inf)


def check_against_numpy(v, f, tri, got, what):
    """the three tolerance checks of the triangles_nearest contract on finite queries; prints each figure before it asserts"""
    v, f, tri = np.asarray(v, np.float32), np.asarray(f, np.int32), np.asarray(tri, np.float32)
    face, distance, on_mesh, on_query = got
    assert np.isfinite(tri).all() and (face >= 0).all() and NC.active(v, f)[face].all(), what
    S = float(max(np.abs(v[f[NC.active(v, f)].reshape(-1)]).max(), np.abs(tri).max()))
    n = len(tri)
    dist64 = distance.astype(np.float64)
    e_mesh = NC.numpy_distances_paired(v, f, face, on_mesh) - 2 * NC.u32(S)
    e_query = NC.numpy_distances_paired(tri.reshape(-1, 3), np.arange(3 * n).reshape(n, 3), np.arange(n), on_query) - 2 * NC.u32(S)
    apart = distance > 0
    gap = np.linalg.norm(on_query.astype(np.float64) - on_mesh.astype(np.float64), axis=1)
    e_cons = np.where(apart, np.abs(gap - dist64) - (2 * NC.u32(S) + NC.u32(distance)), -np.inf)
    ub = numpy_upper_bound(v, f, tri).min(1)
    e_under = dist64 - (ub + eps_of(ub, S))
    print(f"{what}: S = {S:g}, worst excess over the bound (<= 0 passes): witness on the face {e_mesh.max():.3g}, on the query "
          f"{e_query.max():.3g}, consistency {e_cons.max():.3g}, above numpy's upper bound {e_under.max():.3g}; distance 0: {int((~apart).sum())} of {n}")
    assert (e_mesh <= 0).all(), f"{what}: closest_mesh off its face, worst excess {e_mesh.max()}"
    assert (e_query <= 0).all(), f"{what}: closest_query off the query, worst excess {e_query.max()}"
    assert (e_cons <= 0).all(), f"{what}: |closest_query - closest_mesh| against distance, worst excess {e_cons.max()}"
    assert (e_under <= 0).all(), f"{what}: a face is nearer than the returned distance, worst excess {e_under.max()}"
