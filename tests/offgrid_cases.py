"""Shared by tests/test_offgrid_cpu.py and tests/test_gpu_offgrid.py (not a test module): box, triangle and plane queries OFF
THE LATTICE -- ordinary float32 coordinates with full mantissas -- and their answers in exact arithmetic.

Every finite float32 is a dyadic rational, so a set of float32 arrays times one power of two is a set of integers (exact_ints),
and the integer references that tests/boxes_cases.py, tests/tris_cases.py and tests/planes_cases.py apply to snapped inputs
apply to any input: boxes_cases.exact_meets, tris_cases.exact_meets / coplanar / only_touching are REUSED here, not restated.
They share nothing with csrc/tr_boxes.h, tr_tris.h and tr_planes.h, which decide in float64: off the lattice float64 rounds,
and what holds the predicates to geometry there is this module.

FAMILIES.  The 80-face icosphere, displaced, then scaled / moved and rounded to float32 (all later work is on the rounded
values): unit; offset4096 (+ (4096, -4096, 2048)); offset2e20 (* 64 + (2^20, 2^20, -2^20)); tiny (* 1e-30); huge (* 1e30);
aniso (* (1e4, 1, 1e-4)); denormal (* 2^-130); and flat: 60 triangles of their own vertices with hashed x, y in [-1, 1] and
z = float32(0.3) throughout -- exactly coplanar pairs with nothing on a lattice.

NEAR-TOUCHING QUERIES.  Every generator builds, in float64, a contact with one face (the AIMED face), rounds it to float32 and
moves the touching coordinate -- the one along which a float32 step moves the contact most -- by k in {-2, .., 2} float32 steps
(np.nextafter); k > 0 moves the query away from the face.  The rest of the query points away from the face.  The five queries
of one contact are a SERIES.  See tri_queries, box_queries and plane_queries for the kinds.

WHAT MAY BE LEFT OUT of a comparison with the exact tables is decided here, in exact arithmetic, never by what the code under
test returns: for boxes and triangles an EXACT TIE (tri_tie, box_tie: the exact reference says "meets" and on a non-zero axis
of the contract, on which not both spans are single points, the two exact spans share exactly one end); for planes a vertex
whose exact signed value is non-zero and smaller than 2^-51 sum_k |n_k| |v_k - o_k| (three operands, two roundings), and for
a crossing point an edge with sum_k |n_k| |w_k - u_k| > 2^16 |s(u) - s(w)|.  The caps: LEFT_OUT_CAP of a family's pairs,
ILL_CONDITIONED_CAP of its rows."""
import collections
import functools
import math
from fractions import Fraction

import numpy as np

import boxes_cases as BC
import tris_cases as TC
import workloads as W
from boxes_cases import _cross, _dot, _sub

KS = (-2, -1, 0, 1, 2)
FAMILIES = ("unit", "offset4096", "offset2e20", "tiny", "huge", "aniso", "denormal", "flat")
ANISO = np.array([1e4, 1.0, 1e-4])
TRANSFORMS = {                                   # name: (scale, offset), applied in float64 to the displaced icosphere
    "unit": (1.0, 0.0),
    "offset4096": (1.0, np.array([4096.0, -4096.0, 2048.0])),
    "offset2e20": (64.0, np.array([2.0 ** 20, 2.0 ** 20, -2.0 ** 20])),
    "tiny": (1e-30, 0.0),
    "huge": (1e30, 0.0),
    "aniso": (ANISO, 0.0),
    "denormal": (2.0 ** -130, 0.0),
}
FLAT_Z = np.float32(0.3)
LEFT_OUT_CAP = 0.005                             # of a family's pairs (boxes, triangles: exact ties; planes: |s| below the bound)
ILL_CONDITIONED_CAP = 0.05                       # of a family's section rows
MEET_SHARE = (0.2, 0.8)                          # of the aimed pairs of every (family, kind) the exact reference says "meets"

TRI_KINDS = ("vertex on a face interior", "vertex on an edge", "edge across an edge")
FLAT_TRI_KINDS = ("vertex on an edge, in the plane", "edge past a vertex, in the plane")
BOX_KINDS = ("corner on a face interior", "box edge through a point of a face edge", "flat box through a vertex",
             "proper box with a face through a vertex")
PLANE_KINDS = ("origin at a vertex", "origin a vertex moved by steps", "origin a rounded point of an edge",
               "origin beside a vertex, in the plane through it")

# data: triangles float32 [n, 3, 3] / boxes (lo, hi) float32 [n, 3] each / planes (origins, normals) float32 [n, 3] each;
# kind [n]: index into `kinds`; face [n]: the aimed face (planes: the aimed vertex, or the face whose edge holds the origin);
# k [n]: float32 steps away from the face; series [n]: the contact this query is a step of (-1: none)
Queries = collections.namedtuple("Queries", "data kinds kind face k series")


# ---- float32 values as integers --------------------------------------------------------------------------------------------
def exact_ints(*arrays):
    """float32 arrays -> (object arrays of Python integers of the same shapes ..., e): every value x of every array is exactly
    (its integer) * 2^e, with ONE e for all arrays (the smallest exponent of a significand bit among them; 0 where everything
    is 0).  The round trip is asserted, so is finiteness.  -0 maps to 0."""
    arrs = [np.asarray(a) for a in arrays]
    parts = []
    e_min = None
    for a in arrs:
        assert a.dtype == np.float32, "exact_ints takes float32 arrays"
        assert np.isfinite(a).all(), "exact_ints takes finite values"
        m, e = np.frexp(a.astype(np.float64))                 # exact: x = m * 2^e, 1/2 <= |m| < 1; 24 bits of m at the most
        m24 = m * 16777216.0
        assert np.array_equal(m24, np.round(m24))
        m24, e = m24.astype(np.int64), e.astype(np.int64) - 24
        low = np.log2((m24 & -m24) + (m24 == 0)).astype(np.int64)      # trailing zeros: x = (m24 >> low) * 2^(e + low)
        m24, e = m24 >> low, e + low
        parts.append((m24, e))
        if (m24 != 0).any():
            lowest = int(e[m24 != 0].min())
            e_min = lowest if e_min is None else min(e_min, lowest)
    e_min = 0 if e_min is None else e_min
    out = []
    for a, (m24, e) in zip(arrs, parts):
        flat = [int(m) << (int(x) - e_min) if m else 0 for m, x in zip(m24.ravel().tolist(), e.ravel().tolist())]
        back = np.array([math.ldexp(float(k), e_min) for k in flat], np.float64).astype(np.float32).reshape(a.shape)
        assert np.array_equal(back, a) and all(Fraction(k) * Fraction(2) ** e_min == Fraction(float(x))
                                               for k, x in zip(flat[:64], a.ravel()[:64].tolist())), "exact_ints: round trip"
        ints = np.empty(len(flat), object)
        ints[:] = flat
        out.append(ints.reshape(a.shape))
    return (*out, e_min)


def _points(a):
    """an object array [.., 3] of integers -> a list of tuples of three Python integers"""
    return [tuple(p) for p in a.reshape(-1, 3).tolist()]


def _triangles(a):
    """an object array [n, 3, 3] -> a list of triangles, each a tuple of three integer points (the layout of exact_meets)"""
    p = _points(a)
    return [tuple(p[3 * i:3 * i + 3]) for i in range(len(p) // 3)]


# ---- families --------------------------------------------------------------------------------------------------------------
def hashed(n, seed):
    """n float64 in [0, 1) with full mantissas: a 64-bit mixing hash of (index, seed), deterministic"""
    x = np.arange(n, dtype=np.uint64) + np.uint64(seed * 0x9E3779B97F4A7C15 % (1 << 64))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) / float(1 << 53)


@functools.lru_cache(maxsize=None)
def family(name):
    """(v float32 [nv, 3], f int32 [F, 3]) of a family, read-only.  No face is degenerate under the exact normal (asserted)."""
    if name == "flat":
        n = 180
        v = np.stack([(2 * hashed(n, 11) - 1).astype(np.float32), (2 * hashed(n, 29) - 1).astype(np.float32),
                      np.full(n, FLAT_Z, np.float32)], 1)
        f = np.arange(n, dtype=np.int32).reshape(-1, 3)
    else:
        v0, f = W.icosphere(1)
        scale, offset = TRANSFORMS[name]
        v = (W.displaced(v0, seed=3, amplitude=0.08).astype(np.float64) * scale + offset).astype(np.float32)
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    V, _ = exact_ints(v)
    for t in _triangles(V[f]):
        assert TC._normal(t) != (0, 0, 0), f"{name}: a degenerate face"
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


# ---- pieces of the generators (float64 geometry on the float32 values) -----------------------------------------------------
def _unit(x):
    x = np.asarray(x, np.float64)
    x = x / np.abs(x).max()                                    # (keeps the squares of tiny and denormal lengths in range)
    return x / np.sqrt((x * x).sum())


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _step(x, steps):
    """the float32 x moved by `steps` float32 steps (negative: down)"""
    x = np.float32(x)
    to = np.float32(np.inf if steps > 0 else -np.inf)
    for _ in range(abs(int(steps))):
        x = np.nextafter(x, to)
    return x


def _touching_axis(direction, at, axes=(0, 1, 2)):
    """(axis, sign): the coordinate of the float32 point `at` (or the larger step of several points [m, 3]) whose float32 step
    moves the point furthest along `direction`, and the sign of a step that moves it forward"""
    at = np.abs(np.asarray(at, np.float32).reshape(-1, 3))
    reach = np.abs(np.asarray(direction, np.float64)) * np.spacing(at).astype(np.float64).max(0)
    axis = max(axes, key=lambda k: reach[k])
    return axis, (1 if direction[axis] >= 0 else -1)


class _Face:
    """a face seen from one of its edges: A -> B is the edge, C the third vertex, e the unit edge, n the unit normal, m the
    unit in-plane normal of the edge pointing AWAY from C, h a length well below the face's size"""

    def __init__(self, v, t, edge=0):
        self.A, self.B, self.C = (np.asarray(v[t[(edge + i) % 3]], np.float64) for i in range(3))
        self.e = _unit(self.B - self.A)
        self.n = _unit(np.cross(_unit(self.B - self.A), _unit(self.C - self.A)))
        m = np.cross(self.e, self.n)
        self.m = _unit(-m if m @ (self.C - self.A) > 0 else m)
        edges = (self.B - self.A, self.C - self.B, self.A - self.C)
        self.h = 0.3 * min(math.sqrt(float((d * d).sum())) for d in edges)      # (2^-260 and 1e60 are ordinary float64)
        corners = np.stack([self.A, self.B, self.C])
        ext = corners.max(0) - corners.min(0)
        self.half = 0.3 * np.where(ext > 0, ext, ext.max())                  # per axis: a box well below the face's size

    def inside(self, w):
        w = 0.2 + 0.6 * np.asarray(w)
        w = w / w.sum()
        return w[0] * self.A + w[1] * self.B + w[2] * self.C

    def on_edge(self, u):
        return self.A + (0.2 + 0.6 * u) * (self.B - self.A)


def _aimed_faces(name, nf):
    """the faces the queries aim at: 64 of the icosphere's 80 (every fifth left out), all 60 of the flat family"""
    return [i for i in range(nf) if name == "flat" or i % 5 != 4]


# ---- triangle queries ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tri_queries(name):
    """Queries of a family, about 1 000.  Kinds (TRI_KINDS), each a series over k per aimed face:
      vertex on a face interior -- p on the face, q and r on the positive side of its plane: meets iff p is on or below it;
      vertex on an edge -- p on the edge A .. B, q above and r below the face's plane, both beyond the edge: the query crosses
        the plane in a segment that starts at p and runs away from the face: meets iff that start is on or inside the edge
        (q and r stand three times as high as they are far, so p's rounding off the plane moves the start by a third of it);
      edge across an edge -- the edge p .. q crosses A .. B from above to below, r beyond the edge: as before, with the start
        on p .. q; both p and q are moved.
    On `flat` (FLAT_TRI_KINDS), everything in the plane z = float32(0.3):
      vertex on an edge -- p on A .. B, q and r beyond the edge;
      edge past a vertex -- the line p .. q passes through the vertex A across the bisector of its corner, r beyond: meets iff
        A is on or behind the line; both p and q are moved."""
    v, f = family(name)
    flat = name == "flat"
    kinds = FLAT_TRI_KINDS if flat else TRI_KINDS
    tri, kind, face, ks = [], [], [], []
    faces = _aimed_faces(name, len(f))
    h1, h2, h3, h4 = (hashed(len(f) * 4, s) for s in (101, 102, 103, 104))
    for fi in faces:
        for kd in range(len(kinds)):
            for rep in range(2 if flat else 1):                     # flat: two contacts per face and kind (60 faces only)
                x = fi * 4 + kd + rep * 2
                F = _Face(v, f[fi], edge=int(h4[x] * 3))
                h = F.h
                moved = (0,)
                if flat and kd == 0:
                    c = F.on_edge(h1[x])
                    pts = [c, c + F.m * h + F.e * 0.4 * h, c + F.m * 1.3 * h - F.e * 0.3 * h]
                    axis, sign = _touching_axis(F.m, _f32(c), axes=(0, 1))
                elif flat:
                    away = -_unit(_unit(F.B - F.A) + _unit(F.C - F.A))
                    along = np.array([-away[1], away[0], 0.0])
                    pts = [F.A + along * h, F.A - along * h, F.A + away * h]
                    moved = (0, 1)
                    axis, sign = _touching_axis(away, _f32(pts[:2]), axes=(0, 1))
                elif kd == 0:
                    c = F.inside((h1[x], h2[x], h3[x]))
                    pts = [c, c + F.n * h + F.e * 0.3 * h, c + F.n * 1.2 * h - F.e * 0.2 * h + F.m * 0.25 * h]
                    axis, sign = _touching_axis(F.n, _f32(c))
                elif kd == 1:
                    c = F.on_edge(h1[x])
                    pts = [c, c + F.m * h + F.n * 3 * h + F.e * 0.2 * h, c + F.m * h - F.n * 3 * h - F.e * 0.1 * h]
                    axis, sign = _touching_axis(F.m, _f32(c))
                else:
                    c = F.on_edge(h1[x])
                    up = F.n * 2 * h + F.e * 0.5 * h
                    pts = [c + up, c - up, c + F.m * 2 * h]
                    moved = (0, 1)
                    axis, sign = _touching_axis(F.m, _f32(pts[:2]))
                base = _f32(pts)
                if flat:
                    base[:, 2] = FLAT_Z
                for k in KS:
                    q = base.copy()
                    for i in moved:
                        q[i, axis] = _step(q[i, axis], k * sign)
                    tri.append(q)
                    kind.append(kd)
                    face.append(fi)
                    ks.append(k)
    out = Queries(np.ascontiguousarray(tri, np.float32), kinds, np.array(kind), np.array(face), np.array(ks),
                  np.arange(len(tri)) // len(KS))
    out.data.setflags(write=False)
    return out


# ---- box queries -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_queries(name):
    """Queries of a family, about 1 000.  Kinds (BOX_KINDS), each a series over k per aimed face:
      corner on a face interior -- the box's lowest corner along the face's normal lies on the face, the box on the positive
        side: meets iff the corner is on or below the plane;
      box edge through a point of a face edge -- the box edge along the coordinate axis u most across A .. B passes through a
        point of A .. B; seen along u the box is a rectangle whose corner touches the line A .. B from the side away from C:
        meets iff the corner is on or across the line (the axis u x e of the contract);
      a box face through a vertex -- the vertex is the face's only extreme on a coordinate axis and the box begins there: a
        FLAT box (lo = hi on that axis) and a PROPER one in turn: meets iff the box's face is on or inside the vertex."""
    v, f = family(name)
    lo, hi, kind, face, ks = [], [], [], [], []
    faces = _aimed_faces(name, len(f))
    h1, h2, h3, h4 = (hashed(len(f) * 4, s) for s in (201, 202, 203, 204))
    for n_, fi in enumerate(faces):
        for kd in range(3):
            x = fi * 4 + kd
            F = _Face(v, f[fi], edge=int(h4[x] * 3))
            H = F.half
            if kd == 0:
                c = F.inside((h1[x], h2[x], h3[x]))
                out = F.n
                axes = (0, 1, 2)
            elif kd == 1:
                c = F.on_edge(h1[x])
                u = int(np.argmin(np.abs(F.e)))
                out = np.cross(np.eye(3)[u], F.e)
                out = -out if out @ (F.C - F.A) > 0 else out
                axes = tuple(a for a in range(3) if a != u)
            if kd < 2:
                c32 = _f32(c)
                blo, bhi = _f32(c - H), _f32(c + H)
                for a in axes:                                      # the box begins at c and extends along `out`
                    if out[a] >= 0:
                        blo[a] = c32[a]
                    else:
                        bhi[a] = c32[a]
                axis, sign = _touching_axis(out, c32, axes=axes)
                which = 0 if out[axis] >= 0 else 1                  # the bound that touches: lo or hi
                label = kd
            else:
                corners = np.stack([F.A, F.B, F.C])
                top = int(h2[x] * 2)                                # the vertex that is highest (1) / lowest (0) on the axis
                for axis in [(int(h1[x] * 3) + s) % 3 for s in range(3)]:
                    col = corners[:, axis]
                    at = int(np.argmax(col) if top else np.argmin(col))
                    if (np.delete(col, at) != col[at]).all():
                        break
                else:
                    raise AssertionError("a face without an extreme vertex")
                c = corners[at]
                blo, bhi = _f32(c - H), _f32(c + H)
                which, sign = (0, 1) if top else (1, -1)            # above the highest vertex: lo touches, and up is away
                proper = n_ % 2 == 1
                label = 3 if proper else 2
            for k in KS:
                l, g = blo.copy(), bhi.copy()
                bound = _step(c32[axis] if kd < 2 else np.float32(c[axis]), k * sign)
                (l if which == 0 else g)[axis] = bound
                if kd == 2 and not proper:
                    l[axis] = g[axis] = bound
                lo.append(l)
                hi.append(g)
                kind.append(label)
                face.append(fi)
                ks.append(k)
    lo, hi = np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(hi, np.float32)
    lo.setflags(write=False)
    hi.setflags(write=False)
    return Queries((lo, hi), BOX_KINDS, np.array(kind), np.array(face), np.array(ks), np.arange(len(lo)) // len(KS))


# ---- plane queries ---------------------------------------------------------------------------------------------------------
PLANE_VERTICES, PLANE_EDGES, PLANE_BESIDE = 34, 80, 14


@functools.lru_cache(maxsize=None)
def plane_queries(name):
    """Queries of a family, 320: GENERAL float32 normals hashed in [-1, 1]^3 (for `aniso` divided by the family's scale per
    axis, so that all three terms of s matter).  Origins: a vertex exactly and that vertex moved by +-1, +-2 float32 steps on
    the axis whose step changes s most -- one series over k per aimed vertex, k = 0 being the vertex itself (`face` holds the
    VERTEX index); the rounded point of an edge A .. B (`face` holds the face, k = 0, no series); and, beyond the three kinds
    above, a point BESIDE a vertex in the plane through it -- the vertex plus a vector across the normal of about a third of
    the mesh's size, rounded, then moved by k steps: s of the aimed vertex is then a sum of three full terms that cancel to
    within the rounding of the origin, the near-tie of the sign itself (one series per aimed vertex)."""
    v, f = family(name)
    nr = np.stack([2 * hashed(PLANE_VERTICES + PLANE_EDGES + PLANE_BESIDE, s) - 1 for s in (301, 302, 303)], 1)
    if name == "aniso":
        nr = nr / ANISO
    nr = _f32(nr)
    o, kind, face, ks, series = [], [], [], [], []
    h1, h4 = hashed(PLANE_EDGES, 304), hashed(PLANE_EDGES, 305)
    for i in range(PLANE_VERTICES):
        vi = (i * len(v)) // PLANE_VERTICES
        axis, sign = _touching_axis(nr[i].astype(np.float64), v[vi])
        for k in KS:
            p = v[vi].copy()
            p[axis] = _step(p[axis], -k * sign)                      # s(vertex) = n . (vertex - o): k > 0 puts the vertex above
            o.append(p)
            kind.append(0 if k == 0 else 1)
            face.append(vi)
            ks.append(k)
            series.append(i)
    normals = [nr[i] for i in range(PLANE_VERTICES) for _ in KS]
    for j in range(PLANE_EDGES):
        fi = (j * len(f)) // PLANE_EDGES
        F = _Face(v, f[fi], edge=int(h4[j] * 3))
        o.append(_f32(F.on_edge(h1[j])))
        normals.append(nr[PLANE_VERTICES + j])
        kind.append(2)
        face.append(fi)
        ks.append(0)
        series.append(-1)
    size = v.astype(np.float64).max(0) - v.astype(np.float64).min(0)
    size = np.where(size > 0, size, size.max())
    g = np.stack([2 * hashed(PLANE_BESIDE, s) - 1 for s in (306, 307, 308)], 1) * size
    for i in range(PLANE_BESIDE):
        vi = (i * len(v) + len(v) // 2) // PLANE_BESIDE
        n64 = nr[PLANE_VERTICES + PLANE_EDGES + i].astype(np.float64)
        across = g[i] - n64 * ((n64 @ g[i]) / (n64 @ n64))                 # n . across = 0 up to float64 rounding
        base = _f32(v[vi].astype(np.float64) + 0.3 * across)
        axis, sign = _touching_axis(n64, base)
        for k in KS:
            p = base.copy()
            p[axis] = _step(p[axis], -k * sign)
            o.append(p)
            normals.append(nr[PLANE_VERTICES + PLANE_EDGES + i])
            kind.append(3)
            face.append(vi)
            ks.append(k)
            series.append(PLANE_VERTICES + i)
    o, normals = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(normals, np.float32)
    o.setflags(write=False)
    normals.setflags(write=False)
    return Queries((o, normals), PLANE_KINDS, np.array(kind), np.array(face), np.array(ks), np.array(series))


# ---- exact tables: boxes and triangles --------------------------------------------------------------------------------------
def _boxes_overlap(alo, ahi, blo, bhi):
    """[n, F] bool: the closed float32 boxes [alo, ahi] [n, 3] and [blo, bhi] [F, 3] share a point (comparisons are exact)"""
    return ((alo[:, None, :] <= bhi[None]) & (blo[None] <= ahi[:, None, :])).all(-1)


def _table(near, meets, what):
    """[n, F] bool: meets(i, j) in exact integers for every pair whose bounding boxes share a point.  Two closed sets whose
    boxes are disjoint on a coordinate axis share no point -- an exact float32 comparison, no rounding -- so those pairs are
    False without the call; every 61st of them is evaluated all the same, and must come out False."""
    out = np.zeros(near.shape, bool)
    for i, j in np.argwhere(near):
        out[i, j] = meets(i, j)
    for i, j in np.argwhere(~near)[::61]:
        assert not meets(i, j), f"{what}: pair ({i}, {j}) with disjoint boxes meets"
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tri_table(name):
    """[queries, F] bool by tris_cases.exact_meets on the float32 values as integers; computed once per process"""
    v, f = family(name)
    q = tri_queries(name).data
    V, Q, _ = exact_ints(v, q)
    T, QT = _triangles(V[f]), _triangles(Q)
    tv = v[f]
    near = _boxes_overlap(q.min(1), q.max(1), tv.min(1), tv.max(1))
    return _table(near, lambda i, j: TC.exact_meets(T[j], QT[i]), f"{name}, triangles")


@functools.lru_cache(maxsize=None)
def box_table(name):
    """[queries, F] bool by boxes_cases.exact_meets on the float32 values as integers; computed once per process"""
    v, f = family(name)
    lo, hi = box_queries(name).data
    V, LO, HI, _ = exact_ints(v, lo, hi)
    T, L, H = _triangles(V[f]), _points(LO), _points(HI)
    tv = v[f]
    near = _boxes_overlap(lo, hi, tv.min(1), tv.max(1))
    return _table(near, lambda i, j: BC.exact_meets(L[i], H[i], T[j]), f"{name}, boxes")


def _shares_one_end(ts, qs):
    """two exact spans that are not both single points share exactly one end (they belong to a pair that meets)"""
    if min(ts) == max(ts) and min(qs) == max(qs):
        return False
    return min(qs) >= max(ts) or max(qs) <= min(ts)


def tri_tie(t, q):
    """an EXACT TIE of two integer triangles: they meet, only touching (tris_cases.only_touching), and one of the seventeen
    axes on which they share exactly one end is not an axis on which both spans are single points (on the common normal of a
    coplanar pair everything projects to one point: that alone is no tie)"""
    if not (TC.exact_meets(t, q) and TC.only_touching(t, q)):
        return False
    e = [_sub(t[1], t[0]), _sub(t[2], t[1]), _sub(t[0], t[2])]
    g = [_sub(q[1], q[0]), _sub(q[2], q[1]), _sub(q[0], q[2])]
    nt, nq = _cross(e[0], e[1]), _cross(g[0], g[1])
    axes = [nt, nq] + [_cross(a, b) for a in e for b in g] + [_cross(nt, a) for a in e] + [_cross(nq, b) for b in g]
    return any(L != (0, 0, 0) and _shares_one_end([_dot(L, _sub(x, t[0])) for x in t], [_dot(L, _sub(x, t[0])) for x in q])
               for L in axes)


def box_tie(lo, hi, t):
    """an EXACT TIE of an integer box and an integer triangle: they meet, and on a non-zero axis of the contract (the three box
    axes, the triangle's normal, the nine u_i x e_j) on which not both spans are single points they share exactly one end"""
    if not BC.exact_meets(lo, hi, t):
        return False
    e = [_sub(t[1], t[0]), _sub(t[2], t[1]), _sub(t[0], t[2])]
    units = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    axes = units + [_cross(e[0], e[1])] + [_cross(u, a) for a in e for u in units]
    corners = [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    return any(L != (0, 0, 0) and _shares_one_end([_dot(L, x) for x in t], [_dot(L, x) for x in corners]) for L in axes)


def check_sets(name, sort, got, res=None):
    """got [queries, F] bool (the listed faces of a Result `res`) of family `name`, sort "triangles" / "boxes", against the exact
    table: every pair must agree, but exact ties that disagree, at most LEFT_OUT_CAP of the pairs; with `res`, any and count
    must equal the table too on every query without such a pair.  Returns the number of pairs left out."""
    v, f = family(name)
    Q = tri_queries(name) if sort == "triangles" else box_queries(name)
    want = tri_table(name) if sort == "triangles" else box_table(name)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    left = np.zeros(want.shape, bool)
    if len(bad):
        if sort == "triangles":
            V, D, _ = exact_ints(v, Q.data)
            T, QT = _triangles(V[f]), _triangles(D)
            tie = lambda i, j: tri_tie(T[j], QT[i])                                                  # noqa: E731
        else:
            V, LO, HI, _ = exact_ints(v, *Q.data)
            T, L, H = _triangles(V[f]), _points(LO), _points(HI)
            tie = lambda i, j: box_tie(L[i], H[i], T[j])                                             # noqa: E731
        for i, j in bad:
            assert want[i, j] and tie(i, j), (
                f"{name}, {sort}, {Q.kinds[Q.kind[i]]}: query {i} (aimed at face {Q.face[i]}, k = {Q.k[i]}) and face {j}: "
                f"the exact reference says {'meets' if want[i, j] else 'apart'}, and this is no exact tie ({len(bad)} pairs differ)")
            left[i, j] = True
    assert left.sum() <= LEFT_OUT_CAP * want.size, f"{name}, {sort}: {left.sum()} of {want.size} pairs are exact ties that disagree"
    if res is not None:
        clean = ~left.any(1)
        assert np.array_equal(res.count[clean], want.sum(1)[clean]), f"{name}, {sort}: count"
        assert np.array_equal(res.any[clean], want.any(1)[clean]), f"{name}, {sort}: any"
    return int(left.sum())


def aimed(name, sort):
    """[queries] bool: the exact answer of every query against the face it aims at"""
    Q = tri_queries(name) if sort == "triangles" else box_queries(name)
    want = tri_table(name) if sort == "triangles" else box_table(name)
    return want[np.arange(len(Q.face)), Q.face]


def check_inputs(name, sort):
    """the conditions on the generated queries of a family (boxes, triangles): every query valid under its contract (triangles:
    with area as well), per kind MEET_SHARE of the aimed pairs meet and a series flips between k = -2 and k = +2, and on `flat`
    every aimed pair of triangles is exactly coplanar.  Returns {kind: (aimed pairs, of which meet, series that flip)}"""
    v, f = family(name)
    Q = tri_queries(name) if sort == "triangles" else box_queries(name)
    met = aimed(name, sort)
    if sort == "triangles":
        assert Q.data.dtype == np.float32 and np.isfinite(Q.data).all(), f"{name}: an invalid triangle"
        V, D, _ = exact_ints(v, Q.data)
        T, QT = _triangles(V[f]), _triangles(D)
        assert all(TC._normal(q) != (0, 0, 0) for q in QT), f"{name}: a query triangle without area"
        if name == "flat":
            assert all(TC.coplanar(T[j], QT[i]) for i, j in enumerate(Q.face)), "flat: an aimed pair is not coplanar"
    else:
        lo, hi = Q.data
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all(), f"{name}: an invalid box"
    stats = {}
    for kd, label in enumerate(Q.kinds):
        rows = Q.kind == kd
        assert rows.any(), f"{name}, {sort}: no query of the kind {label}"
        share = met[rows].mean()
        first = met[rows & (Q.k == KS[0])]
        last = met[rows & (Q.k == KS[-1])]
        assert np.array_equal(Q.series[rows & (Q.k == KS[0])], Q.series[rows & (Q.k == KS[-1])])
        flips = int((first != last).sum())
        assert MEET_SHARE[0] <= share <= MEET_SHARE[1], f"{name}, {sort}, {label}: {share:.0%} of the aimed pairs meet"
        assert flips >= 1, f"{name}, {sort}, {label}: no series flips between k = -2 and k = +2"
        stats[label] = (int(rows.sum()), int(met[rows].sum()), flips)
    return stats


# ---- the exact reference of the plane queries -------------------------------------------------------------------------------
# meets, cut [n, F] bool; decisive [n, F] bool: all three vertices pass the bound; sign int [n, nv]; rows: {(plane, face):
# ((kind, point) for p0, (kind, point) for p1)} for every cut face -- kind "vertex": point = its index, kind "crossing":
# point = (three Fractions of the exact point, the vertex indices (u, w), well_conditioned)
PlanesReference = collections.namedtuple("PlanesReference", "meets cut decisive sign rows")


@functools.lru_cache(maxsize=None)
def planes_reference(name):
    """The contract of csrc/tr_planes.h restated in exact arithmetic on the float32 values: s = n . (v - o) as an integer (in
    units of 2^(ev + en)); pos / neg / zero per face; the two ends of a cut face by the contract's walk 0 -> 1 -> 2 -> 0 --
    p0 where it enters the positive arc, p1 where it leaves it; a vertex with s = 0 is the end itself, otherwise the end is
    u + s(u) / (s(u) - s(w)) (w - u), u the negative and w the positive vertex, in fractions.Fraction.  The direction of every
    row is checked here: (face normal x plane normal) . (p1 - p0) > 0, exactly."""
    v, f = family(name)
    o, nr = plane_queries(name).data
    V, O, ev = exact_ints(v, o)
    N, _ = exact_ints(nr)
    assert all(any(k != 0 for k in row) for row in N.tolist()), f"{name}: a zero normal"
    D = V[None, :, :] - O[:, None, :]                                            # [n, nv, 3] integers
    terms = N[:, None, :] * D
    S = terms.sum(-1)                                                            # [n, nv]
    bound = np.abs(terms).sum(-1)
    sign = np.array([[(x > 0) - (x < 0) for x in row] for row in S.tolist()], np.int8)
    firm = np.array([[x == 0 or abs(x) << 51 >= b for x, b in zip(rs, rb)] for rs, rb in zip(S.tolist(), bound.tolist())])
    sf = sign[:, f]                                                              # [n, F, 3]
    pos, neg, zero = (sf > 0).sum(-1), (sf < 0).sum(-1), (sf == 0).sum(-1)
    meets = ~((pos == 3) | (neg == 3))
    cut = (pos >= 1) & ((neg >= 1) | (zero == 2))
    decisive = firm[:, f].all(-1)
    scale = Fraction(2) ** ev
    rows = {}
    Vp, Np = _points(V), _points(N)
    for i, j in np.argwhere(cut):
        idx = [int(x) for x in f[j]]
        s = [S[i, x] for x in idx]
        enter = next(e for e in range(3) if not s[e] > 0 and s[(e + 1) % 3] > 0)
        leave = next(e for e in range(3) if s[e] > 0 and not s[(e + 1) % 3] > 0)
        ends, exact = [], []
        for a, b in ((enter, (enter + 1) % 3), ((leave + 1) % 3, leave)):        # a: s <= 0, b: s > 0
            if s[a] == 0:
                ends.append(("vertex", idx[a]))
                exact.append(tuple(Fraction(c) for c in Vp[idx[a]]))
            else:
                u, w = Vp[idx[a]], Vp[idx[b]]
                t = Fraction(s[a], s[a] - s[b])
                p = tuple(u[k] + t * (w[k] - u[k]) for k in range(3))
                well = sum(abs(Np[i][k] * (w[k] - u[k])) for k in range(3)) <= (abs(s[a] - s[b]) << 16)
                ends.append(("crossing", (tuple(c * scale for c in p), (idx[a], idx[b]), well)))
                exact.append(p)
        normal = _cross(_sub(Vp[idx[1]], Vp[idx[0]]), _sub(Vp[idx[2]], Vp[idx[0]]))
        assert _dot(_cross(normal, Np[i]), _sub(exact[1], exact[0])) > 0, f"{name}: plane {i}, face {j}: the direction of the row"
        rows[(int(i), int(j))] = tuple(ends)
    for a in (meets, cut, decisive, sign):
        a.setflags(write=False)
    return PlanesReference(meets, cut, decisive, sign, rows)


def check_plane_inputs(name):
    """the conditions on the generated planes of a family: every plane valid; in every series the exact s of the aimed vertex
    (0 where the origin is the vertex itself) flips its sign between k = -2 and k = +2 -- with it the class of every face around that vertex --
    and between MEET_SHARE of those values are positive; every edge origin leaves the two ends of its edge strictly on either
    side.  Returns {kind: (queries, aimed values > 0, aimed values == 0)}"""
    Q = plane_queries(name)
    o, nr = Q.data
    ref = planes_reference(name)
    v, f = family(name)
    assert np.isfinite(o).all() and np.isfinite(nr).all() and (nr != 0).any(1).all(), f"{name}: an invalid plane"
    series = Q.series >= 0
    at = ref.sign[np.arange(len(o)), np.where(series, Q.face, 0)]
    assert (at[Q.kind == 0] == 0).all(), f"{name}: a plane through a vertex does not hold it"
    for kd in range(len(Q.kinds)):
        assert (Q.kind == kd).any()
    for s in np.unique(Q.series[series]):
        rows = Q.series == s
        assert at[rows & (Q.k == -2)][0] * at[rows & (Q.k == 2)][0] == -1, f"{name}: series {s} of planes does not flip"
    share = (at[series] > 0).mean()
    assert MEET_SHARE[0] <= share <= MEET_SHARE[1], f"{name}: {share:.0%} of the aimed vertices are above their plane"
    edges = Q.kind == 2
    assert edges.sum() == PLANE_EDGES
    for i in np.flatnonzero(edges):
        around = ref.sign[i, f[Q.face[i]]]
        assert (around > 0).any() and (around < 0).any() and ref.cut[i, Q.face[i]], f"{name}: plane {i} does not cross its edge"
    return {Q.kinds[kd]: (int((Q.kind == kd).sum()), int((at[(Q.kind == kd) & series] > 0).sum()),
                          int((at[(Q.kind == kd) & series] == 0).sum())) for kd in range(len(Q.kinds))}


def check_planes(name, met, cut, listed):
    """met, cut: planes_sim.Result (cut with segments) of family `name`; listed(res, n, F) -> [n, F] bool.  Against the exact
    reference: both tables on every decisive pair (the others at most LEFT_OUT_CAP); an end that is a vertex by its bits; an end
    that is a crossing within ONE float32 step of the exact rational point in every coordinate, the step taken at
    max(|u_k|, |w_k|), on every well-conditioned edge (rows with another at most ILL_CONDITIONED_CAP).
    WHY ONE STEP: the contract keeps the float64 value within 2^-51 relative of the interval of u_k and w_k, the conversion adds
    at most half a step, and the error of t adds at most |w_k - u_k| 2^-33 on edges with sum |n_k| |w_k - u_k| <=
    2^16 |s(u) - s(w)| -- far below a step.  Returns (pairs left out, rows on ill-conditioned edges, rows compared, the largest
    error of a crossing in steps)"""
    v, f = family(name)
    ref = planes_reference(name)
    n = len(ref.meets)
    left = ~ref.decisive
    assert left.sum() <= LEFT_OUT_CAP * left.size, f"{name}, planes: {left.sum()} of {left.size} pairs are below the bound"
    for res, want, what in ((met, ref.meets, "meets"), (cut, ref.cut, "cut")):
        got = listed(res, n, len(f))
        bad = np.argwhere((got != want) & ~left)
        assert len(bad) == 0, (f"{name}, planes, {what}: {len(bad)} decisive pairs differ from the exact signs, the first "
                               f"(plane, face) {bad[:4].tolist()}")
        clean = ~left.any(1)
        assert np.array_equal(res.count[clean], want.sum(1)[clean]) and np.array_equal(res.any[clean], want.any(1)[clean]), f"{name}, {what}"
    seg = cut.segments
    assert seg is not None and seg.shape == (len(cut.faces), 2, 3)
    plane = np.repeat(np.arange(n), cut.count)
    worst, compared, ill = Fraction(0), 0, 0
    for r, (i, j) in enumerate(zip(plane.tolist(), cut.faces.tolist())):
        if left[i, j] or not ref.cut[i, j]:
            continue
        ends = ref.rows[(i, j)]
        if any(kind == "crossing" and not point[2] for kind, point in ends):
            ill += 1
            continue
        compared += 1
        for e, (kind, point) in enumerate(ends):
            if kind == "vertex":
                assert np.array_equal(seg[r, e].view(np.uint32), v[point].view(np.uint32)), (
                    f"{name}: plane {i}, face {j}, end {e}: not the bits of vertex {point}")
                continue
            exact, (u, w), _ = point
            for k in range(3):
                step = Fraction(float(np.spacing(np.float32(max(abs(v[u, k]), abs(v[w, k]))))))
                err = abs(Fraction(float(seg[r, e, k])) - exact[k]) / step
                worst = max(worst, err)
                assert err <= 1, (f"{name}: plane {i}, face {j}, end {e}, coordinate {k}: {float(err):.3f} float32 steps from the "
                                  f"exact crossing of the edge ({u}, {w})")
    assert compared > 0 and ill <= ILL_CONDITIONED_CAP * max(1, ill + compared), f"{name}: {ill} of {ill + compared} rows on ill-conditioned edges"
    return int(left.sum()), ill, compared, float(worst)
