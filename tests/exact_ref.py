"""The hit predicate in exact integer arithmetic (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

Float32 values are dyadic rationals: scaled by a power of two they are integers, and every quantity of the hit
predicate -- a polynomial in the inputs -- can be evaluated without any rounding.  This module restates the predicate
from the PROSE of csrc/tr_math.h (the comment blocks "the EXACT part of the contract" and "exact ties"), sharing no
code with csrc/, oracle/ or tests/host_sim/:

    kz         = the dominant axis of the direction, the first of equals; (kx, ky, kz) cyclic
    P'         = P - o;   Ph = (P'x dz - dx P'z,  P'y dz - dy P'z)               (permuted components)
    U, V, W    = chx bhy - chy bhx,  ahx chy - ahy chx,  bhx ahy - bhy ahx      (weights of a, b, c)
    det        = U + V + W;  inside  <=>  no two of U, V, W have strictly opposite signs, and det != 0
    t          = (U Az + V Bz + W Cz) / (det dz),  accepted iff 0 <= t <= 1e7   (the corpora below keep every t far
                 below 1e7 -- directions are as long as the distances they span -- so only 0 <= t is evaluated)
    tie code   = bits 0-2: U, V, W is zero; bit 3: det < 0;  0 = no tie
    owner      = a zero function's edge (U: b -> c, V: c -> a, W: a -> b) seen along the ray,
                 e = ((qx - px) dz - dx (qz - pz), (qy - py) dz - dy (qz - pz)), s = the sign of det;
                 the triangle owns the edge iff  s ey > 0  or  (s ey == 0 and s ex > 0)
    hit        <=> inside, t accepted, and every zero edge owned
    front      = d . ((b - a) x (c - a)) < 0;   uv = (U / det, V / det)

Two engines evaluate one set of formulas (_core): every ray against every triangle in numpy int64 (lattice(): integer
scenes whose magnitudes are asserted small enough that nothing overflows), and listed (ray, triangle) pairs in Python
integers through numpy object arrays (pairs(): any float32 input).

The band of pairs() -- how far below zero an EXACT edge function of a triangle may lie when the contract's float64
arithmetic (tr_woop64_xyz) still calls it inside -- is counted from that function's source text.  U is
fl(fl(chx bhy) - fl(chy bhx)).  Where every P' = P - o is exact in float64 and has at most 29 significant bits
(band_applies() checks that exactly) a product P' d is exact (29 + 24 bits), so a component of Ph carries ONE
rounding, the fma's; each of the two products of U carries one more.  That is three relative roundings of
u = 2^-53 per product: |U_computed - U_exact| <= 3 u (|chx bhy| + |chy bhx|) to first order.  BAND_K is that count
DOUBLED = 6, which also covers the rounding of the final subtraction (at most u times the same sum) and every
second-order term.  Hence: the float64 function >= 0 implies the exact one >= -BAND_K u (|chx bhy| + |chy bhx|), and a
hit whose exact edge functions, normalised to det > 0, lie below that is a wrong answer, not a rounded one.
"""
import functools
from fractions import Fraction

import numpy as np

BAND_K = 6
LATTICE_MAX = 1 << 11        # every |P - o| and |d| of a lattice scene is below it: Ph < 2^23, U < 2^47, t's numerator < 2^61


# ---- the formulas, once, on arrays of int64 or of Python integers -----------------------------------------------------
def _sign(x):
    return (x > 0).astype(np.int8) - (x < 0).astype(np.int8)


def _own(s, ex, ey):
    ex, ey = s * ex, s * ey
    return (ey > 0) | ((ey == 0) & (ex > 0))


def _core(ah, bh, ch, az, bz, cz, dz, eu, ev, ew):
    """ah, bh, ch: (x, y) of Ph of the three vertices; az..cz: P'z; dz: d[kz]; eu, ev, ew: (x, y) of the directed
    edges b -> c, c -> a, a -> b seen along the ray.  Everything broadcastable; exact."""
    U = ch[0] * bh[1] - ch[1] * bh[0]
    V = ah[0] * ch[1] - ah[1] * ch[0]
    W = bh[0] * ah[1] - bh[1] * ah[0]
    det = U + V + W
    sU, sV, sW, sdet = _sign(U), _sign(V), _sign(W), _sign(det)
    neg = (sU < 0) | (sV < 0) | (sW < 0)
    pos = (sU > 0) | (sV > 0) | (sW > 0)
    inside = ~(neg & pos) & (sdet != 0)
    tn = U * az + V * bz + W * cz
    td = det * dz
    st = _sign(tn) * _sign(td)                       # the exact sign of t (0: the origin lies in the triangle's plane)
    z = (sU == 0).astype(np.int8) | ((sV == 0).astype(np.int8) << 1) | ((sW == 0).astype(np.int8) << 2)
    code = np.where(z != 0, z | ((sdet < 0).astype(np.int8) << 3), 0).astype(np.int8)
    s = np.where(sdet < 0, -1, 1)
    own = (_own(s, *eu), _own(s, *ev), _own(s, *ew))
    owned = ((sU != 0) | own[0]) & ((sV != 0) | own[1]) & ((sW != 0) | own[2])
    return dict(U=U, V=V, W=W, det=det, sU=sU, sV=sV, sW=sW, sdet=sdet, inside=inside, tn=tn, td=td, st=st, code=code,
                own=own, owned=owned, hit=inside & (st >= 0) & owned)


def _axes(d):
    """per ray (kx, ky, kz): kz the dominant axis of the direction, the first of equals"""
    a = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    m = a[:, 0].copy()
    g = a[:, 1] > m
    kz[g] = 1
    m[g] = a[g, 1]
    kz[a[:, 2] > m] = 2
    return np.stack([(kz + 1) % 3, (kz + 2) % 3, kz], 1)


# ---- lattice scenes: every ray against every triangle, int64 ------------------------------------------------------------
class Ideal:
    """what the ideal rule says per ray: count [n], sets (a list of arrays of face ids), nearest [n] (-1: none; the
    smaller face id on exactly equal t), alt [n] (the runner-up where its exact t differs from the nearest's by less
    than 2^-20 relative without being equal, else -1), tie [n] (some triangle is met within [0, tmax] through an edge
    or a vertex), border [n] (... through an edge that has no second triangle: the rim of an open patch), front / uv
    of the nearest, and codes: how often each tie code occurred among such triangles (codes[7]: rays in a triangle's
    own plane)"""


def lattice(v, f, o, d, chunk=1 << 21):
    v, f = np.asarray(v), np.asarray(f, np.int64)
    o, d = np.asarray(o), np.asarray(d)
    for x in (v, o, d):
        assert np.array_equal(x, np.rint(x)), "lattice scenes are integers"
    vi, oi, di = v.astype(np.int64), o.astype(np.int64), d.astype(np.int64)
    n, nf = len(oi), len(f)
    assert np.abs(di).max() < LATTICE_MAX and np.abs(di).max(1).min() >= 1
    for k in range(3):
        assert max(abs(int(vi[:, k].max()) - int(oi[:, k].min())), abs(int(oi[:, k].max()) - int(vi[:, k].min()))) < LATTICE_MAX
    ax = _axes(di)
    out = Ideal()
    out.count = np.zeros(n, np.int32)
    out.nearest = np.full(n, -1, np.int32)
    out.alt = np.full(n, -1, np.int32)
    out.tie = np.zeros(n, bool)
    out.front = np.zeros(n, bool)
    out.uv = np.zeros((n, 2), np.float64)
    out.sets = [None] * n
    out.codes = np.zeros(16, np.int64)
    out.border = np.zeros(n, bool)
    # edges with one triangle only (an open patch): [F, 3] in the order of U, V, W = b -> c, c -> a, a -> b
    und = np.sort(np.stack([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], 1), 2)                   # [F, 3, 2]
    _, inv, cnt = np.unique(und.reshape(-1, 2), axis=0, return_inverse=True, return_counts=True)
    bnd = (cnt[inv.reshape(-1)] == 1).reshape(nf, 3)
    step = max(1, chunk // max(nf, 1))
    for kz in range(3):
        perm = [(kz + 1) % 3, (kz + 2) % 3, kz]
        rays = np.flatnonzero(ax[:, 2] == kz)
        P = vi[:, perm]
        E = [P[f[:, q]] - P[f[:, p]] for p, q in ((1, 2), (2, 0), (0, 1))]      # b -> c, c -> a, a -> b   [F, 3]
        for lo in range(0, len(rays), step):
            r = rays[lo:lo + step]
            O, D = oi[r][:, perm], di[r][:, perm]
            dx, dy, dz = D[:, 0:1], D[:, 1:2], D[:, 2:3]
            Pp = P[None, :, :] - O[:, None, :]                                  # [n, V, 3]
            phx = Pp[..., 0] * dz - dx * Pp[..., 2]
            phy = Pp[..., 1] * dz - dy * Pp[..., 2]
            pz = Pp[..., 2]
            g = [f[:, k] for k in range(3)]
            e = [(x[None, :, 0] * dz - dx * x[None, :, 2], x[None, :, 1] * dz - dy * x[None, :, 2]) for x in E]
            c = _core(*[(phx[:, k], phy[:, k]) for k in g], *[pz[:, k] for k in g], dz, *e)
            met = c["inside"] & (c["st"] >= 0)                                  # (t <= tmax: t < 2^12 on a lattice scene)
            out.codes += np.bincount(c["code"][met].astype(np.int64), minlength=16)
            # a ray in the triangle's own plane: U = V = W = 0, no orientation, never a hit
            out.codes[7] += int(np.count_nonzero((c["sU"] == 0) & (c["sV"] == 0) & (c["sW"] == 0)))
            out.tie[r] = (met & (c["code"] != 0)).any(1)
            out.border[r] = (met & (((c["sU"] == 0) & bnd[None, :, 0]) | ((c["sV"] == 0) & bnd[None, :, 1]) |
                                    ((c["sW"] == 0) & bnd[None, :, 2]))).any(1)
            hit = c["hit"]
            out.count[r] = hit.sum(1)
            ri, fi = np.nonzero(hit)
            tn, td = c["tn"][ri, fi], c["td"][ri, fi]
            U, V, det = c["U"][ri, fi], c["V"][ri, fi], c["det"][ri, fi]
            bounds = np.searchsorted(ri, np.arange(len(r) + 1))
            for j in range(len(r)):
                a, b = bounds[j], bounds[j + 1]
                out.sets[r[j]] = fi[a:b].astype(np.int32)
                if a == b:
                    continue
                ts = sorted((Fraction(int(tn[k]), int(td[k])), int(fi[k]), k) for k in range(a, b))
                t0, f0, k0 = ts[0]
                out.nearest[r[j]] = f0
                out.uv[r[j]] = (int(U[k0]) / int(det[k0]), int(V[k0]) / int(det[k0]))
                for t1, f1, _ in ts[1:]:
                    if t1 != t0:
                        if (t1 - t0) * (1 << 20) < t1:
                            out.alt[r[j]] = f1
                        break
    a, b, c3 = (vi[f[:, k]] for k in range(3))
    nrm = np.cross(b - a, c3 - a)
    hitr = out.nearest >= 0
    out.front[hitr] = (di[hitr] * nrm[out.nearest[hitr]]).sum(1) < 0
    return out


def axis_parity(v, f, p2):
    """inside / outside of the closed integer surface (v, f) for the points p2 / 2 (p2 integer, [n, 3]): the parity of
    the ideal crossings of the ray from the point along +x -- in doubled coordinates, so that half-integer points are
    integers too.  Points on the surface have no answer: the caller leaves them out (on_surface)."""
    ideal = lattice(np.asarray(v) * 2, f, p2, np.tile(np.array([1, 0, 0]), (len(p2), 1)))
    return ideal.count % 2 == 1


def on_surface(v, f, p2):
    """which of the points p2 / 2 lie on a triangle of the integer mesh (exact)"""
    v2, f = np.asarray(v).astype(np.int64) * 2, np.asarray(f, np.int64)
    p2 = np.asarray(p2).astype(np.int64)
    a, b, c = (v2[f[:, k]][None] - p2[:, None, :] for k in range(3))      # [n, F, 3]
    nrm = np.cross(b - a, c - a)
    coplanar = (a * nrm).sum(-1) == 0
    # inside or on the border: the three sub-triangle normals (p, x, y) all point along nrm (or vanish)
    s = [(np.cross(x, y) * nrm).sum(-1) for x, y in ((a, b), (b, c), (c, a))]
    return (coplanar & (s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)).any(1)


# ---- any float32 input: listed (ray, triangle) pairs in Python integers ---------------------------------------------------
def _ints(x):
    """float array -> (object array of Python integers, shift): x == ints / 2^shift exactly"""
    flat = [float(t).as_integer_ratio() for t in np.asarray(x, np.float64).ravel()]
    shift = max(q.bit_length() for _, q in flat) - 1
    full = 1 << shift
    return np.array([p * (full // q) for p, q in flat], dtype=object).reshape(np.shape(x)), shift


def _take(x, perm):
    return x[np.arange(len(x))[:, None], perm]


def pairs(v, f, o, d, tri):
    """exact quantities of (ray i, triangle tri[i]) for float32 inputs: the dict of _core (object arrays / int8 signs)
    plus mag = (|p1| + |p2|) of the two products of U, V, W -- the comparison  X >= -band  is made in integers as
    X 2^53 >= -BAND_K (|p1| + |p2|)  (above_band) -- and pre: the precondition of BAND_K holds for this pair (every P - o
    of its three vertices has at most 29 significant bits)"""
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int64)
    o, d, tri = np.asarray(o, np.float32), np.asarray(d, np.float32), np.asarray(tri, np.int64)
    perm = _axes(d.astype(np.float64))
    allp, _ = _ints(np.concatenate([v.ravel(), o.ravel()]))
    vi, oi = allp[:v.size].reshape(-1, 3), allp[v.size:].reshape(-1, 3)
    di, _ = _ints(d)
    O, D = _take(oi, perm), _take(di, perm)
    A, B, C = (_take(vi[f[tri, k]], perm) - O for k in range(3))
    dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]

    def ph(P):
        return P[:, 0] * dz - dx * P[:, 2], P[:, 1] * dz - dy * P[:, 2]
    ah, bh, ch = ph(A), ph(B), ph(C)
    e = [ph(q - p) for p, q in ((B, C), (C, A), (A, B))]
    c = _core(ah, bh, ch, A[:, 2], B[:, 2], C[:, 2], dz, *e)
    ab = lambda x: np.array([abs(t) for t in x], dtype=object)  # noqa: E731
    c["pre"] = np.array([all(_sigbits(x) <= 29 for x in row) for row in np.concatenate([A, B, C], 1)], bool)
    c["mag"] = (ab(ch[0] * bh[1]) + ab(ch[1] * bh[0]), ab(ah[0] * ch[1]) + ab(ah[1] * ch[0]),
                ab(bh[0] * ah[1]) + ab(bh[1] * ah[0]))
    return c


def _sigbits(x):
    x = abs(int(x))
    return (x >> ((x & -x).bit_length() - 1)).bit_length() if x else 0


def above_band(c):
    """per pair: every exact edge function, normalised to det > 0, is >= -BAND_K 2^-53 (|p1| + |p2|)"""
    s = np.where(c["sdet"] < 0, -1, 1).astype(object)
    ok = np.ones(len(s), bool)
    for X, m in zip((c["U"], c["V"], c["W"]), c["mag"]):
        ok &= ((s * X) * (1 << 53) >= -(BAND_K * m)).astype(bool)
    return ok


def in_band(c, k):
    """per pair: edge function k (0, 1, 2 = U, V, W) is not zero but within its band"""
    X, m = (c["U"], c["V"], c["W"])[k], c["mag"][k]
    return (np.array([abs(t) for t in X], dtype=object) * (1 << 53) <= BAND_K * m).astype(bool) & ((c["sU"], c["sV"], c["sW"])[k] != 0)


def band_applies(v, o):
    """the precondition of BAND_K: every P - o (all vertices, the one origin o) is exact in float64 and has at most 29
    significant bits, so that its products with a float32 direction are exact in float64"""
    vi, _ = _ints(np.concatenate([np.asarray(v, np.float32).ravel(), np.asarray(o, np.float32).ravel()]))
    P, O = vi[:-3].reshape(-1, 3), vi[-3:]
    return all(_sigbits(x) <= 29 for x in (P - O[None, :]).ravel())


def star_shaped(v, f, o):
    """True when (v, f) is a closed, connected, consistently wound surface and every triangle's exact
    det[a - o, b - o, c - o] is non-zero with one and the same sign: seen from o every triangle shows the same side,
    the central projection onto a sphere around o is a covering of degree one, and EVERY ray from o crosses the surface
    exactly once."""
    f = np.asarray(f, np.int64)
    half = {}
    for t, (a, b, c) in enumerate(f.tolist()):
        for p, q in ((a, b), (b, c), (c, a)):
            if (p, q) in half:
                return False
            half[(p, q)] = t
    if any((q, p) not in half for p, q in half):
        return False
    seen, todo = {0}, [0]
    while todo:
        a, b, c = f[todo.pop()].tolist()
        for p, q in ((a, b), (b, c), (c, a)):
            t = half[(q, p)]
            if t not in seen:
                seen.add(t)
                todo.append(t)
    if len(seen) != len(f):
        return False
    vi, _ = _ints(np.concatenate([np.asarray(v, np.float32).ravel(), np.asarray(o, np.float32).ravel()]))
    P = vi[:-3].reshape(-1, 3) - vi[-3:][None, :]
    signs = set()
    for a, b, c in f.tolist():
        A, B, Cc = P[a], P[b], P[c]
        det = (A[0] * (B[1] * Cc[2] - B[2] * Cc[1]) - A[1] * (B[0] * Cc[2] - B[2] * Cc[0]) + A[2] * (B[0] * Cc[1] - B[1] * Cc[0]))
        signs.add((det > 0) - (det < 0))
    return len(signs) == 1 and 0 not in signs


# ---- corpus (a): lattice scenes -------------------------------------------------------------------------------------------
def _quads_to_mesh(quads, rng):
    """quads [Q, 4, 3] integer corners in order -> (v, f): shared vertices, a random diagonal and a random winding each"""
    index, verts, faces = {}, [], []

    def vid(p):
        p = tuple(int(x) for x in p)
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]
    for q in quads:
        a, b, c, d = (vid(p) for p in q)
        two = [(a, b, c), (a, c, d)] if rng.random() < 0.5 else [(a, b, d), (b, c, d)]
        for t in two:
            faces.append(t if rng.random() < 0.5 else (t[0], t[2], t[1]))
    return np.array(verts, np.float32), np.array(faces, np.int32)


def _cube_quads(lo, n, q):
    """the 6 n^2 quads of the surface of the cube [lo, lo + n q]^3"""
    g = np.arange(n + 1) * q
    out = []
    for axis in range(3):
        for side in (0, n * q):
            for i in range(n):
                for j in range(n):
                    c4 = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis] = side
                        p[(axis + 1) % 3] = g[i + di]
                        p[(axis + 2) % 3] = g[j + dj]
                        c4.append([p[k] + lo[k] for k in range(3)])
                    out.append(c4)
    return out


def _lattice_dirs(v, f, o, rng, nrand):
    tri = v[f].astype(np.int64)
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    vi = v.astype(np.int64)
    o = np.asarray(o, np.int64)
    d = np.concatenate([vi - o, vi[edges[:, 0]] + vi[edges[:, 1]] - 2 * o, tri.sum(1) - 3 * o,
                        rng.integers(-9, 10, (nrand, 3)), np.eye(3, dtype=np.int64)])
    d = d[np.abs(d).max(1) > 0]
    return np.concatenate([d, -d])


def _lattice_scene(name, v, f, origins, seed):
    rng = np.random.default_rng(seed)
    nrand = min(200, 4 + len(f))
    os_, ds, which = [], [], []
    for k, o in enumerate(origins):
        d = _lattice_dirs(v, f, o, rng, nrand)
        os_.append(np.tile(np.asarray(o, np.float32), (len(d), 1)))
        ds.append(d.astype(np.float32))
        which.append(np.full(len(d), k))
    return dict(name=name, v=v, f=f, o=np.concatenate(os_), d=np.concatenate(ds), origin_of=np.concatenate(which),
                origins=np.asarray(origins, np.float32), closed=True)


@functools.lru_cache(maxsize=None)
def lattice_scenes():
    """corpus (a): integer vertices, origins and directions with |P - o|, |d| < 2^11 -- the contract's float64 part is
    exact, so the contract must EQUAL the ideal rule.  Origins per scene: two strictly inside, one outside but too close
    to be anchored, one far outside (anchored)."""
    out = []
    for n, q in ((1, 40), (2, 20), (5, 8), (8, 5)):
        v, f = _quads_to_mesh(_cube_quads((0, 0, 0), n, q), np.random.default_rng(100 + n))
        out.append(_lattice_scene(f"cube{n}", v, f, [(20, 20, 20), (7, 31, 12), (47, 13, 22), (600, 37, -11)], 200 + n))
    quads = _cube_quads((0, 0, 0), 4, 12) + _cube_quads((8, 8, 8), 4, 8) + _cube_quads((16, 16, 16), 4, 4)
    v, f = _quads_to_mesh(quads, np.random.default_rng(110))
    out.append(_lattice_scene("nested3", v, f, [(24, 24, 24), (21, 26, 23), (55, 20, 30), (-560, 24, 70)], 210))
    # an open patch: 16 x 16 cells of integer heights; half-open at its boundary
    rng = np.random.default_rng(120)
    h = rng.integers(0, 7, (17, 17))
    quads = [[(i + a, j + b, int(h[i + a, j + b])) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))] for i in range(16) for j in range(16)]
    v, f = _quads_to_mesh(quads, rng)
    s = _lattice_scene("heightfield", v, f, [(8, 8, 3), (5, 11, 2), (2, 13, 5), (7, 9, 600)], 220)
    s["closed"] = False
    out.append(s)
    for N in (3, 8, 64):
        ang = 2 * np.pi * np.arange(N) / N
        ring = np.stack([np.rint(100 * np.cos(ang)), np.rint(100 * np.sin(ang)), np.zeros(N)], 1)
        v = np.concatenate([ring, [[0, 0, 7], [0, 0, -7]]]).astype(np.float32)
        rng = np.random.default_rng(130 + N)
        f = []
        for i in range(N):
            j = (i + 1) % N
            for t in ((i, j, N), (j, i, N + 1)):
                f.append(t if rng.random() < 0.5 else (t[0], t[2], t[1]))
        out.append(_lattice_scene(f"fan{N}", v, np.array(f, np.int32), [(0, 0, 0), (3, -2, 1), (140, 60, 5), (30, -600, 40)], 230 + N))
    return out


@functools.lru_cache(maxsize=None)
def lattice_ideal(name):
    s = next(s for s in lattice_scenes() if s["name"] == name)
    return lattice(s["v"], s["f"], s["o"], s["d"])


def lattice_points(s):
    """integer points and points at odd multiples of 1/2 in and around a closed lattice scene, those on the surface
    left out: (points float32 [n, 3], inside [n] by axis_parity)"""
    rng = np.random.default_rng(len(s["f"]))
    lo, hi = s["v"].min(0).astype(np.int64), s["v"].max(0).astype(np.int64)
    p_int = rng.integers(lo - 2, hi + 3, (700, 3)) * 2
    p_half = rng.integers(lo - 2, hi + 2, (700, 3)) * 2 + 1
    vi = s["v"].astype(np.int64)
    near = np.concatenate([vi[rng.integers(0, len(vi), 300)] * 2 + rng.integers(-1, 2, (300, 3)) * c for c in (1, 2)])
    p2 = np.concatenate([p_int, p_half, near])
    p2 = p2[~on_surface(s["v"], s["f"], p2)]
    return (p2 / 2).astype(np.float32), axis_parity(s["v"], s["f"], p2)


# ---- corpus (b): near-degenerate scenes -----------------------------------------------------------------------------------
def _fan(N, hexp, centre, scale):
    ang = 2 * np.pi * np.arange(N) / N
    c = np.asarray(centre, np.float64)
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(N)], 1) + c
    h = 2.0 ** hexp
    v = (np.concatenate([ring, [c + [0, 0, h], c - [0, 0, h]]]).astype(np.float32) * np.float32(scale)).astype(np.float32)
    f = []
    for i in range(N):
        j = (i + 1) % N
        f += [(i, j, N), (j, i, N + 1)]
    return v, np.array(f, np.int32), (np.asarray(centre, np.float32) * np.float32(scale)).astype(np.float32)


def _unimodular(rng):
    """a 3 x 3 integer matrix of determinant 1 ... 17 with entries below 2^22: row additions on diag(1, 1, k)"""
    while True:
        k = int(rng.integers(1, 18))
        M = np.diag([1, 1, k]).astype(object)
        for _ in range(int(rng.integers(8, 15))):
            i, j = rng.choice(3, 2, replace=False)
            m = int(rng.integers(-9, 10))
            if rng.random() < 0.5:
                M[i] = M[i] + m * M[j]
            else:
                M[:, i] = M[:, i] + m * M[:, j]
            if max(abs(int(x)) for x in M.ravel()) >= 1 << 22:
                break
        big = max(abs(int(x)) for x in M.ravel())
        if 1 << 12 <= big < 1 << 22:
            return np.array(M.tolist(), np.float64)


def _tetra(rng):
    M = _unimodular(rng)
    v = (2 * np.concatenate([M, [-M.sum(0)]])).astype(np.float32)      # doubled: every edge midpoint is an integer point
    f = np.array([(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)], np.int32)
    return v, f, np.zeros(3, np.float32)


def _tube():
    """a strip of needle triangles (aspect 10^4) closed into a 12-sided tube with end caps; everything on a 2^-10 grid"""
    M, L = 12, 5000.0
    ang = 2 * np.pi * np.arange(M) / M
    ring = np.stack([np.zeros(M), np.rint(np.cos(ang) * 1024) / 1024, np.rint(np.sin(ang) * 1024) / 1024], 1)
    v = np.concatenate([ring, ring + [L, 0, 0], [[0, 0, 0], [L, 0, 0]]]).astype(np.float32)
    f = []
    for i in range(M):
        j = (i + 1) % M
        f += [(i, j, M + i), (j, M + j, M + i), (j, i, 2 * M), (M + i, M + j, 2 * M + 1)]
    return v, np.array(f, np.int32)


def _f32_exact(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64) == np.asarray(x, np.float64)


def _degenerate_rays(v, f, o, rng, nedge):
    """rays from o exactly through vertices (d = v - o, kept only where that subtraction is exact in float32) and
    through float32-rounded points of edges; both again with d scaled by 0.37 and by 250 (near-ties).  -> (d, tri): tri[i]
    is a triangle incident to ray i's target (the pair whose float64 edge functions the bite conditions look at)"""
    o64, v64 = np.asarray(o, np.float64), v.astype(np.float64)
    dv = v64 - o64
    keep = _f32_exact(dv).all(1) & (np.abs(dv).max(1) > 0)
    first_tri = np.full(len(v), -1, np.int64)
    for t in range(len(f) - 1, -1, -1):
        first_tri[f[t]] = t
    k = rng.integers(0, len(f), nedge)
    e = rng.integers(0, 3, nedge)
    s = rng.random(nedge)
    pa, pb = v64[f[k, e]], v64[f[k, (e + 1) % 3]]
    pt = (pa * (1 - s[:, None]) + pb * s[:, None]).astype(np.float32).astype(np.float64)
    de = (pt - o64).astype(np.float32).astype(np.float64)
    d = np.concatenate([dv[keep], de])
    tri = np.concatenate([first_tri[keep], k])
    ok = np.abs(d).max(1) > 0
    d, tri = d[ok], tri[ok]
    ds = [d.astype(np.float32)] + [(d.astype(np.float32) * np.float32(c)).astype(np.float32) for c in (0.37, 250.0)]
    return np.concatenate(ds), np.tile(tri, 3)


def _needle_rays(v, f, rng, per_edge=64):
    """Near-ties at the resolution of FLOAT64 from float32 rays.  A float32 direction resolves 2^-24 of its length, so
    a ray aimed at an edge misses it by about that much and float64 never has to round.  Except along an axis: from an
    origin o = m - s L e (m the integer midpoint of an edge b c, e a coordinate axis, L a power of two, o proven strictly
    inside by star_shaped) the ray o + t (s L e) runs through the edge exactly, and directions d = s L e + w with
    w = 2^-k (m1, m2) across the axis fan out around it in steps of 2^-k-24 L.  The edge function of b c is LINEAR in w
    and vanishes along the edge's own direction g: with (m1, m2) = the integer points next to the line through 0 along
    g it takes its smallest non-zero values, 2^-k 2^-24 of its two products and less -- for k around 30 that is the
    last bit of a float64, while b and c stay far from the ray, so the products do not shrink with it.
    -> (o [n, 3], d [n, 3], tri [n]): every ray twice, once with each triangle of the edge"""
    v64 = v.astype(np.float64)
    ext = 2.0 ** np.floor(np.log2(np.abs(v64).max()))
    edges = {}
    for t, (a, b, c) in enumerate(f.tolist()):
        for p, q in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(p, q), max(p, q)), []).append(t)
    os_, ds, ts = [], [], []
    for (p, q), tris in sorted(edges.items()):
        mid = (v64[p] + v64[q]) / 2
        g = v64[q] - v64[p]
        found = None
        for L in (ext / 4, ext / 16, ext / 64, ext / 256):
            for ax in range(3):
                for sg in (1.0, -1.0):
                    o = mid.copy()
                    o[ax] -= sg * L
                    if found is None and _f32_exact(o).all() and star_shaped(v, f, o.astype(np.float32)):
                        found = (o, ax, sg, L)
        if found is None:
            continue
        o, ax, sg, L = found
        p1, p2 = (ax + 1) % 3, (ax + 2) % 3
        gm = max(abs(g[p1]), abs(g[p2]))
        if gm == 0:
            continue
        for j in range(per_edge):
            k = int(rng.integers(26, 40))
            lam = float(rng.uniform(0.1, 0.9)) * (1 if rng.random() < 0.5 else -1)
            m1 = np.rint(lam * g[p1] / gm * (1 << 23)) + int(rng.integers(-2, 3))
            m2 = np.rint(lam * g[p2] / gm * (1 << 23)) + int(rng.integers(-2, 3))
            d = np.zeros(3)
            d[ax] = sg * L
            d[p1], d[p2] = m1 * L * 2.0 ** (-k - 23), m2 * L * 2.0 ** (-k - 23)
            assert _f32_exact(d).all()
            for t in tris:
                os_.append(o)
                ds.append(d)
                ts.append(t)
    return np.array(os_, np.float32), np.array(ds, np.float32), np.array(ts, np.int64)


@functools.lru_cache(maxsize=None)
def degenerate_scenes():
    """corpus (b): float64 rounds here; the truth is `exactly one crossing` from an origin that star_shaped() proves
    (rays with inside = True), and even parity from the two origins outside.  One run = one mesh: dict(name, v, f,
    o [n, 3], d [n, 3], tri [n], inside [n], stars: the origins star_shaped() has to prove).  The `needle` runs add what
    makes float64 ROUND on pairs that matter (_needle_rays)."""
    scenes = []
    fans = [(3, 0, (0, 0, 0), 1.0), (5, -30, (0, 0, 0), 1.0), (64, -60, (0, 0, 0), 1.0), (1000, -90, (0, 0, 0), 1.0),
            (64, -9, (0, 0, 0), 1.0), (1000, -20, (0, 0, 0), 1.0),
            (5, -4, (3, -5, 7), 1.0), (64, -11, (3, -5, 7), 1.0),           # heights >= 2^10 ulps of the offset
            (5, 0, (1024, -2048, 512), 1.0), (64, -2, (1024, -2048, 512), 1.0),
            (64, -60, (0, 0, 0), 2.0 ** 20), (64, -60, (0, 0, 0), 2.0 ** -20), (5, -30, (0, 0, 0), 2.0 ** 20),
            (5, -30, (0, 0, 0), 2.0 ** -20)]
    for k, (N, hexp, centre, scale) in enumerate(fans):
        v, f, c = _fan(N, hexp, centre, scale)
        scenes.append((f"fan{N}_h{hexp}_c{int(centre[0])}_s{int(np.log2(scale))}", v, f, c,
                       [c + np.float32(scale) * np.float32([3, 2, 1.5]), c + np.float32(scale) * np.float32([-0.5, 2.75, -1.25])],
                       min(1500, 12 * N), 300 + k))
    rng = np.random.default_rng(7)
    for k in range(10):
        v, f, c = _tetra(rng)
        ext = float(np.abs(v).max())
        scenes.append((f"tetra{k}", v, f, c, [np.float32([2 * ext, ext, 0.5 * ext]), np.float32([-ext, 3 * ext, 2 * ext])], 400, 400 + k))
    v, f = _tube()
    scenes.append(("tube_mid", v, f, np.float32([2500, 0, 0]), [np.float32([2500, 3, 2]), np.float32([-4, 0.5, 0.25])], 600, 500))
    scenes.append(("tube_end", v, f, np.float32([1, 0.0625, 0]), [], 600, 501))
    runs = []
    for name, v, f, c, outs, nedge, seed in scenes:
        rng = np.random.default_rng(seed)
        os_, ds, ts, ins = [], [], [], []
        for o, inside in [(c, True)] + [(np.asarray(x, np.float32), False) for x in outs]:
            d, tri = _degenerate_rays(v, f, o, rng, nedge if inside else max(nedge // 3, 50))
            os_.append(np.tile(np.asarray(o, np.float32), (len(d), 1)))
            ds.append(d)
            ts.append(tri)
            ins.append(np.full(len(d), inside))
        runs.append(dict(name=name, v=v, f=f, o=np.concatenate(os_), d=np.concatenate(ds), tri=np.concatenate(ts),
                         inside=np.concatenate(ins), stars=[np.asarray(c, np.float32)]))
    # the unimodular tetrahedra are too flat to hold a second origin: the needle rays get tetrahedra with some volume
    rng = np.random.default_rng(8)
    ftet = np.array([(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)], np.int32)
    while sum(r["name"].startswith("needle") for r in runs) < 8:
        M = rng.integers(-(1 << 19), 1 << 19, (3, 3)) * 2
        v = np.concatenate([M, [-M.sum(0)]]).astype(np.float32)
        if abs(np.linalg.det(M.astype(np.float64))) < 2.0 ** 57:
            continue
        f = ftet if star_shaped(v, ftet, np.zeros(3, np.float32)) else ftet[:, [0, 2, 1]]
        o, d, tri = _needle_rays(v, f, rng)
        if len(o):
            runs.append(dict(name=f"needle{len(runs)}", v=v, f=f, o=o, d=d, tri=tri, inside=np.ones(len(o), bool),
                             stars=list(np.unique(o, axis=0))))
    return runs


def points_truth(v, f, p):
    """inside / outside of the closed surface (v, f) for float32 points p by the parity of the ideal crossings along +x,
    confirmed along +y, every (point, triangle) pair in Python integers -> (keep [n]: the point lies on no triangle
    and the two axes agree, inside [n])"""
    p = np.asarray(p, np.float32)
    n, nf = len(p), len(f)
    o = np.repeat(p, nf, 0)
    tri = np.tile(np.arange(nf), n)
    par, keep = [], np.ones(n, bool)
    for axis in (0, 1):
        d = np.zeros((n * nf, 3), np.float32)
        d[:, axis] = 1
        c = pairs(v, f, o, d, tri)
        hit = np.asarray(c["hit"], bool).reshape(n, nf)
        touch = (np.asarray(c["inside"], bool) & (c["st"] == 0)).reshape(n, nf) | (c["sdet"] == 0).reshape(n, nf)
        keep &= ~touch.any(1)
        par.append(hit.sum(1) % 2 == 1)
    return keep & (par[0] == par[1]), par[0]


def tetra_points(run):
    """integer points and points at odd multiples of 1/2 in and around one of the doubled tetrahedra (2A, 2B, 2C, 2D) of
    corpus (b): A ... D (half way to the vertices), the middles between two of them, their mirror images and
    multiples outside, and the points next to the origin -> (points float32 [n, 3], inside [n])"""
    h = run["v"].astype(np.float64) / 2
    pts = [np.zeros(3)] + [s * x for x in h for s in (1, -1, 3)]
    pts += [s * (h[i] + h[j]) / 2 for i in range(4) for j in range(i) for s in (1, -1)]
    g = np.array([-1.5, -1, -0.5, 0.5, 1, 1.5])
    pts += [np.array([x, y, z]) for x in g[::2] for y in g[1::2] for z in g[::3]]
    p = np.array(pts)
    p = p[_f32_exact(p).all(1)].astype(np.float32)
    keep, inside = points_truth(run["v"], run["f"], p)
    return p[keep], inside[keep]
