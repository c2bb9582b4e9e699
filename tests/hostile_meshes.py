"""Meshes with hostile vertices (tests/test_hostile_meshes_cpu.py, tests/test_gpu_hostile_meshes.py); not a test module.

The rule (arithmetic contract, "Meshes"): a triangle with a NaN or an infinite coordinate is INACTIVE for every
query -- no ray hits it, closest_point offers it no candidate -- and every other triangle answers as if the inactive ones
were not there.  Finite triangles far away (coordinates up to FLT_MAX) are ordinary triangles; what they do is overflow the
padded boxes and the grid frame.

Every family is a function of its seed alone.  The base is the closed W.icosphere(2) (320 faces); extra triangles have
coordinates uniform in [-2, 2] before they are made hostile, and the faces are permuted so that the hostile ones are
spread over the ids:

    nonfinite           48 extras with one to three of their nine coordinates replaced by NaN, +Inf or -Inf
    faraway             48 extras moved as whole triangles to an offset from OFFSETS on one to three axes, their size scaled
                        with the largest offset (2^-4 of it) and every coordinate clipped to +-FLT_MAX: all finite, and every
                        coordinate of one triangle of one magnitude (no stretched triangles: DESIGN.md, "Meshes")
    faraway_nonfinite   32 of each
    deep_nan            W.deep_tree_mesh(8) (a hierarchy of more than 32 levels) plus 16 extras with NaN only, their finite
                        coordinates inside the tree's own box [0, 1]: the bounds ignore NaN, so the Morton keys of the tree
                        and its depth survive (an infinite frame collapses every key and cannot be deep)

and the single cases of SINGLE.  case(name, seed) returns a Case with its rays and points and what the oracle's brute
force says about them."""
import functools

import numpy as np

import workloads as W

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
OFFSETS = (FLT_MAX, -FLT_MAX, 3e38, -1e30, 2.0 ** 60, -(2.0 ** 100))
FAMILIES = ("nonfinite", "faraway", "faraway_nonfinite")
SEEDS = (0, 1, 2)
SINGLE = ("all_nan_triangle", "unreferenced_nan_vertex", "holed_sphere", "all_inactive", "one_triangle_nan", "one_triangle_inf",
          "two_triangles_nan", "two_triangles_inf", "denormal")
DENORMAL_SCALE = 1e-39


class Case:
    """v [nv, 3] float32, f [nf, 3] int32; hostile [nf]: the faces that make the case what it is; o, d [n, 3] rays;
    p [m, 3] points"""

    def __init__(self, name, v, f, hostile, o, d, p):
        self.name = name
        self.v, self.f = np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32)
        self.hostile = np.asarray(hostile, bool)
        self.o, self.d, self.p = (np.ascontiguousarray(x, F32) for x in (o, d, p))
        self.inactive = ~np.isfinite(self.v[self.f]).all(axis=(1, 2)) if len(self.f) else np.zeros(0, bool)
        for x in (self.v, self.f, self.hostile, self.o, self.d, self.p, self.inactive):
            x.setflags(write=False)


def active_faces(v, f):
    """(the faces without a non-finite coordinate, in their order; new id of every old face, -1 for a removed one)"""
    v, f = np.asarray(v, F32), np.asarray(f, np.int32)
    keep = np.isfinite(v[f]).all(axis=(1, 2)) if len(f) else np.zeros(0, bool)
    new = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return np.ascontiguousarray(f[keep]), new


def map_ids(tri, new):
    """face ids of the whole mesh -> ids of active_faces(mesh); -1 stays -1"""
    tri = np.asarray(tri)
    return np.where(tri >= 0, new[np.maximum(tri, 0)], tri).astype(tri.dtype)


# ---- the families -------------------------------------------------------------------------------------------------------
def _extras(rng, n):
    return rng.uniform(-2.0, 2.0, (n, 3, 3)).astype(F32)


def _make_nonfinite(rng, t, values=(np.nan, np.inf, -np.inf)):
    t = t.copy()
    for k in range(len(t)):
        where = rng.choice(9, size=int(rng.integers(1, 4)), replace=False)
        t[k].reshape(-1)[where] = rng.choice(np.array(values, F32), size=len(where))
    return t


def _make_faraway(rng, t):
    out = np.empty_like(t)
    for k in range(len(t)):
        axes = rng.choice(3, size=int(rng.integers(1, 4)), replace=False)
        off = np.zeros(3)
        off[axes] = rng.choice(np.array(OFFSETS), size=len(axes))
        size = np.abs(off).max() * 2.0 ** -4
        with np.errstate(over="ignore"):
            out[k] = np.clip(t[k].astype(np.float64) * size + off, -FLT_MAX, FLT_MAX).astype(F32)
    assert np.isfinite(out).all()
    return out


def _append(rng, v, f, tris):
    """the mesh plus `tris` [k, 3, 3] as new vertices and faces, the faces permuted -> (v, f, which faces are the new ones)"""
    v2 = np.concatenate([v, tris.reshape(-1, 3)]).astype(F32)
    f2 = np.concatenate([f, np.arange(len(v), len(v2), dtype=np.int32).reshape(-1, 3)]).astype(np.int32)
    new = np.arange(len(f2)) >= len(f)
    perm = rng.permutation(len(f2))
    return v2, f2[perm], new[perm]


def rays(v, f, hostile, seed, lo=-1.5, hi=1.5, n=3000, aimed=1000, far=500):
    """n hash rays in the box, `aimed` of them at ordinary vertices; `far` more towards the finite vertices of hostile
    faces, direction normalised in float64"""
    o, d = W.hash_rays(n, 70 + seed, [lo] * 3, [hi] * 3)
    o, d = np.array(o, F32), np.array(d, F32)
    ordinary = np.unique(f[~hostile]) if (~hostile).any() else np.zeros(0, np.int64)
    ordinary = ordinary[np.isfinite(v[ordinary]).all(1)]
    if len(ordinary):
        k = np.arange(aimed)
        d[3 * k] = v[ordinary[(k * 7919) % len(ordinary)]] - o[3 * k]
    targets = v[np.unique(f[hostile])] if hostile.any() else np.zeros((0, 3), F32)
    targets = targets[np.isfinite(targets).all(1)]
    if len(targets) and far:
        of = np.array(W.hash_rays(far, 170 + seed, [lo] * 3, [hi] * 3)[0], F32)
        df = targets[(np.arange(far) * 31) % len(targets)].astype(np.float64) - of
        df /= np.linalg.norm(df, axis=1, keepdims=True)
        o, d = np.concatenate([o, of]), np.concatenate([d, df.astype(F32)])
    assert np.isfinite(o).all() and np.isfinite(d).all()
    return o, d


def _points(seed, scale=1.3, n=600):
    return np.array(W.hash_rays(n, 270 + seed, [-scale] * 3, [scale] * 3)[0], F32)


def _family(name, seed):
    rng = np.random.default_rng(seed)
    v, f = W.icosphere(2)
    if name == "nonfinite":
        tris = _make_nonfinite(rng, _extras(rng, 48))
    elif name == "faraway":
        tris = _make_faraway(rng, _extras(rng, 48))
    elif name == "faraway_nonfinite":
        tris = np.concatenate([_make_faraway(rng, _extras(rng, 32)), _make_nonfinite(rng, _extras(rng, 32))])
    else:
        raise KeyError(name)
    v, f, hostile = _append(rng, v, f, tris)
    o, d = rays(v, f, hostile, seed)
    return Case(f"{name}:{seed}", v, f, hostile, o, d, _points(seed))


def _deep_nan(seed):
    rng = np.random.default_rng(seed)
    v, f = W.deep_tree_mesh(8)
    inside = _extras(rng, 16) * F32(0.125) + F32(0.5)                   # [0.25, 0.75]: the box of the tree stays what it was
    v, f, hostile = _append(rng, v, f, _make_nonfinite(rng, inside, values=(np.nan,)))
    o, d = rays(v, f, hostile, seed, lo=-0.2, hi=1.2, far=0)
    k = np.arange(1, 3000, 3)
    o[k], d[k] = [1e-10, 1e-10, 1.0], [0.0, 0.0, -1.0]                 # a third of the rays down the pile of identical triangles
    return Case(f"deep_nan:{seed}", v, f, hostile, o, d, _points(seed, 1.2))


def _single(name):
    rng = np.random.default_rng(1234)
    v, f = W.icosphere(2)
    nan, inf = F32(np.nan), F32(np.inf)
    scale = 1.0
    if name == "all_nan_triangle":
        v, f, hostile = _append(rng, v, f, np.full((1, 3, 3), nan, F32))
    elif name == "unreferenced_nan_vertex":
        v = np.concatenate([v, [[nan, 0.25, nan]]]).astype(F32)
        hostile = np.zeros(len(f), bool)
    elif name == "holed_sphere":
        v = v.copy()
        v[5] = nan
        v[77, 1] = inf
        hostile = np.isin(f, (5, 77)).any(1)
    elif name == "all_inactive":
        v, f = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
        v, f, hostile = _append(rng, v, f, _make_nonfinite(rng, _extras(rng, 12)))
    elif name.startswith(("one_triangle", "two_triangles")):
        t = np.array([[[-1.0, -1.0, 0.1], [1.0, -1.0, 0.2], [0.0, 1.5, -0.1]], [[-1.0, -1.2, -0.5], [0.2, 1.3, -0.4], [1.1, -0.9, -0.6]]], F32)
        t[0, 1, 2] = nan if name.endswith("nan") else -inf
        t = t[:1] if name.startswith("one") else t
        v, f = t.reshape(-1, 3), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)
        hostile = np.arange(len(f)) == 0
    elif name == "denormal":
        scale = DENORMAL_SCALE
        v = (v.astype(np.float64) * scale).astype(F32)
        hostile = np.ones(len(f), bool)                                # every coordinate of every face is denormal
    else:
        raise KeyError(name)
    o, d = rays(v, f, np.zeros(len(f), bool), 9, far=0)
    p = _points(9)
    if scale != 1.0:
        o, p = (o.astype(np.float64) * scale).astype(F32), (p.astype(np.float64) * scale).astype(F32)
        k = np.arange(1000)
        ordinary = np.unique(f)
        d[3 * k] = v[ordinary[(k * 7919) % len(ordinary)]] - o[3 * k]  # (denormal directions: exact differences)
    return Case(name, v, f, hostile, o, d, p)


def refit_sequence(seed=0):
    """(faces, [(label, vertices)]): one set of faces -- the sphere plus 48 extras, permuted -- under four vertex arrays of
    one shape: clean, the extras made non-finite, the extras moved far away, clean again"""
    rng = np.random.default_rng(1000 + seed)
    v, f = W.icosphere(2)
    extras = _extras(rng, 48)
    steps = [("clean", extras), ("nonfinite", _make_nonfinite(rng, extras)), ("faraway", _make_faraway(rng, extras)), ("clean again", extras)]
    perm = rng.permutation(len(f) + len(extras))
    faces = np.concatenate([f, np.arange(len(v), len(v) + 3 * len(extras), dtype=np.int32).reshape(-1, 3)])[perm].astype(np.int32)
    return faces, [(label, np.concatenate([v, t.reshape(-1, 3)]).astype(F32)) for label, t in steps]


def case(name, seed=None):
    """the Case `name` (a family of FAMILIES or "deep_nan" with a seed, or one of SINGLE), built once"""
    return _case(name, seed)


@functools.lru_cache(maxsize=None)
def _case(name, seed):
    if name in FAMILIES:
        return _family(name, seed)
    if name == "deep_nan":
        return _deep_nan(seed)
    return _single(name)


ALL_CASES = [(name, seed) for name in FAMILIES + ("deep_nan",) for seed in SEEDS] + [(name, None) for name in SINGLE]
CASE_IDS = [name if seed is None else f"{name}-{seed}" for name, seed in ALL_CASES]


# ---- what the oracle's brute force says -------------------------------------------------------------------------------
def oracle(name, seed=None, mode=0):
    """{"closest": (hit, front, tri, loc, uv), "count", "location": (loc, ray, tri), "location_t"} of the case's rays"""
    return _oracle(name, seed, mode)


def oracle_results(v, f, o, d, mode):
    from oracle.oracle import OracleIntersector
    R = OracleIntersector(v, f, mode)
    loc, ray, tri, t = R.intersects_location(o, d, with_t=True)
    out = {"closest": R.closest_raw(o, d)[:5], "count": R.intersects_count(o, d), "location": (loc, ray, tri), "location_t": t}
    for x in (*out["closest"], out["count"], *out["location"], t):
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name, seed, mode):
    c = case(name, seed)
    return oracle_results(c.v, c.f, c.o, c.d, mode)


@functools.lru_cache(maxsize=None)
def oracle_active(name, seed=None):
    """the brute force on active_faces(mesh): ids are those of the reduced mesh"""
    c = case(name, seed)
    fa, _ = active_faces(c.v, c.f)
    return oracle_results(c.v, fa, c.o, c.d, 0)


# ---- the rules that need no oracle ------------------------------------------------------------------------------------
# "The same query on active_faces(mesh)" has a domain: a ray is ANCHORED to the mesh's grid frame before anything else
# (contract 3: tr_ray_anchor moves a ray that starts far outside the frame to just before its entry point), and the frame
# is a function of ALL vertices that faces reference -- an infinite vertex makes it infinite (nothing is anchored), the
# finite coordinates of an inactive triangle widen it.  The two meshes therefore trace the same ray only where both
# anchor it to the same origin, which same_anchor() decides with the oracle's statement of the anchoring; measured on
# "nonfinite" seed 0, 136 of 3500 rays are anchored differently and 6 of them change their hit (rays aimed at vertices).
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def same_anchor(name, seed=None):
    """[n] bool: the rays that the mesh and active_faces(mesh) anchor to the same origin, bit for bit"""
    from oracle.oracle import OracleIntersector
    c = case(name, seed)
    fa, _ = active_faces(c.v, c.f)
    a, b = (OracleIntersector(c.v, ff, 0).anchor(c.o, c.d) for ff in (c.f, fa))
    keep = (a.view(np.uint32) == b.view(np.uint32)).all(1)
    keep.setflags(write=False)
    return keep


def tiled(exp, reps, n):
    """the results of a batch of n rays (the dict of oracle()) for the batch repeated `reps` times"""
    loc, ray, tri = exp["location"]
    return {"closest": tuple(np.concatenate([x] * reps) for x in exp["closest"]), "count": np.tile(exp["count"], reps),
            "location": (np.concatenate([loc] * reps), np.concatenate([ray + np.int32(j * n) for j in range(reps)]).astype(ray.dtype),
                         np.tile(tri, reps))}


def check_rules(c, query, got, alone, keep, what, reps=1):
    """got / alone: numpy outputs of one query on the case's mesh / on active_faces of it, in the forms of
    hostile_rays.check_rules: any -> hit, first -> tri, closest -> (hit, front, tri, loc, uv), count -> count,
    location -> (loc, ray, tri); keep = same_anchor(...).
      * no output names an inactive face;  * no output holds a non-finite float;
      * on the rays of `keep`, every output equals the reduced mesh's, face ids mapped, bit for bit."""
    assert len(keep) == len(c.o)
    _, new = active_faces(c.v, c.f)
    n = len(c.o) * reps                                    # (reps: the case's rays repeated, test_gpu_hostile_meshes.py)
    keep = np.tile(keep, reps)

    def faces(tri, name):
        tri = np.asarray(tri).reshape(-1)
        assert ((tri >= -1) & (tri < len(c.f))).all(), f"{what}: {name} outside the mesh"
        assert not c.inactive[tri[tri >= 0]].any(), f"{what}: {name} names an inactive face"

    def finite(x, name):
        assert np.isfinite(np.asarray(x)).all(), f"{what}: {name} holds a non-finite float"

    def per_ray(name, g, a):
        g, a = np.asarray(g).reshape(n, -1), np.asarray(a).reshape(n, -1)
        assert g.dtype == a.dtype and _same(g[keep], a[keep]), f"{what}: {name} differs from the active faces alone"

    if query in ("any", "count"):
        per_ray(query, got, alone)
    elif query == "first":
        faces(got, "tri")
        per_ray("tri", map_ids(np.asarray(got).reshape(-1), new), alone)
    elif query == "closest":
        hit, front, tri, loc, uv = (np.asarray(g) for g in got)
        faces(tri, "tri"); finite(loc, "loc"); finite(uv, "uv")
        assert np.array_equal(hit.reshape(-1), tri.reshape(-1) >= 0), f"{what}: hit and tri disagree"
        for name, g, a in zip(("hit", "front", "tri", "loc", "uv"), (hit, front, map_ids(tri, new), loc, uv), alone):
            per_ray(name, g, a)
    elif query == "location":
        (loc, ray, tri), (aloc, aray, atri) = (tuple(np.asarray(x) for x in g) for g in (got, alone))
        faces(tri, "tri"); finite(loc, "loc")
        assert ray.min(initial=0) >= 0 and ray.max(initial=0) < n and np.all(np.diff(ray) >= 0), f"{what}: ray ids of the lists"
        rows, arows = keep[ray], keep[aray]
        for name, g, a in zip(("loc", "ray", "tri"), (loc[rows], ray[rows], map_ids(tri, new)[rows]), (aloc[arows], aray[arows], atri[arows])):
            assert g.dtype == a.dtype and _same(g, a), f"{what}: location {name} differs from the active faces alone"
    else:
        raise KeyError(query)


def check_nearest_rules(c, got, alone, what):
    """closest_point outputs (closest, distance, tri) on the mesh / on active_faces of it: no anchoring, every point"""
    _, new = active_faces(c.v, c.f)
    closest, distance, tri = (np.asarray(g) for g in got)
    assert ((tri >= -1) & (tri < len(c.f))).all() and not c.inactive[tri[tri >= 0]].any(), f"{what}: tri names an inactive face"
    found = tri >= 0
    assert np.isfinite(closest[found]).all() and np.isfinite(distance[found]).all(), f"{what}: a non-finite float beside a triangle"
    assert np.isnan(closest[~found]).all() and np.isposinf(distance[~found]).all(), f"{what}: no triangle, but not (NaN, +Inf)"
    ac, ad, at = alone
    assert _same(map_ids(tri, new), at) and _same(distance, ad), f"{what}: differs from the active faces alone"
    assert _same(closest[found], np.asarray(ac)[found]), f"{what}: closest differs from the active faces alone"
