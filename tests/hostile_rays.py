"""Rays at the ends of the float range, mixed among ordinary ones (tests/test_gpu_hostile_rays.py).

hostile_batch() derives, from a base set of ordinary rays aimed at a scene, the families the ray set-up code makes
promises about (csrc/tr_math.h tr_ray_setup / tr_inv / tr_ray_anchor, csrc/tr_bvh.h tr_fuse_axis) and returns them with
the ordinary rays in one batch, in one of two layouts.  Every ray knows its family and the base ray it came from, so that
the rules that do not need an oracle can be stated per ray:

    family        what becomes of the base ray (o, d)
    nonfinite     one of the six components is NaN, NaN with the sign bit, +Inf or -Inf; a few with several        (miss)
    zero          d = (+-0, +-0, +-0), the eight sign patterns                                                    (miss)
    scale:k       d * 2^k, k in SCALES: -136 all components denormal, 40 / 41 either side of TR_BAND_MAXLEN,
                  126 denormal reciprocals and denormal hit distances; k in IDENTITY_SCALES: the base ray's bits
    comp:x        one direction component replaced: 1e-45, -1e-42, +0, -0 in a minor one, the origin moved into the plane
                  of that coordinate through the base ray's target; 3e38 (its sign kept) in the dominant one, the origin
                  moved so that the line passes through the target; all:3e38: all three +-3e38, the origin on that
                  diagonal through the target
    far:O/D       origin at O behind the target on the ray's dominant axis, direction D along that axis
    origin:x      the dominant origin component replaced by +-3.4e38 (misses: beyond tmax) or 1e-45
    ordinary      the base rays, every one of them, unchanged

The target of a base ray is the oracle's closest hit (o + d for a miss): the families that turn the direction still aim
at the surface the base ray saw.

A ray of scale:126, comp:3e38, all:3e38 or far:3e38/... has a denormal reciprocal: the fused grid-node test then accepts
nearly every node ("the cost cliff"), which is why these families stay at a few hundred rays per batch."""
import functools
import os

import numpy as np

SCALES = (-136, -100, -22, -10, 40, 41, 100, 126)
IDENTITY_SCALES = (-10, 40, 41, 100, 126)          # below, the reference's tmax = 1e7 starts to cut hits off
MISS_BY_CONSTRUCTION = ("scale:-136", "scale:-100", "origin:+3.4e38", "origin:-3.4e38")
INVALID = ("nonfinite", "zero")
PER_INVALID_VARIANT = 16                            # 28 non-finite and 8 zero variants: 448 + 128 = 576 invalid rays
RUNS = (64, 64, 128, 192, 64, 64)                   # the blocked layout's runs of invalid rays, first and last at the ends
FAR = (("far:2^60/-2^40", 2.0 ** 60, 2.0 ** 40), ("far:3e38/-3e38", 3e38, 3e38), ("far:3e38/-1e32", 3e38, 1e32),
       ("far:1e31/-1e25", 1e31, 1e25))

_NAN, _NAN_NEG = np.uint32(0x7FC00000).view(np.float32), np.uint32(0xFFC00000).view(np.float32)
_INF = np.float32(np.inf)
# (component 0..2 of the origin, 3..5 of the direction) -> value
_NONFINITE = [{c: x} for c in range(6) for x in (_NAN, _NAN_NEG, _INF, -_INF)] + [
    {0: _NAN, 5: _INF}, {c: _NAN_NEG for c in range(6)}, {3: _INF, 4: -_INF}, {0: _INF, 1: _INF, 2: -_INF}]
_ZERO = [tuple(np.float32(-0.0) if (k >> c) & 1 else np.float32(0.0) for c in range(3)) for k in range(8)]


class Batch:
    """o, d [n, 3] float32; family [n] (index into .names); src [n] (the base ray each one came from); pos [B] (where base
    ray j stands, unchanged, in the batch)"""

    def __init__(self, o, d, family, src, names):
        self.o, self.d, self.family, self.src, self.names = o, d, family, src, names
        self.n = len(o)
        ordinary = np.flatnonzero(family == names.index("ordinary"))
        self.pos = np.empty(len(ordinary), np.int64)
        self.pos[src[ordinary]] = ordinary

    def mask(self, *prefixes):
        """rays whose family name starts with one of `prefixes`"""
        ids = [k for k, name in enumerate(self.names) if name.startswith(prefixes)]
        return np.isin(self.family, ids)

    def members(self, name):
        return np.flatnonzero(self.family == self.names.index(name))


def _spread(B, m, j):
    """m base indices spread evenly over the base set, shifted per family so that families do not share their rays"""
    return ((np.arange(m, dtype=np.int64) * B) // m + 7 * j) % B


def _content(o, d, target, per):
    o, d, target = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (o, d, target))
    B = len(o)
    dom = np.argmax(np.abs(d), axis=1)
    sgn = np.where(np.signbit(d), np.float32(-1), np.float32(1))
    names, parts = [], []

    def add(name, src, oo, dd):
        names.append(name)
        parts.append((np.full(len(src), len(names) - 1, np.int32), src, oo.astype(np.float32), dd.astype(np.float32)))

    # 1. non-finite, 2. zero direction
    for fam, variants in (("nonfinite", _NONFINITE), ("zero", _ZERO)):
        src = _spread(B, PER_INVALID_VARIANT * len(variants), len(names))
        od = np.concatenate([o[src], d[src]], axis=1)
        for k, var in enumerate(variants):
            rows = slice(k * PER_INVALID_VARIANT, (k + 1) * PER_INVALID_VARIANT)
            if fam == "zero":
                od[rows, 3:] = var
            else:
                for c, x in var.items():
                    od[rows, c] = x
        add(fam, src, od[:, :3], od[:, 3:])
    # 3. power-of-two scales of the direction
    for k in SCALES:
        src = _spread(B, per, len(names))
        add(f"scale:{k}", src, o[src], np.ldexp(d[src], k))
    # 4. single components at the ends
    r = np.arange(per)
    for name, x in (("comp:1e-45", 1e-45), ("comp:-1e-42", -1e-42), ("comp:+0", 0.0), ("comp:-0", -0.0)):
        src = _spread(B, per, len(names))
        oo, dd, c = o[src].copy(), d[src].copy(), (dom[src] + 1) % 3
        dd[r, c] = np.float32(x)
        oo[r, c] = target[src][r, c]                # the ray now runs in the plane of that coordinate through its target
        add(name, src, oo, dd)
    src = _spread(B, per, len(names))
    oo, dd = target[src].copy(), d[src].copy()
    oo[r, dom[src]] = o[src][r, dom[src]]
    dd[r, dom[src]] = sgn[src][r, dom[src]] * np.float32(3e38)
    add("comp:3e38", src, oo, dd)
    src = _spread(B, per, len(names))
    # back along the diagonal by the power of two below the base ray's own distance to its target -- and no further than
    # 2^21 times the target's smallest non-zero coordinate: the rounded origin then still resolves the target to an eighth
    # of that coordinate (the deep tree's triangles are 1e-9 wide at 1e-10 from an axis: from a distance of 1 nothing would
    # aim at them)
    mag = np.abs(target[src])
    dist = np.minimum(np.max(np.abs(target[src] - o[src]), axis=1), np.min(np.where(mag > 0, mag, np.inf), axis=1) * np.float32(2.0 ** 21))
    back = np.exp2(np.floor(np.log2(np.maximum(dist, np.float32(2.0 ** -60))))).astype(np.float32)
    add("all:3e38", src, target[src] - sgn[src] * back[:, None], sgn[src] * np.float32(3e38))
    # 5. far origins, axis-parallel; origin components at the ends under the ordinary direction
    for name, O, D in FAR:
        src = _spread(B, per, len(names))
        oo, dd = target[src].copy(), np.zeros((per, 3), np.float32)
        oo[r, dom[src]] = -sgn[src][r, dom[src]] * np.float32(O)
        dd[r, dom[src]] = sgn[src][r, dom[src]] * np.float32(D)
        add(name, src, oo, dd)
    for name, x in (("origin:+3.4e38", 3.4e38), ("origin:-3.4e38", -3.4e38), ("origin:1e-45", 1e-45)):
        src = _spread(B, per, len(names))
        oo = o[src].copy()
        oo[r, dom[src]] = np.float32(x)
        add(name, src, oo, d[src])
    # 6. the ordinary rays
    add("ordinary", np.arange(B, dtype=np.int64), o, d)
    fam, src, oo, dd = (np.concatenate([p[k] for p in parts]) for k in range(4))
    return fam, src, oo, dd, names


def _merge(classes):
    """one order over the members of all classes (lists of index arrays) in which each class is spread evenly, classes of
    one size a fraction of their period apart"""
    idx = np.concatenate(classes)
    key = np.concatenate([(np.arange(len(c)) + (k + 0.5) / len(classes)) / max(len(c), 1) for k, c in enumerate(classes)])
    return idx[np.argsort(key, kind="stable")]


def hostile_batch(o, d, target, layout, per=368):
    """layout "interleaved": every 64 consecutive rays hold ordinary rays and several hostile families;
    "blocked": the invalid rays (nonfinite, zero) stand in runs of RUNS with the other rays between them, the first and
    the last run at the ends of the batch.  Same content in both; the length is no multiple of 64."""
    fam, src, oo, dd, names = _content(o, d, target, per)
    n = len(fam)
    ordinary = names.index("ordinary")
    invalid = np.isin(fam, [names.index(x) for x in INVALID])
    # every hostile family spread evenly over the hostile rays, these merged evenly with the ordinary ones

    def round_robin(sel):
        return _merge([sel[fam[sel] == k] for k in np.unique(fam[sel])])
    if layout == "interleaved":
        order = _merge([np.flatnonzero(fam == ordinary), round_robin(np.flatnonzero(fam != ordinary))])
    elif layout == "blocked":
        live = _merge([np.flatnonzero(fam == ordinary), round_robin(np.flatnonzero((fam != ordinary) & ~invalid))])
        dead = round_robin(np.flatnonzero(invalid))
        assert len(dead) == sum(RUNS)
        s = len(live) // 5 // 64 * 64
        gaps = [0, s, s, s + 48, s, len(live) - (4 * s + 48)]          # the third and fourth run start off a multiple of 64
        assert min(gaps[1:]) > 0
        chunks, a, b = [], 0, 0
        for gap, run in zip(gaps, RUNS):
            chunks += [live[a:a + gap], dead[b:b + run]]
            a, b = a + gap, b + run
        order = np.concatenate(chunks)
    else:
        raise ValueError(layout)
    assert len(order) == n and n % 64 != 0 and np.array_equal(np.sort(order), np.arange(n))
    batch = Batch(np.ascontiguousarray(oo[order]), np.ascontiguousarray(dd[order]), fam[order], src[order], names)
    batch.order = order                             # position in the layout-free content (the same for both layouts)
    dead = batch.mask(*INVALID)
    if layout == "interleaved":
        for lo in range(0, n - 63, 64):
            g = batch.family[lo:lo + 64]
            assert (g == ordinary).any() and len(np.unique(g[g != ordinary])) >= 4 and dead[lo:lo + 64].any() and not dead[lo:lo + 64].all()
    else:
        edges = np.flatnonzero(np.diff(np.concatenate([[0], dead.astype(np.int8), [0]])))
        assert [int(x) for x in edges[1::2] - edges[0::2]] == list(RUNS) and dead[:64].all() and dead[-64:].all()
    return batch


# ---- the rules that hold whatever the oracle says ---------------------------------------------------------------------
def per_ray_rows(ray, n):
    """location lists -> (count of rows per ray, offset of each ray's first row); rows of one ray are consecutive"""
    assert np.all(np.diff(ray) >= 0), "the rows of the location lists are not in ray order"
    cnt = np.bincount(ray, minlength=n)
    return cnt, np.concatenate([[0], np.cumsum(cnt)[:-1]])


def _rows_of(rays, cnt, off):
    """flat row indices of the given rays, in order"""
    c = cnt[rays]
    start = np.repeat(off[rays], c)
    within = np.arange(int(c.sum())) - np.repeat(np.concatenate([[0], np.cumsum(c)[:-1]]), c)
    return start + within


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_rules(batch, query, got, alone, what):
    """got / alone: numpy outputs of one query on the batch / on the ordinary rays alone (the base set, in its order):
    any -> hit, first -> tri, closest -> (hit, front, tri, loc, uv), count -> count, location -> (loc, ray, tri)"""
    dead = batch.mask(*INVALID)
    twins = [(batch.members(f"scale:{k}"), k) for k in IDENTITY_SCALES]

    def per_ray(name, g, a, miss):
        g = g.reshape(batch.n, -1)
        assert np.all(g[dead] == miss), f"{what}: {name} of an invalid ray is not {miss}"
        assert _same(g[batch.pos], a.reshape(len(batch.pos), -1)), f"{what}: {name} of the ordinary rays differs from the ordinary rays alone"
        for rays, k in twins:
            assert _same(g[rays], g[batch.pos[batch.src[rays]]]), f"{what}: {name} at scale 2^{k} differs from the unscaled ray"
        if g.dtype.kind == "f":
            assert np.isfinite(g).all(), f"{what}: {name} holds a non-finite float"

    if query == "any":
        per_ray("hit", got, alone, False)
    elif query == "first":
        per_ray("tri", got, alone, -1)
    elif query == "count":
        per_ray("count", got, alone, 0)
    elif query == "closest":
        for name, g, a, miss in zip(("hit", "front", "tri", "loc", "uv"), got, alone, (False, False, -1, 0.0, 0.0)):
            per_ray(name, g, a, miss)
    else:
        (loc, ray, tri), (aloc, aray, atri) = got, alone
        assert np.isfinite(loc).all(), f"{what}: the location list holds a non-finite float"
        assert ray.min(initial=0) >= 0 and ray.max(initial=0) < batch.n
        cnt, off = per_ray_rows(ray, batch.n)
        assert not cnt[dead].any(), f"{what}: an invalid ray owns rows of the location lists"
        acnt, aoff = per_ray_rows(aray, len(batch.pos))
        assert np.array_equal(cnt[batch.pos], acnt), f"{what}: rows per ordinary ray differ from the ordinary rays alone"
        rows = _rows_of(batch.pos, cnt, off)
        assert _same(loc[rows], aloc) and _same(tri[rows], atri), f"{what}: rows of the ordinary rays differ from the ordinary rays alone"
        for rays, k in twins:
            base = batch.pos[batch.src[rays]]
            assert np.array_equal(cnt[rays], cnt[base]), f"{what}: rows per ray at scale 2^{k}"
            a, b = _rows_of(rays, cnt, off), _rows_of(base, cnt, off)
            assert _same(loc[a], loc[b]) and _same(tri[a], tri[b]), f"{what}: rows at scale 2^{k} differ from the unscaled ray's"


# ---- the three scenes, their base rays and what the oracle says about them ---------------------------------------------
def scene(name, base=8192):
    """(v, f, o, d, target, the oracle's results on the base rays alone), computed once per (name, base)"""
    return _scene(name, base)


@functools.lru_cache(maxsize=None)
def _scene(name, base):
    """(v, f, o, d, target, the oracle's results on the base rays alone): the smallest scenes of the kernel matrix that
    reach every flavour -- a soup (up to 100 hits per ray), six nested shells under a pinhole camera (12 hits per ray),
    the deep tree (hierarchy deeper than 32 levels; a sixteenth of the rays go down the pile of 3000 identical triangles)"""
    import workloads as W
    from oracle.oracle import OracleIntersector
    if name == "soup":
        v, f = W.random_soup(20000, seed=5)
        o, d = W.hash_rays(base, 61, [-1.3] * 3, [1.3] * 3)
    elif name == "shells":
        v, f = W.nested_shells(4, radii=(1.0, 0.85, 0.7, 0.55, 0.4, 0.25))
        o, d = W.pinhole_grid(128, base // 128, distance=2.5)
        o, d = np.broadcast_to(o, d.shape).reshape(-1, 3), d.reshape(-1, 3)
    elif name == "deep":
        v, f = W.deep_tree_mesh(3000)
        o, d = W.hash_rays(base, 62, [-0.2] * 3, [1.2] * 3)
        o[:base // 16] = [1e-10, 1e-10, 1.0]
        d[:base // 16] = [0.0, 0.0, -1.0]
    else:
        raise KeyError(name)
    o, d = np.array(o, np.float32, order="C"), np.array(d, np.float32, order="C")
    R = OracleIntersector(v, f, 1)
    alone = {"closest": R.closest_raw(o, d)[:5], "count": R.intersects_count(o, d), "location": R.intersects_location(o, d)}
    hit, loc = alone["closest"][0], alone["closest"][3]
    target = np.where(hit[:, None], loc, o + d).astype(np.float32)
    for x in (v, f, o, d, target, *alone["closest"], alone["count"], *alone["location"]):
        x.setflags(write=False)
    return v, f, o, d, target, alone


def expected(name, layout, base=8192, per=368):
    """(batch, the oracle's results on it), computed once per (name, layout, base, per)"""
    return _expected(name, layout, base, per)


@functools.lru_cache(maxsize=None)
def _expected(name, layout, base, per):
    """(batch, the oracle's results on it), with the conditions that keep a test on it from passing by vacuity"""
    from oracle.oracle import OracleIntersector
    v, f, o, d, target, alone = scene(name, base)
    batch = hostile_batch(o, d, target, layout, per)
    R = OracleIntersector(v, f, 1)
    exp = {"closest": R.closest_raw(batch.o, batch.d)[:5], "count": R.intersects_count(batch.o, batch.d),
           "location": R.intersects_location(batch.o, batch.d)}
    hit = exp["closest"][0]
    assert 0.05 <= float(alone["closest"][0].mean()) <= 0.9, (name, float(alone["closest"][0].mean()))
    for k, fam in enumerate(batch.names):
        m = batch.family == k
        assert m.sum() >= 64, (name, fam, int(m.sum()))
        if fam in INVALID or fam in MISS_BY_CONSTRUCTION:
            assert not hit[m].any() and not exp["count"][m].any(), (name, fam)
        else:
            assert hit[m].mean() >= 0.05, (name, fam, float(hit[m].mean()))
    assert batch.mask("scale:126").sum() <= 512
    for x in (batch.o, batch.d, batch.family, batch.src, batch.pos, *exp["closest"], exp["count"], *exp["location"]):
        x.setflags(write=False)
    return batch, exp


# ---- the float64 geometry (tests/geom64.py) on the rays whose hostile component leaves the geometry in place -----------------
# closest_f64 judges robustness in units of the ray parameter (a runner-up hit closer than 1e-4 * max(1, t) makes a ray
# non-robust): with a component of 3e38 every t is ~1e-38 and every ray with a second hit would drop out.  These families
# are handed over with their direction scaled by 2^-126 in float64 -- exact, the same line, the same hit points, t back in
# scene units.
F64_RESCALED = ("comp:3e38", "all:3e38")
F64_RESCALE = 2.0 ** -126


@functools.lru_cache(maxsize=None)
def _content_f64(name, base, per):
    """closest_f64 on the ordinary rays and on families comp: / all: -> (their content indices, hit, tri, loc, robust); the
    same rays in both layouts, so computed once per scene (slices of rays on a few threads: numpy releases the lock)"""
    from concurrent.futures import ThreadPoolExecutor
    from geom64 import closest_f64
    v, f = scene(name, base)[:2]
    batch, _ = expected(name, "interleaved", base, per)
    rays = np.flatnonzero(batch.mask("ordinary", "comp:", "all:"))
    d64 = batch.d.astype(np.float64)
    d64[batch.mask(*F64_RESCALED)] *= F64_RESCALE
    assert np.isfinite(d64[rays]).all() and not np.any((d64[rays] == 0) & (batch.d[rays] != 0))      # (nothing underflowed)
    parts = [rays[k:k + 256] for k in range(0, len(rays), 256)]
    with ThreadPoolExecutor(max_workers=min(8, len(os.sched_getaffinity(0)))) as pool:
        res = list(pool.map(lambda p: closest_f64(v, f, batch.o[p], d64[p], chunk=64), parts))
    hit, tri, _, loc, robust = (np.concatenate([r[k] for r in res]) for k in range(5))
    return batch.order[rays], hit, tri, loc, robust


def geometry_f64(name, layout, base=8192, per=368):
    """the float64 geometry of every ray the rule covers -> (covered, hit, tri, loc, robust, compare loc, {family: its
    rays}) over the batch: the ordinary rays and families comp: / all: themselves; the scaled rays of k >= -10 take their
    base ray's hit, tri and robustness (closest_f64 "called with the unscaled direction"), and their loc is not compared"""
    return _geometry_f64(name, layout, base, per)


@functools.lru_cache(maxsize=None)
def _geometry_f64(name, layout, base, per):
    batch, _ = expected(name, layout, base, per)
    content, h, t, l, rb = _content_f64(name, base, per)
    where = np.empty(batch.n, np.int64)
    where[batch.order] = np.arange(batch.n)
    own = where[content]
    n = batch.n
    covered, hit, tri, loc, robust = np.zeros(n, bool), np.zeros(n, bool), np.full(n, -1, np.int64), np.zeros((n, 3)), np.zeros(n, bool)
    covered[own], hit[own], tri[own], loc[own], robust[own] = True, h, t, l, rb
    with_loc = covered.copy()
    for k in IDENTITY_SCALES:
        rays = batch.members(f"scale:{k}")
        twin = batch.pos[batch.src[rays]]
        covered[rays], hit[rays], tri[rays], robust[rays] = True, hit[twin], tri[twin], robust[twin]
    families = {fam: batch.members(fam) for fam in batch.names if covered[batch.members(fam)].any()}
    assert sum(len(r) for r in families.values()) == covered.sum()
    return covered, hit, tri, loc, robust, with_loc, families


def check_geometry(ref, got_hit, got_tri, got_loc, what):
    """as tests/test_geometry_f64.py: on the robust rays hit and tri exactly, loc within 1e-5 relative (None: the query
    has no such output) -- and the robust rays are more than 0.9 of EVERY covered family, and hold hits in every one whose
    rays hit (the 8192 ordinary rays would carry a share taken over all of them whatever the small families do)"""
    covered, hit, tri, loc, robust, with_loc, families = ref
    for fam, rays in families.items():
        assert robust[rays].mean() > 0.9, f"{what}: {fam}: the robust subset must cover almost all rays ({robust[rays].mean():.3f})"
        # (every finite family hits on 5 % of its rays at least, expected(): with a fifth of those allowed to be non-robust)
        assert (robust[rays] & hit[rays]).mean() >= 0.04, f"{what}: {fam}: {int((robust[rays] & hit[rays]).sum())} robust rays that hit"
    m = covered & robust
    if got_hit is not None:
        assert np.array_equal(got_hit.reshape(-1)[m], hit[m]), f"{what}: hit against the float64 geometry"
    if got_tri is not None:
        assert np.array_equal(got_tri.reshape(-1)[m], tri[m]), f"{what}: tri against the float64 geometry"
    if got_loc is not None:
        m &= hit & with_loc
        np.testing.assert_allclose(got_loc.reshape(-1, 3)[m], loc[m], rtol=1e-5, atol=1e-5, err_msg=what)
