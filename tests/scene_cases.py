"""Shared by tests/test_scene_cpu.py and tests/test_gpu_scene.py (not a test module): the members, placements, rays and
bounds of the instanced-scene checks (csrc/tr_scene.h), the lattice scene whose transforms are exact in float32, and the
second, numpy, computation of the brute force."""
import functools
from fractions import Fraction

import numpy as np

import exact_ref
import hostile_meshes as HM
import range_cases as RC

KEYS_ANY = ("any",)
KEYS_CLOSEST = ("hit", "front", "instance", "tri", "loc", "uv", "t")
KEYS = KEYS_ANY + KEYS_CLOSEST
ICO, SHELLS, TRI, INACTIVE, NOFACES = range(5)
F32 = np.float32


@functools.lru_cache(maxsize=None)
def members():
    """[(vertices, faces)]: RC.icosphere (1 280 triangles), RC.shells5 (1 600), one triangle, a mesh whose twelve faces all
    have a non-finite coordinate (zero active faces) and a mesh without faces"""
    iv, if_ = RC.icosphere()[:2]
    sv, sf = RC.shells5()[:2]
    tv = np.array([[-1.0, -1.0, 0.1], [1.0, -1.0, 0.2], [0.0, 1.5, -0.1]], F32)
    tf = np.array([[0, 1, 2]], np.int32)
    c = HM.case("all_inactive", 0)
    assert len(c.f) == 12 and c.inactive.all()
    return [(iv, if_), (sv, sf), (tv, tf), (np.array(c.v), np.array(c.f)), (iv[:3].copy(), np.zeros((0, 3), np.int32))]


def placement(lin, t):
    M = np.zeros((3, 4), F32)
    M[:, :3] = np.asarray(lin, np.float64)
    M[:, 3] = t
    return M


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def general(rng, scale=1.0):
    """a general affine linear part: rotation x shear x unequal scales, determinant of either sign away from zero"""
    R = rotation(rng.normal(size=3), rng.uniform(0, 2 * np.pi))
    S = np.diag(rng.uniform(0.6, 1.6, 3) * scale)
    H = np.eye(3)
    H[0, 1], H[1, 2] = rng.uniform(-0.4, 0.4, 2)
    return R @ H @ S


def world_box(v, M):
    """box of the placed finite vertices of a member (float64)"""
    v = np.asarray(v, np.float64)
    v = v[np.isfinite(v).all(1)]
    w = v @ np.asarray(M, np.float64)[:, :3].T + np.asarray(M, np.float64)[:, 3]
    return w.min(0), w.max(0)


def _scene(name, mesh_of, Ms, regions=None, rays_per_region=1500, seed=1):
    mesh_of = np.asarray(mesh_of, np.int32).reshape(-1)
    Ms = np.asarray(Ms, F32).reshape(-1, 3, 4)
    mem = members()
    if regions is None:      # one region: the world extent of the instances that can be hit
        boxes = [world_box(mem[m][0], M) for m, M in zip(mesh_of, Ms)
                 if len(mem[m][1]) and m != INACTIVE and np.isfinite(M).all() and abs(np.linalg.det(M[:, :3].astype(np.float64))) > 0]
        lo = np.min([b[0] for b in boxes], 0) if boxes else -np.ones(3)
        hi = np.max([b[1] for b in boxes], 0) if boxes else np.ones(3)
        regions = [(lo, hi)]
    o, d, lo_, hi_ = [], [], [], []
    for k, (lo, hi) in enumerate(regions):
        box = np.stack([np.asarray(lo, F32), np.asarray(hi, F32)])
        ro, rd, rlo, rhi = RC.rays_in_box(box, rays_per_region, seed + 7 * k)
        o.append(ro); d.append(rd); lo_.append(rlo); hi_.append(rhi)
    ho, hd, hlo, hhi, bad = RC.hostile_rays(o[0], d[0], lo_[0], hi_[0])
    o, d, lo_, hi_ = (np.ascontiguousarray(np.concatenate(x + [h])) for x, h in ((o, ho), (d, hd), (lo_, hlo), (hi_, hhi)))
    nbad = np.concatenate([np.zeros(len(o) - len(bad), bool), bad])
    return dict(name=name, mesh_of=mesh_of, M=Ms, o=o, d=d, lo=lo_, hi=hi_, bad=nbad)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(mesh_of, M [n, 3, 4], o, d, lo, hi, bad): instance counts 0, 1, 2, 3 and 65; overlapping and
    interpenetrating placements, two instances with the same placement, general affine maps, a mirror, scales 2^-20 and
    2^20, a singular M and an M with a NaN, members without a triangle that can be hit"""
    rng = np.random.default_rng(2024)
    out = {}
    out["none"] = _scene("none", [], np.zeros((0, 3, 4)))
    out["one_affine"] = _scene("one_affine", [ICO], [placement(general(rng), [0.3, -0.2, 0.1])])
    same = placement(rotation([1, 2, 3], 0.7) * 1.25, [0.5, 0.25, -0.125])
    out["two_same"] = _scene("two_same", [ICO, ICO], [same, same])
    out["three"] = _scene("three", [ICO, SHELLS, TRI],
                          [placement(np.eye(3), [0.4, 0, 0]), placement(general(rng, 0.8), [-0.3, 0.2, 0.1]),      # interpenetrating
                           placement(rotation([0, 1, 0], 1.1) * 1.5, [0.1, 0.1, 0.2])])
    # a mirror, tiny and huge copies, and instances that nothing can hit; rays around each scale
    mirror = placement(np.diag([-1.0, 1.0, 1.0]) @ rotation([1, 1, 0], 0.4), [0.2, 0.0, -0.1])
    tiny = placement(np.eye(3) * 2.0 ** -20, [0.25, 0.5, -0.75])
    huge = placement(rotation([0, 0, 1], 0.3) * 2.0 ** 20, [3.0, -5.0, 7.0])
    singular = placement([[1, 2, 3], [2, 4, 6], [0, 1, 1]], [0, 0, 0])
    withnan = placement(np.eye(3), [0, np.nan, 0])
    mem = members()
    regions = [world_box(mem[ICO][0], mirror), world_box(mem[ICO][0], tiny), world_box(mem[ICO][0], huge)]
    out["odd"] = _scene("odd", [ICO, ICO, ICO, SHELLS, ICO, INACTIVE, NOFACES, TRI],
                        [mirror, tiny, huge, singular, withnan, placement(np.eye(3), [0, 0, 0]), placement(np.eye(3), [0, 0, 0]),
                         placement(np.diag([1.0, -1.0, 1.0]), [0.1, 0.2, 0.3])], regions=regions, rays_per_region=1000)
    # 65 instances on a jittered 5 x 5 x 3 grid (overlapping neighbours): mostly single triangles, some spheres and shells
    mesh_of, Ms = [], []
    for k in range(65):
        cell = np.array([k % 5, (k // 5) % 5, k // 25], np.float64) * 1.6 + rng.uniform(-0.3, 0.3, 3)
        m = ICO if k % 9 == 0 else SHELLS if k % 16 == 5 else INACTIVE if k == 33 else NOFACES if k == 47 else TRI
        if k == 51:
            Ms.append(singular)
        else:
            Ms.append(placement(general(rng, 0.9), cell))
        mesh_of.append(m)
    out["many65"] = _scene("many65", mesh_of, Ms, rays_per_region=2500)
    assert [len(s["mesh_of"]) for s in out.values()] == [0, 1, 2, 3, 8, 65]
    return out


def reversed_scene(s):
    """the same instances listed in reverse order"""
    r = dict(s)
    r["mesh_of"], r["M"] = np.ascontiguousarray(s["mesh_of"][::-1]), np.ascontiguousarray(s["M"][::-1])
    return r


def exact_bounds(want, lo, hi):
    """bounds placed exactly on the hits of a brute force: tmax = t on the even hit rays, tmin = t on the odd ones, no
    other bound.  The float32 distance then lies in the band of the bound and the float64 part decides the hit."""
    lo, hi = lo.copy(), hi.copy()
    idx = np.flatnonzero(want["hit"])
    lo[:], hi[:] = 0, np.inf
    hi[idx[::2]] = want["t"][idx[::2]]
    lo[idx[1::2]] = want["t"][idx[1::2]]
    return lo, hi


def numpy_brute(mem, mesh_of, M, o, d, lo, hi):
    """the second computation: range_sim.brute per instance on the rays of scene_sim.transform, reduced in numpy by
    (t, instance, face); loc through scene_sim.points, front inverted under a mirror"""
    import range_sim
    import scene_sim
    n = len(o)
    out = dict(any=np.zeros(n, bool), hit=np.zeros(n, bool), front=np.zeros(n, bool), instance=np.full(n, -1, np.int32),
               tri=np.full(n, -1, np.int32), t=np.full(n, np.inf, F32), loc=np.zeros((n, 3), F32), uv=np.zeros((n, 2), F32))
    W_, valid, flip = scene_sim.record(M) if len(mesh_of) else (None, [], [])
    with np.errstate(invalid="ignore"):
        world_ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    for k in range(len(mesh_of)):
        v, f = mem[mesh_of[k]]
        if not valid[k] or len(f) == 0:
            continue
        o2, d2, ok = scene_sim.transform(M[k], o, d)
        ok &= world_ok
        r = range_sim.brute(v, f, o2, d2, lo, hi)
        better = ok & r["hit"] & (r["t"] < out["t"])      # ascending instance order: only strictly nearer displaces
        out["any"] |= ok & r["any"]
        out["hit"] |= better
        out["front"][better] = r["front"][better] != flip[k]
        out["instance"][better] = k
        out["tri"][better] = r["tri"][better]
        out["t"][better] = r["t"][better]
        out["uv"][better] = r["uv"][better]
        out["loc"][better] = scene_sim.points(M[k], r["loc"][better])
    return out


# ---- the lattice scene: transforms that are exact in float32 ------------------------------------------------------------
def _signed_perm(perm, signs):
    P = np.zeros((3, 3), np.int64)
    for row, (col, s) in enumerate(zip(perm, signs)):
        P[row, col] = s
    return P


# (member scene of exact_ref.lattice_scenes, signed permutation, scale = num / den a power of two, integer translation)
_LATTICE_INSTANCES = (
    ("cube2", ((0, 1, 2), (-1, 1, 1)), (1, 4), (14, 2, 2)),          # a mirror: x -> -x
    ("cube5", ((1, 2, 0), (1, 1, 1)), (1, 4), (24, 2, 4)),           # a rotation
    ("heightfield", ((0, 1, 2), (1, 1, -1)), (2, 1), (2, 24, 46)),   # a mirror in z, scaled up
    ("cube2", ((2, 0, 1), (1, -1, -1)), (1, 2), (40, 42, 24)),       # the first member again, a proper rotation
    ("cube1", ((1, 0, 2), (1, 1, 1)), (1, 8), (44, 4, 50)),          # a swap of x and y: a mirror
)


@functools.lru_cache(maxsize=None)
def lattice_scene():
    """dict(members [(v, f)], mesh_of, M [n, 3, 4] float32, v, f: the baked integer mesh (instance order), face_base [n]: the
    baked index of each instance's face 0, boxes [n, 2, 3], o, d: integer rays, ideal: exact_ref.lattice on the baked mesh,
    inst_of_face, perms [n]: the signed permutation of each placement).  EVERY candidate ray below is kept, the ones on which the ideal rule meets a triangle through an edge or a
    vertex (ideal.tie, about 8 %) included: check_against_ideal says what is asserted on those."""
    by_name = {s["name"]: s for s in exact_ref.lattice_scenes()}
    names = []
    for name, *_ in _LATTICE_INSTANCES:
        if name not in names:
            names.append(name)
    mem = [(by_name[n]["v"], by_name[n]["f"]) for n in names]
    mesh_of, Ms, vs, fs, base, boxes, perms = [], [], [], [], [], [], []
    nv = nf = 0
    for name, (perm, signs), (num, den), t in _LATTICE_INSTANCES:
        P = _signed_perm(perm, signs)
        v, f = by_name[name]["v"].astype(np.int64), by_name[name]["f"].astype(np.int64)
        scaled = (v @ P.T) * num
        assert (scaled % den == 0).all(), name
        w = scaled // den + np.asarray(t, np.int64)
        Ms.append(placement(P.astype(np.float64) * (num / den), t))
        mesh_of.append(names.index(name))
        perms.append(P)
        vs.append(w); fs.append(f + nv); base.append(nf)
        boxes.append((w.min(0), w.max(0)))
        nv += len(w); nf += len(f)
    v, f = np.concatenate(vs), np.concatenate(fs)
    boxes = np.array(boxes)
    assert v.min() >= 0 and v.max() <= 64, "the world extent stays within 64 units"
    for a in range(len(boxes)):
        for b in range(a):
            gap = np.maximum(boxes[a][0] - boxes[b][1], boxes[b][0] - boxes[a][1]).max()
            assert gap >= 1, f"instances {a} and {b} are {gap} apart"
    # candidate rays: from integer origins between and around the instances towards the centroids (x 3), towards points of
    # the faces off their centroid, along small random integer directions, and -- exact ties on purpose -- from one origin between
    # the instances and one outside, through every vertex and every edge midpoint (x 2)
    rng = np.random.default_rng(77)
    origins = np.array([(32, 20, 30), (20, 16, 20), (8, 40, 20), (50, 30, 45), (-60, 30, 20), (33, -90, 41), (30, 31, 140), (100, 90, -40)], np.int64)
    tri = v[f]
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    os_, ds = [], []
    for k, o in enumerate(origins):
        cent = tri.sum(1) - 3 * o
        pick = rng.integers(0, len(f), 400)
        wts = rng.integers(1, 6, (400, 3))
        off = (tri[pick] * wts[:, :, None]).sum(1) - wts.sum(1, keepdims=True) * o      # (a point of the face, scaled by the weights' sum)
        rnd = rng.integers(-9, 10, (300, 3))
        dd = np.concatenate([cent, off, rnd] + ([v - o, v[edges[:, 0]] + v[edges[:, 1]] - 2 * o] if k in (0, 4) else []))
        dd = dd[(np.abs(dd).max(1) > 0) & (np.abs(dd).max(1) < 256)]
        os_.append(np.tile(o, (len(dd), 1))); ds.append(dd)
    o, d = np.concatenate(os_), np.concatenate(ds)
    assert np.abs(o).max() <= 256
    ideal = exact_ref.lattice(v, f, o, d)
    assert len(o) > 8000 and ideal.tie.sum() > 2000 and (~ideal.tie).sum() > 7000
    inst_of_face = np.repeat(np.arange(len(base)), np.diff(base + [nf]))
    return dict(members=mem, mesh_of=np.array(mesh_of, np.int32), M=np.array(Ms, F32), v=v, f=f, face_base=np.array(base), boxes=boxes,
                o=o.astype(F32), d=d.astype(F32), ideal=ideal, inst_of_face=inst_of_face, perms=perms)


def exact_distances(v, f, o, d, faces):
    """the exact t of ray (o, d) on the planes of `faces` of the integer mesh, as float64 quotients of exact int64s"""
    a, b, c = (v[f[faces, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    return ((a - o) * nrm).sum(1) / (d * nrm).sum(1)


def check_lattice_separation(L):
    """from the ideal's sets: the exact distances of any two accepted hits of one ray in DIFFERENT instances differ by at
    least 2^-8 relative (four times the 2^-11 bound on a float32 distance), on every ray"""
    vi, fi = L["v"], L["f"]
    oi, di = L["o"].astype(np.int64), L["d"].astype(np.int64)
    worst, pairs = np.inf, 0
    for i, s in enumerate(L["ideal"].sets):
        inst = L["inst_of_face"][s]
        if len(set(inst.tolist())) < 2:
            continue
        t = exact_distances(vi, fi, oi[i], di[i], s)
        for a in range(len(s)):
            for b in range(a):
                if inst[a] != inst[b]:
                    pairs += 1
                    worst = min(worst, abs(t[a] - t[b]) / max(t[a], t[b]))
    assert pairs > 100 and worst >= 2.0 ** -8, f"{pairs} pairs across instances, nearest {worst:.3g} relative"
    return pairs, worst


def met_faces(v, f, o, d):
    """the faces of the integer mesh that the ray (o, d) meets at some t >= 0 in their interior, ON AN EDGE OR AT A VERTEX --
    the inside test without the ownership rule, in a form that names no projection: the scalar triple products
    U = d . ((b - o) x (c - o)), V = d . ((c - o) x (a - o)), W = d . ((a - o) x (b - o)) are the edge functions up to one
    common factor; inside or on the border iff no two of them have strictly opposite signs and U + V + W != 0.  Exact in
    int64 (|P - o| < 2^9, |d| < 2^8).  -> dict(met [F], edge [F]: met with a zero edge function, tn, td [F]: the exact t as
    numerator / denominator with td > 0, facing [F]: sign of d . n, inplane [F]: the ray lies in the face's plane)"""
    a, b, c = (v[f[:, k]] - o for k in range(3))
    U, V, W_ = ((d * np.cross(x, y)).sum(1) for x, y in ((b, c), (c, a), (a, b)))
    det = U + V + W_
    neg, pos = (U < 0) | (V < 0) | (W_ < 0), (U > 0) | (V > 0) | (W_ > 0)
    nrm = np.cross(b - a, c - a)
    tn, td = (a * nrm).sum(1), (d * nrm).sum(1)
    sg = np.sign(td)
    met = ~(neg & pos) & (det != 0) & (td != 0) & (tn * sg >= 0)
    return dict(met=met, edge=met & ((U == 0) | (V == 0) | (W_ == 0)), tn=tn * sg, td=td * sg, facing=sg,
                inplane=(U == 0) & (V == 0) & (W_ == 0))


@functools.lru_cache(maxsize=None)
def lattice_frame_ideal():
    """The ideal rule IN EACH INSTANCE'S OWN FRAME, for the tie rays of lattice_scene(): what the contract promises there.
    Which triangle around an edge or a vertex owns it -- and at a silhouette, at the rim of an open patch or beside a triangle
    that holds the ray in its plane, whether ANY does -- is decided in the projected frame of the ray (tr_math.h, "exact ties"),
    and the scene applies the rule to the OBJECT-space ray.  The rule reads P - o and d only and every sign in it is unchanged
    by a positive common scale, so the object-space rule of instance k is the rule on the world-space integers turned by the
    signed permutation of its placement alone: exact_ref.lattice on (v P, o P, d P) with the faces of instance k.  Integer
    numpy throughout, no code of csrc/.  -> (rays [m]: indices of the tie rays, hit [m], nearest [m]: baked face or -1,
    alt [m], front [m]: as the WORLD sees the placed face)"""
    L = lattice_scene()
    vi, fi = L["v"], L["f"]
    rays = np.flatnonzero(L["ideal"].tie)
    oi, di = L["o"].astype(np.int64)[rays], L["d"].astype(np.int64)[rays]
    m = len(rays)
    best_t = [None] * m
    nearest, alt, front = np.full(m, -1, np.int64), np.full(m, -1, np.int64), np.zeros(m, bool)
    ends = list(L["face_base"][1:]) + [len(fi)]
    for k, (P, lo, hi) in enumerate(zip(L["perms"], L["face_base"], ends)):
        ideal = exact_ref.lattice(vi @ P, fi[lo:hi], oi @ P, di @ P)
        flip = round(np.linalg.det(P)) < 0
        for j in np.flatnonzero(ideal.nearest >= 0):
            g = lo + int(ideal.nearest[j])
            a, b, c = (vi[fi[g, q]] for q in range(3))
            nrm = np.cross(b - a, c - a)
            t = Fraction(int(((a - oi[j]) * nrm).sum()), int((di[j] * nrm).sum()))
            if best_t[j] is None or t < best_t[j]:      # (instances in ascending order: an equal distance does not displace)
                best_t[j], nearest[j], front[j] = t, g, bool(ideal.front[j]) != flip
                alt[j] = lo + int(ideal.alt[j]) if ideal.alt[j] >= 0 else -1
    return rays, nearest >= 0, nearest, alt, front


def check_against_ideal(L, got, what):
    """Every ray is compared.
    Rays on which the ideal rule on the baked mesh meets no triangle through an edge or a vertex (~ideal.tie): the hit mask
    EQUALS the ideal's, (instance, tri) as a baked face index equals nearest, or alt where there is one, front equals the
    ideal's.
    Rays that do (ideal.tie): the owner of an edge or a vertex depends on the projected frame, which a signed permutation
    changes -- so they are held, just as strictly (mask, face, front EQUAL), to the same integer rule evaluated in each
    instance's own frame (lattice_frame_ideal), and to what no frame can change: the named baked face is one the ray really
    meets, in its interior, on an edge or at a vertex (met_faces).
    On every ray with a hit, front is the exact orientation of the NAMED face, sign(d . n) in integers.
    -> (tie rays, tie rays on which the baked mesh's ideal names another face, tie rays on which its hit mask differs)"""
    ideal = L["ideal"]
    vi, fi = L["v"], L["f"]
    oi, di = L["o"].astype(np.int64), L["d"].astype(np.int64)
    hit, tie = ideal.nearest >= 0, ideal.tie
    differs = got["hit"] != hit
    assert not (differs & ~tie).any(), f"{what}: hit mask differs on {int((differs & ~tie).sum())} rays without a tie, first {np.flatnonzero(differs & ~tie)[:8]}"
    if got.get("any") is not None:
        assert np.array_equal(got["any"], got["hit"]), f"{what}: any differs from hit"
    baked = np.where(got["hit"], L["face_base"][np.maximum(got["instance"], 0)] + got["tri"], -1)
    full = (baked == ideal.nearest) | ((ideal.alt >= 0) & (baked == ideal.alt))
    assert full[~tie].all(), f"{what}: {int((~full & ~tie).sum())} rays without a tie name another triangle, first {np.flatnonzero(~full & ~tie)[:8]}"
    same = baked == ideal.nearest
    assert np.array_equal(got["front"][same & ~tie], ideal.front[same & ~tie]), f"{what}: front differs"
    assert (got["instance"][~got["hit"]] == -1).all() and (got["tri"][~got["hit"]] == -1).all() and not got["front"][~got["hit"]].any()
    # front: the exact orientation of the named face, on every ray with a hit
    h = np.flatnonzero(got["hit"])
    a, b, c = (vi[fi[baked[h], k]] for k in range(3))
    facing = (di[h] * np.cross(b - a, c - a)).sum(1) < 0
    assert np.array_equal(got["front"][h], facing), f"{what}: front is not the orientation of the named face on {int((got['front'][h] != facing).sum())} rays"
    # the tie rays: the rule in each instance's frame, and the frame-free fact
    rays, fhit, fnearest, falt, ffront = lattice_frame_ideal()
    assert np.array_equal(rays, np.flatnonzero(tie))
    bad = got["hit"][rays] != fhit
    assert not bad.any(), f"{what}: hit mask differs from the rule in the instances' frames on {int(bad.sum())} tie rays, first {rays[bad][:8]}"
    ok = (baked[rays] == fnearest) | ((falt >= 0) & (baked[rays] == falt))
    assert ok.all(), f"{what}: {int((~ok).sum())} tie rays name another triangle than the rule in the instances' frames, first {rays[~ok][:8]}"
    agree = baked[rays] == fnearest
    assert np.array_equal(got["front"][rays][agree], ffront[agree]), f"{what}: front differs on tie rays"
    for i in rays[got["hit"][rays]]:
        assert met_faces(vi, fi, oi[i], di[i])["met"][baked[i]], f"{what}: ray {i} (a tie) names face {baked[i]}, which it does not meet"
    for k in range(len(L["mesh_of"])):
        assert (got["instance"] == k).sum() > 50, f"{what}: instance {k} is hardly ever the nearest"
    return int(tie.sum()), int((tie & ~full).sum()), int((tie & differs).sum())


@functools.lru_cache(maxsize=None)
def brute_of(name, kind):
    """(lo, hi, scene_sim.brute) of scenes()[name] under the bounds `kind`: 'none', 'hash' (the scene's own) or 'exact'
    (placed on the hits of the unbounded brute force), computed once"""
    import scene_sim
    s = scenes()[name]
    if kind == "none":
        lo = hi = None
    elif kind == "hash":
        lo, hi = s["lo"], s["hi"]
    else:
        lo, hi = exact_bounds(brute_of(name, "none")[2], s["lo"], s["hi"])
    return lo, hi, scene_sim.brute(members(), s["mesh_of"], s["M"], s["o"], s["d"], lo, hi)
