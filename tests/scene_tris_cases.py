"""Shared by tests/test_scene_tris_cpu.py and tests/test_gpu_scene_tris.py (not a test module): the scenes of the triangle
queries on instanced scenes (csrc/tr_scene_tris.h) -- those of tests/scene_cases.py, the overflowing placement of
tests/scene_nearest_cases.py and scenes of small members (1 and 2 triangles, the 12-face cube, the 80-face icosphere, the deep
tree) under 1 to 8 instances --, their query triangles (tests/tris_cases.py pushed through the placements), the brute force of
each computed once, the comparison of two scene_tris_sim.Result, a wave whose lanes meet different instances, and the scene
whose placements are exact in float32 with its integer reference."""
import functools

import numpy as np

import nearest_cases as NC
import scene_cases as SC
import scene_nearest_cases as NN
import tris_cases as TC
import workloads as W

F32 = np.float32
FIELDS = ("any", "count", "offsets", "instance", "face")
ONE, TWO, CUBE, ICO80, DEEP = range(5)
MAX_PLACED = 96      # placed faces of a scene taken as queries, evenly spread


# ---- scenes ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_members():
    """[(vertices, faces)]: one triangle, two triangles (no hierarchy; one node), the 12-face cube, the 80-face icosphere and
    the deep tree (more than 32 levels, 3 000 coincident triangles at the origin among its 3 064)"""
    one = (np.array([[-1.0, -1.0, 0.125], [1.0, -1.0, 0.25], [0.0, 1.5, -0.125]], F32), np.array([[0, 1, 2]], np.int32))
    two = (np.array([[-1, -1, 0], [1, -1, 0.25], [1, 1, 0], [-1, 1, -0.25]], F32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    cv, cf, _ = NC.cube()
    iv, i_f, _ = NC.icosphere()
    dv, df = W.deep_tree_mesh(3000)
    out = [one, two, (cv, cf), (iv, i_f), (np.asarray(dv, F32), np.asarray(df, np.int32))]
    assert [len(f) for _, f in out] == [1, 2, 12, 80, 3064]
    return [(np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32)) for v, f in out]


@functools.lru_cache(maxsize=None)
def small_scenes():
    """name -> (mesh_of, M): 1, 2, 3, 5 and 8 instances of small_members(), overlapping neighbours, a mirror and unequal scales"""
    rng = np.random.default_rng(41)
    out = {}
    out["small1"] = ([ICO80], [SC.placement(SC.general(rng), [0.25, -0.5, 0.125])])
    out["small2"] = ([ONE, TWO], [SC.placement(SC.rotation([1, 0, 1], 0.9), [0, 0, 0]), SC.placement(np.diag([1.0, -2.0, 0.5]), [0.25, 0, 0.1])])
    out["small3"] = ([DEEP, CUBE, ONE], [SC.placement(SC.general(rng, 1.2), [0, 0, 0]), SC.placement(SC.general(rng, 0.7), [0.5, 0.25, 0.5]),
                                         SC.placement(np.eye(3) * 0.5, [0.5, 0.5, 0.5])])
    out["small5"] = ([TWO, ICO80, CUBE, ICO80, ONE],
                     [SC.placement(SC.general(rng), [0.4 * k, 0.1 * k, -0.2 * k]) for k in range(5)])
    mesh_of = [CUBE, ONE, DEEP, TWO, ICO80, CUBE, TWO, ICO80]
    out["small8"] = (mesh_of, [SC.placement(SC.general(rng, 0.8), rng.uniform(-0.6, 0.6, 3)) for _ in mesh_of])
    return {k: (np.asarray(m, np.int32), np.asarray(M, F32)) for k, (m, M) in out.items()}


def names():
    return list(SC.scenes()) + ["overflow"] + list(small_scenes())


def scene_of(name):
    """(members, mesh_of, M [n, 3, 4]) of a scene by name"""
    if name in SC.scenes():
        s = SC.scenes()[name]
        return SC.members(), s["mesh_of"], s["M"]
    if name == "overflow":
        q = NN.overflow_scene()
        return q["members"], q["mesh_of"], q["M"]
    mesh_of, M = small_scenes()[name]
    return small_members(), mesh_of, M


def member_set(name):
    """which list of members the scene draws from: 'scene_cases', 'overflow' or 'small' (the GPU tests build each list once)"""
    return "scene_cases" if name in SC.scenes() else ("overflow" if name == "overflow" else "small")


# ---- queries -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def queries_of(name):
    """[n, 3, 3] float32, read-only: placed faces of the scene itself (they touch by construction), those displaced by a
    fraction of their own size, hashed triangles of three sizes across the scene's world box, triangles larger than the scene,
    and tris_cases.hostile_triangles"""
    import scene_tris_sim as S
    members, mesh_of, M = scene_of(name)
    v, f, inst_of, _ = S.bake(members, mesh_of, M)
    act = NC.active(v, f) if len(f) else np.zeros(0, bool)
    fin = v[f[act]].reshape(-1, 3).astype(np.float64) if act.any() else np.array([[-1.0] * 3, [1.0] * 3])
    parts = []
    if act.any():
        # evenly over the active baked faces of every instance: every instance that offers something is touched
        pick = np.concatenate([np.flatnonzero(act & (inst_of == k))[:: max(1, int((act & (inst_of == k)).sum()) // 12)][:12]
                               for k in np.unique(inst_of[act])])[:MAX_PLACED]
        own = v[f[pick]]
        parts.append(own)
        with np.errstate(over="ignore", invalid="ignore"):
            size = (own.max(1) - own.min(1)).max(1)[:, None, None]
            parts.append((own + size * F32(0.25)).astype(F32)[::2])
    lo, hi = fin.min(0), fin.max(0)
    ext = float(min((hi - lo).max(), 1e30))
    # around the median placed vertex too: under placements of very different scales the world box is mostly empty
    mid = np.median(fin, 0)
    spread = float(np.median(np.abs(fin - mid).max(1))) + 1e-6
    with np.errstate(over="ignore", invalid="ignore"):
        parts.append(TC.hashed_triangles(150, lo - 0.1 * ext, hi + 0.1 * ext, ext, seed=5))
        parts.append(TC.hashed_triangles(150, mid - 2 * spread, mid + 2 * spread, 2 * spread, seed=9))
        parts.append(TC.larger_than(np.clip(fin, -1e30, 1e30)))
        hostile = TC.hostile_triangles(TC.hashed_triangles(40, mid - spread, mid + spread, spread, seed=13))[0]
    parts.append(hostile)
    tri = np.ascontiguousarray(np.concatenate([np.asarray(p, F32).reshape(-1, 3, 3) for p in parts]), F32)
    tri.setflags(write=False)
    return tri


@functools.lru_cache(maxsize=None)
def brute_of(name):
    """scene_tris_sim.brute of scene `name` on queries_of(name): computed once per process and never changed"""
    import scene_tris_sim as S
    members, mesh_of, M = scene_of(name)
    with np.errstate(all="ignore"):
        res = S.brute(members, mesh_of, M, queries_of(name))
    for a in res:
        a.setflags(write=False)
    return res


def assert_same(got, want, what):
    """two scene_tris_sim.Result (or tuples laid out like one; None entries of `got` are skipped), element for element"""
    for name, g, w in zip(FIELDS, got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, expected {w.shape}"
        assert g.dtype == w.dtype, f"{what}: {name} has type {g.dtype}, expected {w.dtype}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {name} differs at {bad[:8]} ({len(bad)} of {len(g)}): {g[bad[:4]]} != {w[bad[:4]]}")


def check_identities(res, what):
    """what holds for any Result whatever the scene: any == (count > 0), count == diff(offsets), rows strictly ascending by
    (instance, face) within a query"""
    assert np.array_equal(res.any, res.count > 0), what
    assert np.array_equal(res.count, np.diff(res.offsets)), what
    assert len(res.face) == len(res.instance) == res.offsets[-1] and res.offsets[0] == 0, what
    if len(res.face) > 1:
        key = res.instance.astype(np.int64) * (1 << 32) + res.face
        inner = np.ones(len(key) - 1, bool)
        starts = res.offsets[1:-1]
        inner[starts[(starts > 0) & (starts < len(key))] - 1] = False
        assert (np.diff(key)[inner] > 0).all(), f"{what}: a list is not strictly ascending by (instance, face)"


def renumbered(res, order):
    """the Result of a scene whose instances were LISTED in `order` (listing j holds instance order[j]) with the instances
    named as in the original listing and each query's rows sorted again"""
    order = np.asarray(order)
    inst = order[res.instance].astype(np.int32)
    q = np.repeat(np.arange(len(res.count)), res.count)
    perm = np.lexsort((res.face, inst, q))
    return type(res)(res.any, res.count, res.offsets, inst[perm], res.face[perm])


def check_fixture_conditions():
    """the inputs reach the edges the comparisons are about; asserted from the brute force"""
    two = single = none = twice = 0
    for name in names():
        w = brute_of(name)
        check_identities(w, name)
        tri = queries_of(name)
        valid = np.isfinite(tri).all(axis=(1, 2))
        assert (~valid).sum() >= 27 and not w.any[~valid].any(), name
        for i in np.flatnonzero(w.count > 1):
            rows = w.instance[w.offsets[i]:w.offsets[i + 1]]
            two += len(np.unique(rows)) >= 2
            twice += (np.bincount(rows) >= 2).any()
        single += int((w.count == 1).sum())
        none += int((valid & ~w.any).sum())
        if name != "none":
            assert w.any.any() and not w.any.all(), f"{name}: every answer is the same"
            members, mesh_of, M = scene_of(name)
            touched = np.unique(w.instance)
            assert len(touched) >= min(2, len(mesh_of)), f"{name}: instances {touched} only"
    assert not brute_of("none").any.any() and brute_of("none").offsets[-1] == 0
    assert two > 50 and twice > 50 and none > 50 and single > 5, (two, twice, none, single)
    # a mirrored placement and a non-uniform scale occur
    dets, uneven = [], 0
    for name in names():
        for M in scene_of(name)[2]:
            L = np.asarray(M, np.float64)[:, :3]
            if np.isfinite(L).all():
                dets.append(np.linalg.det(L))
                s = np.linalg.svd(L, compute_uv=False)
                uneven += s[-1] > 0 and s[0] / s[-1] > 1.5
    assert min(dets) < 0 < max(dets) and uneven > 10
    # odd: the singular (3), NaN (4), inactive (5) and faceless (6) instances are never met; the mirrored, tiny and huge are
    odd = brute_of("odd").instance
    assert not np.isin(odd, (3, 4, 5, 6)).any() and all((odd == k).any() for k in (0, 1, 2, 7))
    # overflow: the large copy's faces (inactive once placed) are never met, the small copy's and the second instance's are
    q = NN.overflow_scene()
    nf = len(q["members"][0][1]) // 2
    ov = brute_of("overflow")
    assert not ((ov.instance == 0) & (ov.face < nf)).any() and ((ov.instance == 0) & (ov.face >= nf)).any() and (ov.instance == 1).any()


# ---- a wave whose lanes meet different instances ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def split_wave():
    """(mesh_of, M, triangles, the brute force) on small_members(): two triangles, the icosphere and the cube in a row, 10
    apart.  Query i < 192 is a placed face of instance i mod 3, so its only contacts are there.  Queries 192 .. 199 are long
    triangles along the row that cut through instances 0 AND 1: instance 0 has no hierarchy to overflow in, so a stack of one
    entry that overflows does so in instance 1, after the pairs of instance 0 were found."""
    import scene_tris_sim as S
    rng = np.random.default_rng(6)
    mesh_of = np.array([TWO, ICO80, CUBE], np.int32)
    M = np.array([SC.placement(SC.rotation([0, 1, 0], 0.3), [-10, 0, 0]), SC.placement(SC.general(rng, 0.9), [0, 0, 0]),
                  SC.placement(SC.general(rng, 0.9), [10, 0, 0])], F32)
    v, f, inst_of, _ = S.bake(small_members(), mesh_of, M)
    own = [v[f[inst_of == k]] for k in range(3)]
    lanes = np.stack([own[i % 3][(i // 3) % len(own[i % 3])] for i in range(192)])
    long_ = np.array([[[-11.5, -0.3 + 0.05 * j, -0.4], [1.5, 0.2, 0.3 + 0.02 * j], [-11.5, 0.4, 0.35 - 0.03 * j]] for j in range(8)], F32)
    tri = np.ascontiguousarray(np.concatenate([lanes, long_]), F32)
    want = S.brute(small_members(), mesh_of, M, tri)
    for i in range(192):
        rows = want.instance[want.offsets[i]:want.offsets[i + 1]]
        assert len(rows) and (rows == i % 3).all(), i
    for i in range(192, 200):
        rows = want.instance[want.offsets[i]:want.offsets[i + 1]]
        assert (rows == 0).any() and (rows == 1).sum() >= 2 and not (rows == 2).any(), (i, rows)
    return mesh_of, M, tri, want


# ---- placements that are exact in float32 ------------------------------------------------------------------------------------------
# the signed permutations of scene_cases.lattice_scene() with power-of-two scales; scales 1 / 2 and 1 and translations chosen so that
# the placed coordinates stay EVEN multiples of 2^-10 within [-1, 1]: tris_cases.lattice_triangles and the exactness bound of
# csrc/tr_tris.h (|k| <= 2^11 with the steps the queries add) hold on the baked mesh
_EXACT_INSTANCES = (("cube", 0, (1, 2), (-256, 128, 0)), ("icosphere", 1, (1, 1), (256, -128, 64)), ("flat", 2, (1, 1), (0, 384, -256)),
                    ("cube", 3, (1, 1), (-384, -384, 256)), ("flat", 4, (1, 2), (128, -64, 384)))
EXACT_QUERIES = 240


@functools.lru_cache(maxsize=None)
def exact_scene():
    """dict(members, mesh_of, M, v, f: the INTEGER-baked mesh as float32 (int64 arithmetic, no chain), face_base, tri, met,
    touching, coplanar [n, F]): tris_cases.snapped_meshes() placed by signed permutations, scales 1 / 2 and 1 and grid
    translations, queries drawn by tris_cases.lattice_triangles from the baked mesh, and tris_cases.exact_tables (integer
    arithmetic that shares nothing with csrc/tr_tris.h) on it"""
    snapped = TC.snapped_meshes()
    names_ = list(snapped)
    perms = [SC._signed_perm(*inst[1]) for inst in SC._LATTICE_INSTANCES]
    members = [snapped[n] for n in names_]
    mesh_of, Ms, vs, fs, base = [], [], [], [], []
    nv = nf = 0
    for name, p, scale, t in _EXACT_INSTANCES:
        P = perms[p]
        v, f = snapped[name]
        k = TC.snapped(v)
        num, den = scale
        scaled = (k @ P.T) * num
        assert (scaled % den == 0).all(), name
        w = scaled // den + np.asarray(t, np.int64)
        assert (w % 2 == 0).all() and np.abs(w).max() <= 1024
        Ms.append(SC.placement(P.astype(np.float64) * (num / den), np.asarray(t, np.float64) / TC.GRID))
        mesh_of.append(names_.index(name))
        vs.append(w); fs.append(np.asarray(f, np.int64) + nv); base.append(nf)
        nv += len(w); nf += len(f)
    v = (np.concatenate(vs) / TC.GRID).astype(F32)
    f = np.concatenate(fs).astype(np.int32)
    assert any(round(np.linalg.det(perms[i[1]])) < 0 for i in _EXACT_INSTANCES) and any(round(np.linalg.det(perms[i[1]])) > 0 for i in _EXACT_INSTANCES)
    tri = TC.lattice_triangles(v, f, EXACT_QUERIES, seed=700, kinds=(0, 1, 2, 3, 2))
    met, touching, cop = TC.exact_tables(v, f, tri)
    out = dict(members=members, mesh_of=np.array(mesh_of, np.int32), M=np.array(Ms, F32), v=v, f=f, face_base=np.array(base), tri=tri,
               met=met, touching=touching, coplanar=cop)
    for a in (v, f, tri, met, touching, cop):
        a.setflags(write=False)
    return out


def listed(res, n, face_base, nf):
    """[n, nf] bool: baked face face_base[instance] + face is in the list of query i"""
    got = np.zeros((n, nf), bool)
    got[np.repeat(np.arange(n), res.count), np.asarray(face_base)[res.instance] + res.face] = True
    return got


def check_exact(res, what):
    """a Result on exact_scene() against the integer reference, pair by pair; asserts that coplanar and only-touching pairs
    occur among the meeting ones.  -> (pairs, met, only touching, coplanar and met)"""
    E = exact_scene()
    got = listed(res, len(E["tri"]), E["face_base"], len(E["f"]))
    bad = np.argwhere(got != E["met"])
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} pairs differ from the exact reference, the first (query, baked face) {bad[:4].tolist()}"
    assert np.array_equal(res.count, E["met"].sum(1)) and np.array_equal(res.any, E["met"].any(1)), what
    check_identities(res, what)
    stats = (int(got.size), int(E["met"].sum()), int(E["touching"].sum()), int((E["coplanar"] & E["met"]).sum()))
    assert stats[1] > 300 and stats[2] > 60 and stats[3] > 30, stats
    touched = np.unique(res.instance)
    assert len(touched) == len(E["mesh_of"]), f"{what}: instances {touched} only"
    return stats
