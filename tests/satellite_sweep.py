"""Shared by tests/test_satellite_sweep_cpu.py, tests/test_gpu_satellite_sweep.py and scripts/fuzz_satellites.py (not a test
module): the generator and the family table of the randomised parity sweep of the fourteen satellite query libraries.

draw(family, seed, iteration) is a deterministic function: a random mesh of one of eight kinds (the kind is iteration % 8, the
seed decides the parameters only), scaled and shifted, a batch of queries from the generators of the *_cases modules, the
family's knobs, and in every second iteration displaced vertices for one refit.  TABLE[family] says how to get the host brute
force, the host walk (tests/host_sim) and every native entry of the family once; the comparators are the families' own.
Nothing here is a new oracle: brute forces, walks, natives and comparators are imported from the modules that own them."""
import numpy as np

import boxes_cases as BC
import cross_cases as CC
import nearest_cases as NC
import planes_cases as PC
import range_cases as RC
import scene_cases as SC
import scene_cross_cases as XC
import scene_nearest_cases as NN
import scene_points_cases as SPC
import scene_tris_cases as ST
import tri_nearest_cases as TN
import tris_cases as TC
import within_cases as WC
import workloads as W

# (draw() seeds its generator with the family's index: a new family goes to the END, so that the cases of the others stay)
FAMILIES = ("points", "nearest", "range", "within", "cross", "boxes", "tris", "planes", "scene", "scene_cross", "scene_points", "scene_nearest",
            "tri_nearest", "scene_tris")
SCENES = ("scene", "scene_cross", "scene_points", "scene_nearest", "scene_tris")
KINDS = ("few", "icosphere", "soup", "shells", "displaced", "deep", "flat", "holed")      # (a) .. (h) of the sweep
CLOSED_KINDS = (1, 3, 4)
MAX_TRIS, MAX_MEMBER_TRIS, MAX_QUERIES, MAX_INSTANCES = 1500, 400, 700, 70
EDGE_BATCHES = (1, 63, 64, 65, 127, 128, 129)
EDGE_INSTANCES = (1, 2, 63, 64, 65, 70)
ANISOTROPIC = np.array([1.0, 1.0 / 64.0, 16.0])
COARSE_OFFSET = np.array([4096.0, -4096.0, 2048.0])
F32 = np.float32
# the seed and the iterations of the suite: two passes over the eight mesh kinds (the same for the CPU and the GPU half)
SUITE_SEED = 7
SUITE_ITERATIONS = {family: 16 for family in FAMILIES}


class Case:
    """one drawn case: the inputs, the knobs and `line`, the description that reproduces it"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return self.line


# ---- meshes -------------------------------------------------------------------------------------------------------------
def _unindexed(v, f):
    """every face with three vertices of its own: a vertex can be made hostile without touching the neighbours"""
    return np.ascontiguousarray(v[f].reshape(-1, 3), F32), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


def _base_mesh(rng, kind, cap):
    """(v, f, label) of mesh kind `kind` (an index into KINDS) with at most `cap` triangles, before scale and offset"""
    small = cap < MAX_TRIS
    if kind == 0:
        nt = int(rng.integers(1, 4))
        v, f = W.random_soup(nt, seed=int(rng.integers(1 << 30)), size=0.5)
        return v, f, f"few({nt})"
    if kind == 1:
        s = int(rng.integers(0, 3 if small else 4))
        return W.icosphere(s) + (f"icosphere({s})",)
    if kind == 2:
        nt, size = int(rng.integers(2, cap + 1)), float(rng.uniform(0.02, 0.6))
        return W.random_soup(nt, seed=int(rng.integers(1 << 30)), size=size) + (f"soup({nt}, size {size:.3f})",)
    if kind == 3:
        s = int(rng.integers(0, 2)) if small else int(rng.integers(1, 3))
        return W.nested_shells(s) + (f"shells({s})",)
    if kind == 4:
        s, amp, sd = int(rng.integers(1, 3 if small else 4)), float(rng.uniform(0.01, 0.3)), int(rng.integers(1000))
        v, f = W.icosphere(s)
        return W.displaced(v, seed=sd, amplitude=amp), f, f"displaced({s}, amplitude {amp:.3f})"
    if kind == 5:
        reps = int(rng.integers(100, min(800, cap - 64) + 1))      # (64 + reps triangles)
        return W.deep_tree_mesh(reps) + (f"deep({reps})",)
    if kind == 6:
        nt, size, axis = int(rng.integers(2, cap + 1)), float(rng.uniform(0.02, 0.6)), int(rng.integers(3))
        v, f = W.random_soup(nt, seed=int(rng.integers(1 << 30)), size=size)
        v[:, axis] = F32(rng.uniform(-1, 1))
        return v, f, f"flat({nt}, size {size:.3f}, axis {axis})"
    inner = int(rng.integers(1, 5))
    v, f, label = _base_mesh(rng, inner, cap)
    v, f = _unindexed(v, f)
    share = float(rng.uniform(0.05, 0.5))
    bad = np.flatnonzero(rng.random(len(f)) < share)
    if len(bad) == 0:
        bad = np.array([int(rng.integers(len(f)))])
    v = v.copy()
    v[f[bad, rng.integers(0, 3, len(bad))], rng.integers(0, 3, len(bad))] = np.nan
    return v, f, f"holed({label}, {len(bad)} of {len(f)} faces inactive)"


def _placed(rng, v, kind, iteration):
    """kinds (b) .. (h): a uniform scale in [0.1, 20] and an offset in [-3, 3]^3; in one iteration of four the scale is
    anisotropic, in another the offset puts the mesh on a coarse float grid"""
    if kind == 0:
        return v, ""
    scale, offset = np.full(3, rng.uniform(0.1, 20.0)), rng.uniform(-3, 3, 3)
    which = (iteration // len(KINDS) + iteration) % 4      # (not tied to the kind: each kind meets each of them in turn)
    note = f", scale {scale[0]:.3f}"
    if which == 1:
        scale, note = scale * ANISOTROPIC, note + " x (1, 1/64, 16)"
    if which == 3:
        offset, note = COARSE_OFFSET, note + ", offset (4096, -4096, 2048)"
    return (v.astype(np.float64) * scale + offset).astype(F32), note


def finite_box(v):
    v = np.asarray(v, np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    return v.min(0), v.max(0)


def draw_mesh(rng, kind, iteration, cap=MAX_TRIS, refit=False):
    """(v, f, v2 or None, label): v2 = the vertices moved by up to 0.2 of the extent each, the topology (and every NaN) kept"""
    v, f, label = _base_mesh(rng, kind, cap)
    v, note = _placed(rng, v, kind, iteration)
    assert 1 <= len(f) <= cap
    v2 = None
    if refit:
        lo, hi = finite_box(v)
        v2 = (v.astype(np.float64) + rng.uniform(-0.2, 0.2, v.shape) * (hi - lo)).astype(F32)
    return np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32), v2, label + note


def draw_batch(rng, family, seed, iteration):
    """half of the iterations an edge size, the others uniform in [1, 700]: by a schedule of the (seed, family) over 14
    iterations, so that a run of 14 meets every edge size once"""
    slot = np.random.default_rng((seed, FAMILIES.index(family))).permutation(2 * len(EDGE_BATCHES))[iteration % (2 * len(EDGE_BATCHES))]
    return int(EDGE_BATCHES[slot]) if slot < len(EDGE_BATCHES) else int(rng.integers(1, MAX_QUERIES + 1))


def refits(iteration):
    """every second iteration, and not the same kinds in every pass over them"""
    return (iteration // len(KINDS) + iteration) % 2 == 1


# ---- queries ------------------------------------------------------------------------------------------------------------
def _wide_box(lo, hi):
    ext = np.maximum(hi - lo, 1e-3 * max(float((hi - lo).max()), 1e-6))
    return lo - 0.3 * ext, hi + 0.3 * ext, ext


def _points(rng, lo, hi, n):
    wlo, whi, _ = _wide_box(lo, hi)
    return NC.hash_points(n, int(rng.integers(1 << 20)), wlo, whi)


def _rays(rng, lo, hi, n):
    """hash rays from the widened box, half of them aimed at the mesh, and per-ray bounds (one case in four: none)"""
    wlo, whi, ext = _wide_box(lo, hi)
    o, d = W.hash_rays(n, int(rng.integers(1 << 20)), wlo, whi)
    o, d = np.ascontiguousarray(o, F32), np.array(d, F32)
    aimed = rng.random(n) < 0.5
    d[aimed] = ((lo + hi) / 2 - o[aimed] + rng.normal(0, 0.05, (int(aimed.sum()), 3)) * ext).astype(F32)
    if rng.random() < 0.25:
        return o, np.ascontiguousarray(d), None, None
    tlo, thi = RC.hash_bounds(n, int(rng.integers(1 << 20)), 1.0)
    top = np.where(aimed, 2.0, 1.5 * float(ext.max())).astype(F32)      # (an aimed ray reaches the centre at t = 1)
    return o, np.ascontiguousarray(d), (tlo * top).astype(F32), (thi * top).astype(F32)


def _direction(rng):
    return SPC.DEFAULT.copy() if rng.random() < 0.5 else rng.uniform(-1, 1, 3).astype(F32)


def _query_triangles(rng, v, lo, hi, n):
    """faces of a second random mesh placed over the first, degenerate ones sprinkled in, filled up with hashed triangles"""
    v2, f2, _, label = draw_mesh(rng, int(rng.integers(1, 5)), 0, cap=MAX_QUERIES)
    lo2, hi2 = finite_box(v2)
    s = (hi - lo).max() / max((hi2 - lo2).max(), 1e-30) * rng.uniform(0.5, 1.2)
    own = TC.own_faces(((v2.astype(np.float64) - (lo2 + hi2) / 2) * s + (lo + hi) / 2).astype(F32), f2, limit=n)
    rest = TC.hashed_triangles(n - len(own), *_wide_box(lo, hi)[:2], TC.extent(v), seed=int(rng.integers(1 << 20)))
    tri = np.concatenate([own, rest])[rng.permutation(n)]
    tri[3::7, 2] = tri[3::7, 0]                                        # a doubled vertex
    tri[5::11, 1:] = tri[5::11, :1]                                    # a point
    return np.ascontiguousarray(tri, F32), label


def _capacity(family):
    import boxes_sim, cross_sim, nearest_sim, range_sim, scene_cross_sim, scene_nearest_sim, scene_points_sim, scene_tris_sim      # noqa: E401
    import tri_nearest_sim, tris_sim, within_sim      # noqa: E401
    sims = dict(nearest=nearest_sim, range=range_sim, within=within_sim, cross=cross_sim, boxes=boxes_sim, tris=tris_sim, scene=range_sim,
                scene_cross=scene_cross_sim, scene_points=scene_points_sim, scene_nearest=scene_nearest_sim, tri_nearest=tri_nearest_sim,
                scene_tris=scene_tris_sim)
    return sims[family].stack_capacity()


def _queries(rng, family, v, lo, hi, n):
    """(dict of query arrays, note) of a family on geometry whose finite box is (lo, hi); v: the vertices a generator reads"""
    q, note = {}, ""
    if family in ("points", "nearest", "within", "boxes", "scene_points", "scene_nearest"):
        q["p"] = _points(rng, lo, hi, n)
    if family in ("points", "scene_points"):
        q["d"] = _direction(rng)
        note = f", direction {q['d'].tolist()}"
    if family == "within":
        q["radius"] = WC.hashed_radii(n, WC.extent(v), seed=int(rng.integers(1 << 20)))
    if family == "scene_nearest":
        if rng.random() < 0.25:
            q["md"], note = None, ", unbounded"
        else:
            q["md"], note = WC.hashed_radii(n, float((hi - lo).max()), seed=int(rng.integers(1 << 20))), ", hashed max_distance"
    if family == "boxes":
        q["lo"], q["hi"] = BC.hashed_boxes(q["p"], BC.extent(v), seed=int(rng.integers(1 << 20)))
    if family == "tris":
        q["tri"], label = _query_triangles(rng, v, lo, hi, n)
        note = f", query faces of {label}"
    if family == "planes":
        q["o"], q["n"] = PC.hashed_planes(v, n, int(rng.integers(1 << 20)))
    if family in ("range", "cross", "scene", "scene_cross"):
        q["o"], q["d"], q["tmin"], q["tmax"] = _rays(rng, lo, hi, n)
        note = ", no bounds" if q["tmin"] is None else ", per-ray [tmin, tmax]"
    if family in ("tri_nearest", "scene_tris"):
        q["tri"], label = _query_triangles(rng, v, lo, hi, n)
        note = f", query faces of {label}"
        if family == "tri_nearest":
            if rng.random() < 0.25:
                q["md"], note = None, note + ", unbounded"
            else:
                q["md"], note = WC.hashed_radii(n, float((hi - lo).max()), seed=int(rng.integers(1 << 20))), note + ", hashed max_distance"
        # every thirteenth query is invalid (one NaN component, each of the nine in turn): inside live waves and instance loops
        rows = np.arange(9, n, 13)
        q["tri"].reshape(n, 9)[rows, rows % 9] = np.nan
    return q, note


def invalid_queries(case):
    """[n] bool: the query triangles of the two triangle families that hold a NaN"""
    return ~np.isfinite(case.q["tri"]).all(axis=(1, 2))


SCHEDULED_LIMITS = (0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, None)      # (None: the capacity)


def _knobs(rng, family, seed, iteration):
    if family == "points":
        return {}
    if family == "planes":
        return {"frontier_entries": int(rng.choice(PC.FRONTIERS))}
    if family in ("tri_nearest", "scene_tris"):
        # the nearest-face walk pushes a far child only where the bound so far does not cull it, and independent draws left
        # too few iterations at a limit a lane can overflow: the limits come by a schedule of the (seed, family) over 16
        # iterations, as the batch sizes do, so that every pass of 16 holds 14 at a limit of 1, 2 or 3
        slot = np.random.default_rng((seed, FAMILIES.index(family), 0, 0)).permutation(len(SCHEDULED_LIMITS))[iteration % len(SCHEDULED_LIMITS)]
        limit = SCHEDULED_LIMITS[slot]
        return {"stack_entries": _capacity(family) if limit is None else limit}
    # (1, 2 and 3 entries are the ones a lane can overflow: drawn more often than the two that cannot lose a push)
    return {"stack_entries": int(rng.choice([0, 1, 2, 3, _capacity(family)], p=[0.1, 0.3, 0.25, 0.25, 0.1]))}


# ---- draw ---------------------------------------------------------------------------------------------------------------
def draw(family, seed, iteration):
    rng = np.random.default_rng((seed, FAMILIES.index(family), iteration))
    kind = iteration % len(KINDS)
    n = draw_batch(rng, family, seed, iteration)
    head = f"{family} seed {seed} iteration {iteration}: kind ({'abcdefgh'[kind]}) "
    if family not in SCENES:
        v, f, v2, label = draw_mesh(rng, kind, iteration, refit=refits(iteration))
        lo, hi = finite_box(v)
        q, note = _queries(rng, family, v, lo, hi, n)
        knobs = _knobs(rng, family, seed, iteration)
        line = head + f"{label}, {len(f)} triangles, batch {n}{note}, {knobs}, refit {v2 is not None}"
        return Case(family=family, seed=seed, iteration=iteration, kind=kind, v=v, f=f, v2=v2, n=n, q=q, knobs=knobs, line=line)
    # a scene: 1 to 4 members (the first of this iteration's kind), 1 to 70 instances placed by general affine maps
    members, labels = [], []
    for m in range(int(rng.integers(1, 5))):
        # (the other members: any kind, half of the time a closed one, which has an inside)
        other = int(rng.choice(CLOSED_KINDS)) if rng.random() < 0.5 else int(rng.integers(len(KINDS)))
        v, f, _, label = draw_mesh(rng, kind if m == 0 else other, iteration + m, cap=MAX_MEMBER_TRIS)
        members.append((v, f)); labels.append(f"{label} [{len(f)}]")
    ninst = int(rng.choice(EDGE_INSTANCES)) if rng.random() < 0.5 else int(rng.integers(1, MAX_INSTANCES + 1))
    mesh_of = rng.integers(0, len(members), ninst).astype(np.int32)
    mesh_of[int(rng.integers(ninst))] = 0                              # (this iteration's kind is placed at least once)
    spread = 0.4 + 0.5 * ninst ** (1 / 3)                              # (copies about one unit across: neighbours overlap)
    Ms = []
    for k in range(ninst):
        lo, hi = finite_box(members[mesh_of[k]][0])
        size = max(float((hi - lo).max()), 1e-6)
        lin = SC.general(rng, scale=1.0 / size)                        # every placed copy about one unit across, whatever its member's scale
        if rng.random() < 0.3:
            lin = lin @ np.diag([-1.0, 1.0, 1.0])                      # a mirror
        t = rng.uniform(-spread, spread, 3) - lin @ ((lo + hi) / 2)
        Ms.append(SC.placement(lin, t))
    Ms = np.asarray(Ms, F32).reshape(-1, 3, 4)
    if ninst >= 2:                                                     # two equal placements of one member
        a, b = rng.choice(ninst, 2, replace=False)
        Ms[b], mesh_of[b] = Ms[a], mesh_of[a]
    order = rng.permutation(ninst).astype(np.int32)
    mesh_of, Ms = np.ascontiguousarray(mesh_of[order]), np.ascontiguousarray(Ms[order])      # (a random instance order)
    boxes = [SC.world_box(members[m][0], M) for m, M in zip(mesh_of, Ms)]
    lo, hi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
    world = np.concatenate([np.stack(b) for b in boxes]).astype(F32)
    q, note = _queries(rng, family, world, lo, hi, n)
    knobs = _knobs(rng, family, seed, iteration)
    knobs["order"] = rng.permutation(ninst).astype(np.int32)           # the order the host walk visits the instances in
    refit_member, v2 = None, None
    if refits(iteration):
        refit_member = int(rng.integers(len(members)))
        v = members[refit_member][0]
        mlo, mhi = finite_box(v)
        v2 = (v.astype(np.float64) + rng.uniform(-0.2, 0.2, v.shape) * (mhi - mlo)).astype(F32)
    line = head + f"members {labels}, {ninst} instances, batch {n}{note}, stack_entries {knobs['stack_entries']}, refit of member {refit_member}"
    return Case(family=family, seed=seed, iteration=iteration, kind=kind, members=members, mesh_of=mesh_of, M=Ms, v2=v2, refit_member=refit_member,
                n=n, q=q, knobs=knobs, line=line)


def geometry(case, refitted=False):
    """what the brute force reads: (v, f) of a mesh family, the list of members of a scene family; after the refit: with v2"""
    if case.family not in SCENES:
        return case.v2 if refitted else case.v, case.f
    mem = list(case.members)
    if refitted:
        mem[case.refit_member] = (case.v2, mem[case.refit_member][1])
    return mem


# ---- the host tree and its refit ----------------------------------------------------------------------------------------
def _tri_boxes(a, b, c):
    """tr_tri_box (csrc/tr_math.h) in numpy float32: fminf / fmaxf skip a NaN, each bound padded outward"""
    with np.errstate(invalid="ignore", over="ignore"):
        l, h = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
        pad = lambda x: np.abs(x) * F32(2.0 ** -21) + F32(2.0 ** -100)      # noqa: E731
        return (l - pad(l)).astype(F32), (h + pad(h)).astype(F32)


def _frame(mn, mx):
    """tr_qframe_make (csrc/tr_bvh.h) in numpy: base = the bounds' minimum, scale = a power of two whose plane 65535 reaches
    the maximum"""
    frame = np.zeros(6, F32)
    for k in range(3):
        with np.errstate(invalid="ignore", over="ignore"):
            ext = F32(mx[k]) - F32(mn[k])
        s = F32(1.0)
        if ext > 0 and ext <= F32(3.0e38):
            s = F32(np.ldexp(1.0, max(int(np.frexp(F32(ext / F32(65535.0)))[1]), -126)))
        for _ in range(300):
            if F32(np.float64(65535.0) * np.float64(s) + np.float64(mn[k])) >= mx[k]:
                break
            s = F32(s * F32(2.0))
        frame[k], frame[3 + k] = mn[k], s
    return frame


def _grid(x, frame, axis, upper):
    """tr_qfloor / tr_qceil: the largest grid plane <= x / the smallest >= x, through the traversal's own decode"""
    planes = (np.arange(65536, dtype=np.float64) * np.float64(frame[3 + axis]) + np.float64(frame[axis])).astype(F32)
    if upper:
        q = np.minimum(np.searchsorted(planes, x, "left"), 65535)
        return np.where(np.isnan(x), 65535, q).astype(np.uint32)
    q = np.maximum(np.searchsorted(planes, x, "right") - 1, 0)
    return np.where(np.isnan(x), 0, q).astype(np.uint32)


def refit_host(B, v2, f):
    """a sim.SimBVH of the same topology on the moved vertices: the triangle records rewritten in place (vertices and
    tr_tri_scale), every child box the union of what lies below it, bottom up, the grid nodes on the frame of the new bounds
    -- what a refit of the library leaves"""
    from sim import SimBVH
    v2, f = np.ascontiguousarray(v2, F32), np.asarray(f)
    tris = np.array(B.tris, np.uint32)
    face = tris[:, 9].view(np.int32)
    abc = v2[f[face]]                                                 # [nf, 3, 3] in slot order
    tris[:, :9] = abc.reshape(-1, 9).view(np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = np.abs(abc[:, 1] - abc[:, 0]), np.abs(abc[:, 2] - abc[:, 0])
        esum = ((e1[:, 0] + e1[:, 1]) + e1[:, 2]) + ((e2[:, 0] + e2[:, 1]) + e2[:, 2])
    tris[:, 10] = esum.astype(F32).view(np.uint32)
    nodes = np.array(B.nodes, np.uint32)
    qnodes, frame = np.array(B.qnodes, np.uint32), np.array(B.frame, F32)
    if len(nodes):
        llo, lhi = _tri_boxes(abc[:, 0], abc[:, 1], abc[:, 2])
        child = nodes[:, 12:14].view(np.int32)
        order, todo = [], [0]
        while todo:                                                   # parents before children; unions in reverse
            i = todo.pop()
            order.append(i)
            todo.extend(int(c) for c in child[i] if c >= 0)
        assert len(order) == len(nodes)
        nlo, nhi = np.zeros((len(nodes), 3), F32), np.zeros((len(nodes), 3), F32)
        clo, chi = np.zeros((len(nodes), 2, 3), F32), np.zeros((len(nodes), 2, 3), F32)
        for i in reversed(order):
            for k in (0, 1):
                c = int(child[i, k])
                clo[i, k], chi[i, k] = (llo[~c], lhi[~c]) if c < 0 else (nlo[c], nhi[c])
            nlo[i], nhi[i] = np.fmin(clo[i, 0], clo[i, 1]), np.fmax(chi[i, 0], chi[i, 1])
        boxes = np.stack([clo[..., 0], clo[..., 1], clo[..., 2], chi[..., 2], chi[..., 0], chi[..., 1]], -1)      # tr_node_set_box
        nodes[:, :12] = np.ascontiguousarray(boxes, F32).reshape(-1, 12).view(np.uint32)
        with np.errstate(invalid="ignore"):
            frame = _frame(np.fmin.reduce(llo, 0), np.fmax.reduce(lhi, 0))
        ql = [_grid(clo[..., a], frame, a, False) for a in range(3)]
        qh = [_grid(chi[..., a], frame, a, True) for a in range(3)]
        for k in (0, 1):                                              # tr_qnode_set_box
            qnodes[:, 3 * k] = ql[0][:, k] | (ql[1][:, k] << 16)
            qnodes[:, 3 * k + 1] = ql[2][:, k] | (qh[2][:, k] << 16)
            qnodes[:, 3 * k + 2] = qh[0][:, k] | (qh[1][:, k] << 16)
    return SimBVH(arrays=(nodes, np.array(B.links), tris), qarrays=(qnodes, frame))


def host_trees(case):
    from sim import SimBVH
    if case.family not in SCENES:
        return SimBVH(case.v, case.f)
    return [SimBVH(v, f) for v, f in case.members]


def host_trees_refitted(case, trees):
    if case.family not in SCENES:
        return refit_host(trees, case.v2, case.f)
    out = list(trees)
    out[case.refit_member] = refit_host(trees[case.refit_member], case.v2, case.members[case.refit_member][1])
    return out


# ---- the family table ---------------------------------------------------------------------------------------------------
# brute(case, geometry) -> want;  walk(case, trees, geometry) -> (got, lost [n] bool or None: the walk does not report it);
# native(case, handle, device, want) -> got (every native entry of the family once; points: compares inside check_all);
# same(got, want, what): the family's comparator;  hits(want) -> [n] bool or count per query: what the lists or masks hold;
# no_result(case, got, what), the two triangle families: the queries made invalid by a NaN came back as "no result"
def _oracle(geom):
    from oracle.oracle import OracleIntersector
    return OracleIntersector(geom[0], geom[1], 1)


def _points_box(geom):
    lo, hi = finite_box(geom[0])
    return lo.astype(F32), hi.astype(F32)


def _points_brute(c, geom):
    import test_gpu_contains as G
    R = _oracle(geom)
    dirs = np.tile(c.q["d"], (c.n, 1)).astype(F32)
    cp, cm = R.intersects_count(c.q["p"], dirs), R.intersects_count(c.q["p"], -dirs)
    in_box, inside, broken = G.decision(c.q["p"], _points_box(geom), cp, cm)
    return dict(inside=inside, broken=broken, counts=np.stack([cp, cm]), summary=np.array([in_box.sum(), broken.sum()], np.int64))


def _points_walk(c, B, geom):
    import points_sim
    return points_sim.contains(B, c.q["p"], c.q["d"], _points_box(geom)), None


def _points_same(got, want, what):
    for k in ("counts", "inside", "broken", "summary"):
        assert np.array_equal(np.asarray(got[k]), want[k]), f"{what}: {k} differs at {np.flatnonzero((np.asarray(got[k]) != want[k]).reshape(-1))[:8]}"


def _points_native(c, r, device, geom):
    import test_gpu_contains as G
    import triro.backend.ops as hops
    inside, broken, counts, summary = G.check_all(r, _oracle(geom), c.q["p"], c.q["d"], device, c.line, addressing=hops.contains_addressing(r.as_wrapper),
                                                  box=_points_box(geom), retry=False)
    return dict(inside=inside, broken=broken, counts=counts, summary=summary)


def _nearest_walk(c, B, geom=None):
    import nearest_sim
    got = nearest_sim.walk(B, c.q["p"], c.knobs["stack_entries"], want_lost=True)
    return got[:3], got[3]


def _range_walk(c, B, geom=None):
    import range_sim
    out = range_sim.walk(B, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], c.knobs["stack_entries"])
    return out, out["lost"] | out["lost_any"]


def _planes_both(run):
    return tuple(run(cut) for cut in (False, True))


def _planes_walk(c, B, geom=None):
    import planes_sim
    got = _planes_both(lambda cut: planes_sim.walk(B, c.q["o"], c.q["n"], cut=cut, frontier_entries=c.knobs["frontier_entries"], want_stats=True))
    return tuple(g[0] for g in got), got[0][1].overflows > 0


def _planes_same(got, want, what):
    for cut, g, w in zip((False, True), got, want):
        PC.assert_same(g, w, f"{what}, cut={cut}")


def _scene_walk(c, trees, geom=None):
    import scene_sim
    out = scene_sim.walk(trees, c.mesh_of, c.M, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], c.knobs["stack_entries"], order=c.knobs["order"])
    return out, out["lost"] | out["lost_any"]


def _scene_points_walk(c, trees, geom=None):
    import scene_points_sim
    got, lost = scene_points_sim.walk(trees, c.mesh_of, c.M, c.q["p"], c.q["d"], c.knobs["stack_entries"], order=c.knobs["order"], want_lost=True)
    return got, lost >= 0


def _split(got, k):
    """a walk's (k results..., lost) -> ((k results), lost)"""
    return got[:k], got[k]


def _scene_tris_no_result(c, got, what):
    bad = invalid_queries(c)
    assert not np.asarray(got.any)[bad].any() and not np.asarray(got.count)[bad].any(), f"{what}: an invalid query has rows"


def _sim(name):
    import importlib
    return importlib.import_module(name + "_sim")


def _gpu(name):
    import importlib
    return importlib.import_module("test_gpu_" + name)


TABLE = {
    "points": dict(
        brute=_points_brute, walk=_points_walk, same=_points_same, native=_points_native,
        hits=lambda w: w["inside"]),
    "nearest": dict(
        brute=lambda c, g: _sim("nearest").brute(g[0], g[1], c.q["p"]), walk=_nearest_walk, same=NC.assert_same_bits,
        native=lambda c, r, dev, geom: _gpu("nearest").native(r, c.q["p"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w[2] >= 0),
    "range": dict(
        brute=lambda c, g: _sim("range").brute(g[0], g[1], c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"]), walk=_range_walk, same=RC.assert_same_bits,
        native=lambda c, r, dev, geom: _gpu("range").native(r, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w["hit"]),
    "within": dict(
        brute=lambda c, g: _sim("within").brute(g[0], g[1], c.q["p"], c.q["radius"]),
        walk=lambda c, B, geom=None: _sim("within").walk(B, c.q["p"], c.q["radius"], c.knobs["stack_entries"], want_lost=True), same=WC.assert_same,
        native=lambda c, r, dev, geom: _gpu("within").native(r, c.q["p"], c.q["radius"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.count),
    "cross": dict(
        brute=lambda c, g: _sim("cross").brute(g[0], g[1], c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"]),
        walk=lambda c, B, geom=None: _sim("cross").walk(B, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], c.knobs["stack_entries"], want_lost=True),
        same=CC.assert_same,
        native=lambda c, r, dev, geom: _gpu("cross").native(r, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.count),
    "boxes": dict(
        brute=lambda c, g: _sim("boxes").brute(g[0], g[1], c.q["lo"], c.q["hi"]),
        walk=lambda c, B, geom=None: _sim("boxes").walk(B, c.q["lo"], c.q["hi"], c.knobs["stack_entries"], want_lost=True), same=BC.assert_same,
        native=lambda c, r, dev, geom: _gpu("boxes").native(r, c.q["lo"], c.q["hi"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.count),
    "tris": dict(
        brute=lambda c, g: _sim("tris").brute(g[0], g[1], c.q["tri"]),
        walk=lambda c, B, geom=None: _sim("tris").walk(B, c.q["tri"], c.knobs["stack_entries"], want_lost=True), same=TC.assert_same,
        native=lambda c, r, dev, geom: _gpu("tris").native(r, c.q["tri"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.count),
    "planes": dict(
        brute=lambda c, g: _planes_both(lambda cut: _sim("planes").brute(g[0], g[1], c.q["o"], c.q["n"], cut=cut)), walk=_planes_walk,
        same=_planes_same,
        native=lambda c, r, dev, geom: _planes_both(
            lambda cut: _gpu("planes").native(r, c.q["o"], c.q["n"], dev, cut=cut, frontier_entries=c.knobs["frontier_entries"])),
        hits=lambda w: w[0].count),
    "scene": dict(
        brute=lambda c, mem: _sim("scene").brute(mem, c.mesh_of, c.M, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"]), walk=_scene_walk,
        same=lambda got, want, what: RC.assert_same_bits(got, want, what, keys=SC.KEYS),
        native=lambda c, s, dev, geom: _gpu("scene").native(s, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w["hit"]),
    "scene_cross": dict(
        brute=lambda c, mem: _sim("scene_cross").brute(mem, c.mesh_of, c.M, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"]),
        walk=lambda c, trees, geom=None: _sim("scene_cross").walk(trees, c.mesh_of, c.M, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], c.knobs["stack_entries"],
                                                       order=c.knobs["order"], want_lost=True),
        same=XC.assert_same,
        native=lambda c, s, dev, geom: _gpu("scene_cross").native(s, c.q["o"], c.q["d"], c.q["tmin"], c.q["tmax"], dev,
                                                                  stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.count),
    "scene_points": dict(
        brute=lambda c, mem: _sim("scene_points").brute(mem, c.mesh_of, c.M, c.q["p"], c.q["d"]), walk=_scene_points_walk, same=SPC.assert_same,
        native=lambda c, s, dev, geom: _gpu("scene_points").native(s, c.q["p"], c.q["d"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.count),
    "scene_nearest": dict(
        brute=lambda c, mem: _sim("scene_nearest").brute(mem, c.mesh_of, c.M, c.q["p"], c.q["md"]),
        walk=lambda c, trees, geom=None: _sim("scene_nearest").walk(trees, c.mesh_of, c.M, c.q["p"], c.q["md"], c.knobs["stack_entries"], order=c.knobs["order"],
                                                         want_lost=True),
        same=NN.assert_same,
        native=lambda c, s, dev, geom: _gpu("scene_nearest").native(s, c.q["p"], c.q["md"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.tri >= 0),
    "tri_nearest": dict(
        brute=lambda c, g: _sim("tri_nearest").brute(g[0], g[1], c.q["tri"], c.q["md"]),
        walk=lambda c, B, geom=None: _split(_sim("tri_nearest").walk(B, c.q["tri"], c.q["md"], c.knobs["stack_entries"], want_lost=True), 4),
        same=TN.assert_same,
        native=lambda c, r, dev, geom: _gpu("tri_nearest").native(r, c.q["tri"], dev, c.q["md"], stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w[0] >= 0,
        no_result=lambda c, got, what: TN.check_no_result(got, invalid_queries(c), what + ": an invalid query has a result")),
    "scene_tris": dict(
        brute=lambda c, mem: _sim("scene_tris").brute(mem, c.mesh_of, c.M, c.q["tri"]),
        walk=lambda c, trees, geom=None: _sim("scene_tris").walk(trees, c.mesh_of, c.M, c.q["tri"], c.knobs["stack_entries"], order=c.knobs["order"],
                                                                 want_lost=True),
        same=ST.assert_same,
        # (the three C entries themselves, between poisoned guard rows, every row inside checked: no binding to wrap)
        native=lambda c, s, dev, geom: _gpu("scene_tris").native(s, c.q["tri"], dev, stack_entries=c.knobs["stack_entries"]),
        hits=lambda w: w.count,
        no_result=_scene_tris_no_result),
}
assert tuple(TABLE) == FAMILIES


def natives():
    """the union of the native entry points the families' GPU modules wrap: every call of one is followed by assert_written"""
    names = ["contains_points_native", "closest_point_native", "range_any_native", "range_closest_native", "scene_any_native",
             "scene_closest_native", "scene_closest_point_native", "triangles_nearest_native"]
    for name in ("within", "cross", "boxes", "tris", "planes", "scene_cross", "scene_points"):
        names += [x for x in _gpu(name).NATIVES if x not in names]
    return tuple(names)


# ---- one case on the host and on the device -----------------------------------------------------------------------------
def run_host(case, walk=None):
    """the host walk against the brute force, after the build and after the refit -> [(want, lost or None)] per state.  walk:
    another walk of the family's signature (a mutant's)"""
    row = TABLE[case.family]
    walk = walk or row["walk"]
    trees = host_trees(case)
    out = []
    for refitted in ((False, True) if case.v2 is not None else (False,)):
        if refitted:
            trees = host_trees_refitted(case, trees)
        geom = geometry(case, refitted)
        want = row["brute"](case, geom)
        got, lost = walk(case, trees, geom)
        what = f"{case.line} [host walk{', after the refit' if refitted else ''}]"
        row["same"](got, want, what)
        if "no_result" in row:
            row["no_result"](case, got, what)
        out.append((want, lost))
    return out


def run_device(case, device):
    """a fresh handle, every native entry of the family at the drawn knobs against the brute force, bit for bit; with v2 the
    refit and the same again.  Nothing is caught: an error of a native call ends the run"""
    import torch
    row = TABLE[case.family]

    def T(x):
        return torch.from_numpy(np.array(x, order="C")).to(device)
    from triro.ray.ray_optix import RayMeshIntersector
    if case.family in SCENES:
        from triro.ray import RaySceneIntersector
        handles = [RayMeshIntersector(vertices=T(v), faces=T(f)) for v, f in case.members]
        handle = RaySceneIntersector(handles, case.mesh_of, case.M)
    else:
        handles = None
        handle = RayMeshIntersector(vertices=T(case.v), faces=T(case.f))
    for refitted in ((False, True) if case.v2 is not None else (False,)):
        if refitted:
            (handles[case.refit_member] if handles else handle).refit(T(case.v2))      # (a scene: of one member, no commit)
        geom = geometry(case, refitted)
        want = row["brute"](case, geom)
        got = row["native"](case, handle, device, geom)
        what = f"{case.line} [native{', after the refit' if refitted else ''}]"
        row["same"](got, want, what)
        if "no_result" in row:
            row["no_result"](case, got, what)
