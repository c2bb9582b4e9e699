"""The randomised parity sweep of the fourteen satellite query libraries, on the host (tests/satellite_sweep.py: the generator
and the family table; tests/test_gpu_satellite_sweep.py: the same cases on the GPU).

1. every family, the suite's seed and iterations: the host walk on SimBVH(v, f) -- and after the refit on the refitted host tree
   -- equals the brute force with the family's comparator, bit for bit; over the run the inputs meet the conditions that keep
   the sweep from being vacuous (every mesh kind, a batch below 64, a batch that is no multiple of 64, lanes that lose a push in
   a third of the iterations, lists or masks that are neither empty nor all-true in half of them); nearest and within also pass
   nearest_cases.check_against_numpy, the independent float64 evaluation, on every iteration but the deep and the holed kinds,
   and tri_nearest its own (tri_nearest_cases.check_against_numpy) on up to 64 queries with area per state; tri_nearest has
   distances of exactly 0 next to positive ones in a third of the iterations, scene_tris queries with rows in two or more
   instances in a quarter; in both, the queries made invalid by a NaN come back as "no result" (satellite_sweep.run_host).
2. planted faults: mutant host simulations built in tmp_path (a copy of the simulation's source and of csrc/*.h with ONE
   textual substitution, compiled by the simulation's own lib()) must disagree with the unmutated brute force within the run."""
import contextlib
import glob
import io
import os
import re
import shutil

import numpy as np
import pytest

import nearest_cases as NC
import satellite_sweep as S
import tri_nearest_cases as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc")
NO_TOLERANCE_KINDS = (5, 7)          # deep (coincident triangles in bulk) and holed (inactive faces): as the fixed tolerance cases


def _numpy_check(case, states):
    """NC.check_against_numpy on the brute force of every state -> the largest excess over a bound (<= 0 passes)"""
    worst = -np.inf
    for k, (want, _) in enumerate(states):
        v, f = S.geometry(case, refitted=k == 1)
        closest, distance, tri = want if case.family == "nearest" else want.nearest[:3]
        found = tri >= 0                                  # (within: the bounded nearest of a point with no face in its radius is none)
        if not found.any():
            continue
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            NC.check_against_numpy(v, f, case.q["p"][found], closest[found], distance[found], tri[found], what=case.line)
        figures = re.search(r"distance (\S+), closest (\S+), consistency (\S+), winner (\S+);", out.getvalue())
        worst = max(worst, *(float(x) for x in figures.groups()))
    return worst


NUMPY_QUERIES = 64                   # of tri_nearest per state: the numpy pass is [queries, faces, 27 + 3 points]


def _has_area(t):
    """[n] bool: the finite triangles [n, 3, 3] whose cross product is not zero in float64 (a NaN compares false)"""
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1) > 0


def _tri_numpy_check(case, states):
    """TN.check_against_numpy on the brute force of every state, on at most NUMPY_QUERIES of the queries that are finite, found
    and have area -> the largest excess over a bound (<= 0 passes).  A query without area that pierces a face is not at
    distance 0 (the documented caveat of the contract: test_the_degenerate_caveat_a_piercing_segment_is_not_at_zero), which
    numpy's upper bound does not know; active mesh faces without area are left out for the same reason, and with them the
    queries they win"""
    worst = -np.inf
    tri = case.q["tri"]
    for k, (want, _) in enumerate(states):
        v, f = S.geometry(case, refitted=k == 1)
        keep = ~(NC.active(v, f) & ~_has_area(np.asarray(v, np.float32)[f]))
        face = want[0]
        rows = np.flatnonzero(np.isfinite(tri).all(axis=(1, 2)) & (face >= 0) & _has_area(tri) & keep[np.maximum(face, 0)])
        rows = rows[:: max(1, -(-len(rows) // NUMPY_QUERIES))][:NUMPY_QUERIES]
        if len(rows) == 0:
            continue
        renumber = np.cumsum(keep) - 1
        got = (renumber[face[rows]].astype(np.int32), want[1][rows], want[2][rows], want[3][rows])
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            TN.check_against_numpy(v, f[keep], tri[rows], got, what=case.line)
        figures = re.search(r"witness on the face (\S+), on the query (\S+), consistency (\S+), above numpy's upper bound (\S+);", out.getvalue())
        worst = max(worst, *(float(x) for x in figures.groups()))
    return worst


def _identical(a, b):
    """two query arrays (or None twice) of one shape, type and bytes: a NaN equals itself"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _several_instances(want):
    """a query of a scene_tris_sim.Result has rows in two or more instances"""
    return any(len(np.unique(want.instance[want.offsets[i]:want.offsets[i + 1]])) >= 2 for i in np.flatnonzero(want.count > 1))


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
def test_host_walks_match_the_brute_force_and_the_inputs_reach_the_edges(family):
    n_it = S.SUITE_ITERATIONS[family]
    hits = S.TABLE[family]["hits"]
    kinds, batches, lost, nonempty, not_all, reports_lost, worst = set(), [], 0, 0, 0, False, -np.inf
    zero_and_positive = several = 0
    for iteration in range(n_it):
        case = S.draw(family, S.SUITE_SEED, iteration)
        again = S.draw(family, S.SUITE_SEED, iteration)
        assert case.line == again.line and all(_identical(a, b) for a, b in zip(case.q.values(), again.q.values())), "draw is not deterministic"
        states = S.run_host(case)                         # raises on the first mismatch, with the line that reproduces the case
        kinds.add(case.kind)
        batches.append(case.n)
        reports_lost |= states[0][1] is not None
        lost += any(l is not None and l.any() for _, l in states)
        found = [np.asarray(hits(want)) > 0 for want, _ in states]
        nonempty += any(x.any() for x in found)
        not_all += any(not x.all() for x in found)
        if family in ("nearest", "within") and case.kind not in NO_TOLERANCE_KINDS:
            worst = max(worst, _numpy_check(case, states))
        if family in ("tri_nearest", "scene_tris"):       # (the invalid queries run_host holds to "no result" are there)
            assert np.array_equal(np.flatnonzero(S.invalid_queries(case)), np.arange(9, case.n, 13)), case.line
        if family == "tri_nearest":
            # (an exact 0 next to a positive distance: ties between meeting faces, the (d2, face) order and the non-strict cull)
            zero_and_positive += any(((w[0] >= 0) & (w[1] == 0)).any() and ((w[0] >= 0) & (w[1] > 0)).any() for w, _ in states)
            if case.kind not in NO_TOLERANCE_KINDS:
                worst = max(worst, _tri_numpy_check(case, states))
        if family == "scene_tris":
            several += any(_several_instances(w) for w, _ in states)
    print(f"{family}: {n_it} iterations, kinds {sorted(kinds)}, batches {sorted(batches)}, a lane lost a push in {lost}, "
          f"non-empty in {nonempty}, not all-true in {not_all}" + (f", largest excess of check_against_numpy {worst:.3g}" if worst > -np.inf else "")
          + (f", a distance of 0 next to a positive one in {zero_and_positive}" if family == "tri_nearest" else "")
          + (f", a query with rows in two or more instances in {several}" if family == "scene_tris" else ""))
    assert kinds == set(range(len(S.KINDS))), "a mesh kind does not occur"
    assert min(batches) < 64, "no batch below 64"
    assert any(n % 64 for n in batches), "every batch is a multiple of 64"
    if reports_lost:                                      # (the per-point routine of `points` has no stack to overflow)
        assert 3 * lost >= n_it, f"a lane loses a push in {lost} of {n_it} iterations only"
    assert 2 * nonempty >= n_it, f"lists / masks are non-empty in {nonempty} of {n_it} iterations only"
    if family != "nearest":                               # (the unbounded nearest of a mesh with an active face always exists: it has no mask)
        assert 2 * not_all >= n_it, f"lists / masks are not all-true in {not_all} of {n_it} iterations only"
    if family in ("nearest", "within", "tri_nearest"):
        assert worst <= 0
    if family == "tri_nearest":
        assert 3 * zero_and_positive >= n_it, f"a distance of 0 next to a positive one in {zero_and_positive} of {n_it} iterations only"
    if family == "scene_tris":       # (otherwise the overflow rule's c0 and the (instance, face) row order are never exercised)
        assert 4 * several >= n_it, f"a query has rows in two or more instances in {several} of {n_it} iterations only"


def test_the_refitted_host_tree_is_the_tree_of_a_build_when_nothing_moved():
    """refit_host on the vertices the tree was built from reproduces its arrays bit for bit: boxes, triangle records, grid nodes"""
    from sim import SimBVH
    for iteration in (1, 2, 5, 6, 7):
        case = S.draw("nearest", S.SUITE_SEED, iteration)
        B = SimBVH(case.v, case.f)
        R = S.refit_host(B, case.v, case.f)
        for name in ("nodes", "links", "tris", "qnodes", "frame"):
            a, b = np.ascontiguousarray(getattr(B, name)), np.ascontiguousarray(getattr(R, name))
            assert a.tobytes() == b.tobytes(), f"{case.line}: {name} differs after a refit that moved nothing"


# ---- 2. planted faults ----------------------------------------------------------------------------------------------------
# (name, family whose sweep runs, header, the text replaced, its replacement): one per shared mechanism of tr_walk.h, one
# culling mutant per query header.  Every one gives wrong answers and stays memory-safe: none writes or pushes past a bound.
#
# A comparison that only changes between strict and non-strict differs from the original on an exact tie alone.  The bounds
# the walks cull by are computed against PADDED boxes (tr_tri_box), so such a tie needs inputs on a coarse float grid: the
# sweep has them (the offset (4096, -4096, 2048)) and kills that form in tr_nearest.h and tr_tris.h; in tr_planes.h the tie is a
# plane through a vertex (every seventh of planes_cases.hashed_planes), in the acceptance of a face.  In tr_within.h, tr_boxes.h,
# tr_range.h and tr_cross.h no drawn case holds such a tie (`!(lf > R2)` -> `!(lf >= R2)`, `hix < q.lox` -> `hix <= q.lox`,
# `!(tf < cut)` -> `!(tf <= cut)` and `tt >= lo` -> `tt > lo` all survive: DESIGN.md), so the planted culling fault there is a
# comparison against the wrong bound, which culls too eagerly.
#
# tr_tri_nearest.h culls by a margin-free box-against-box lower bound of a COMPUTED float64 distance: the strict form of its cull
# (tn_cull) is killed by exact ties at distance 0 between several meeting faces, which need no grid; tn_rewalk_bound swaps the
# two children's bounds in the stackless re-walk, which only a lane that lost a push reaches; tn_leaf_tie turns the (d2, face)
# order round.  tr_scene_tris.h: scene_tris_overflow drops the whole query's pairs, not the overflowing instance's, and
# scene_tris_cull tests the placed box against the wrong plane.  Removing the NaN guard of tr_scene_tris_apart (`proven`)
# SURVIVES the sweep: the holed kind makes one coordinate of a vertex NaN, which fminf / fmaxf skip, so every node box stays
# finite and no placed box has a NaN corner; that mutant stays with test_a_box_with_a_nan_corner_never_culls
# (tests/test_scene_tris_cpu.py).
_SET_VISIT = ("leaf(~c, acc);\n    }\n    if (tr_set_full<MODE>(acc)) { st.node = -1; return; }\n"
              "    const bool go0 = n.c0 >= 0 && !n.apart0, go1 = n.c1 >= 0 && !n.apart1")
_PLANE_MEETS = " + (s1 > 0.0) + (s2 > 0.0), neg = (s0 < 0.0) + (s1 < 0.0) + (s2 < 0.0);\n    return !(pos == 3"
MUTANTS = (
    # tr_walk.h: the re-walk climbs past child 1 when it comes back from child 0
    ("rewalk_climb", "within", "tr_walk.h", "b.nodes[parent].c0 == node ? 1 : 2", "b.nodes[parent].c0 == node ? 2 : 2"),
    # tr_walk.h: tr_rows_limit gives a query with one row none
    ("rows_limit", "within", "tr_walk.h", "if (count <= 0 || off < 0 || off >= total) return 0;", "if (count <= 1 || off < 0 || off >= total) return 0;"),
    # tr_walk.h: the sift of tr_rows_sort compares the wrong way round (a permutation still, in another order)
    ("rows_sort", "within", "tr_walk.h", "if (!rows.before(root, child)) break;", "if (!rows.before(child, root)) break;"),
    # the set walk (tr_set_visit, the visit of tr_set_probe): child 1 is dropped when child 0 is a leaf
    ("set_walk_second_child", "tris", "tr_boxes.h", _SET_VISIT + ";", _SET_VISIT + " && n.c0 >= 0;"),
    # one culling (or acceptance) mutant per query header
    ("nearest_cull", "nearest", "tr_nearest.h", "go_f = cf >= 0 && !(lf > best.d2);", "go_f = cf >= 0 && !(lf >= best.d2);"),
    ("within_cull", "within", "tr_within.h", "go_f = cf >= 0 && !(lf > R2);", "go_f = cf >= 0 && !(lf > 0.5 * R2);"),
    ("boxes_cull", "boxes", "tr_boxes.h", "return hix < q.lox ||", "return hix < q.hix ||"),
    ("tris_cull", "tris", "tr_tris.h", "czf) < qb.loz ||", "czf) <= qb.loz ||"),
    ("planes_meets", "planes", "tr_planes.h", "const int pos = (s0 > 0.0)" + _PLANE_MEETS, "const int pos = (s0 >= 0.0)" + _PLANE_MEETS),
    ("range_cull", "range", "tr_range.h", "return tr_slab_hit(tn, tf, lim) && !(tf < cut);", "return tr_slab_hit(tn, tf, lim) && !(tn < cut);"),
    ("cross_cull", "cross", "tr_cross.h", "go_f = cf >= 0 && tr_range_box(tnf, tff, lim, cut);", "go_f = cf >= 0 && tr_range_box(tnf, tnf, lim, cut);"),
    ("tn_cull", "tri_nearest", "tr_tri_nearest.h", "go_f = cf >= 0 && !(lf > best.d2);", "go_f = cf >= 0 && !(lf >= best.d2);"),
    ("tn_rewalk_bound", "tri_nearest", "tr_tri_nearest.h", "return !((phase ? n.lb1 : n.lb0) > best.d2);", "return !((phase ? n.lb0 : n.lb1) > best.d2);"),
    ("tn_leaf_tie", "tri_nearest", "tr_tri_nearest.h", "(lb == best.d2 && t.face > best.face)", "(lb == best.d2 && t.face < best.face)"),
    ("scene_tris_overflow", "scene_tris", "tr_scene_tris.h", "probe.acc.count = c0;", "probe.acc.count = 0;"),
    ("scene_tris_cull", "scene_tris", "tr_scene_tris.h", "tr_box_apart(qb, LO[0], LO[1], LO[2], HI[0], HI[1], HI[2]);",
     "tr_box_apart(qb, LO[0], LO[1], LO[2], HI[0], HI[1], HI[1]);"),
)


@contextlib.contextmanager
def mutant_library(tmp_path, family, header, old, new):
    """a build of the family's host simulation with `old` -> `new` in the copy of `header` -> its bound ctypes library"""
    import importlib
    sim = importlib.import_module(f"{family}_sim")
    here = tmp_path / "tests" / "host_sim"
    csrc = tmp_path / "trimesh-ray-optix_amd" / "csrc"
    os.makedirs(here); os.makedirs(csrc)
    shutil.copy(os.path.join(ROOT, "tests", "host_sim", f"{family}_sim.cpp"), here)
    for h in glob.glob(os.path.join(CSRC, "*.h")):
        shutil.copy(h, csrc)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    text = open(csrc / header).read()
    assert text.count(old) == 1, f"{header}: the text to replace occurs {text.count(old)} times"
    with open(csrc / header, "w") as fp:
        fp.write(text.replace(old, new))
    saved = {k: getattr(sim, k) for k in ("_HERE", "_LIB", "SOURCE") if hasattr(sim, k)}
    try:
        sim._HERE, sim._LIB = str(here), None
        if "SOURCE" in saved:
            sim.SOURCE = str(here / f"{family}_sim.cpp")
        mutant = sim.lib()                                # compiled with the flags of the simulation's own lib()
    finally:
        for k, x in saved.items():
            setattr(sim, k, x)
    original = sim.lib()
    assert mutant is not original

    def walk(case, trees, geom):
        sim._LIB = mutant                                 # (the walk alone: the brute force stays the unmutated library's)
        try:
            return S.TABLE[family]["walk"](case, trees, geom)
        finally:
            sim._LIB = original
    yield walk


def first_kill(family, walk, iterations, seed=None):
    """the first iteration of the family's sweep in which the walk disagrees with the brute force, or None"""
    for iteration in range(iterations):
        try:
            S.run_host(S.draw(family, S.SUITE_SEED if seed is None else seed, iteration), walk=walk)
        except AssertionError:
            return iteration
    return None


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_planted_faults_are_found(tmp_path, mutant):
    name, family, header, old, new = mutant
    with mutant_library(tmp_path, family, header, old, new) as walk:
        killed = first_kill(family, walk, S.SUITE_ITERATIONS[family])
    print(f"mutant {name} ({header}, sweep of {family}): " + ("survives" if killed is None else f"killed in iteration {killed}"))
    assert killed is not None, f"mutant {name} survives the {S.SUITE_ITERATIONS[family]} iterations of {family}"
