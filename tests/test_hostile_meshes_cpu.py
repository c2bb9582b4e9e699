"""Meshes with NaN, infinite and far-away vertices (tests/hostile_meshes.py) on the oracle and on the host build of the
product headers: what tests/test_gpu_hostile_meshes.py rests on, checked on a machine without a GPU.

For every family (three seeds) and every single case:
  * the conditions that keep a test on it from passing by vacuity (hits, hostile faces, the infinite frame);
  * the oracle's BVH mode returns the bits of its brute force -- the ground truth of every comparison here and on the GPU;
  * the rules that need no oracle (hostile_meshes.check_rules) hold on the oracle's own outputs;
  * every mode of the host simulation (generic, fused 1, 5, 6, the unordered schedule; any, first, closest, count and the
    lists) returns the brute force's bits;
  * the nearest-triangle walk with every stack limit that matters (all entries, one entry: every walk overflows) returns
    the bits of the brute force over the active triangles, and keeps the rules;
  * the host routine of contains_points returns the oracle's counts and decisions;
  * the fused box tests accept what the contract's box test accepts (check_fused, check_fused_wide);
  * the host construction passes bvh_checks.check_structure, which judges NaN and infinite bounds as fminf / fmaxf do."""
import numpy as np
import pytest

import bvh_checks as K
import hostile_meshes as M

CASES = pytest.mark.parametrize("name,seed", M.ALL_CASES, ids=M.CASE_IDS)
# hits the brute force must find at least: the sphere and the deep tree with a third of the rays down its pile give 1 000
# and more; two triangles of which one is active are hit by a ninth of the rays; a mesh without an active face by none
MIN_HITS = {"all_inactive": 0, "one_triangle_nan": 0, "one_triangle_inf": 0, "two_triangles_nan": 300, "two_triangles_inf": 300}
INFINITE_FRAME = ("nonfinite", "faraway_nonfinite", "faraway", "all_inactive")
SIM_MODES = (("generic", 0, False), ("fused 1", 1, False), ("fused 5", 5, False), ("fused 6", 6, False), ("unordered schedule", 0, True))
DEFAULT_DIRECTION = np.array([0.4395064455, 0.617598629942, 0.652231566745], np.float32)


def host_structure(c):
    from sim import SimBVH
    B = SimBVH(c.v, c.f)
    mn, mx = K.bounds_of(K.padded_boxes(c.v, c.f))
    info = dict(depth=B.depth, aabb_min=mn.tolist(), aabb_max=mx.tolist())
    return B, info


@CASES
def test_conditions_on_the_batch(name, seed):
    c = M.case(name, seed)
    exp = M.oracle(name, seed)
    hit, tri = exp["closest"][0], exp["closest"][2]
    assert int(hit.sum()) >= MIN_HITS.get(name, 1000), int(hit.sum())
    assert c.hostile.any() or name == "unreferenced_nan_vertex"
    assert len(c.f) <= 400 and len(c.o) >= 3000 and len(c.p) == 600
    if name in ("nonfinite", "faraway_nonfinite", "deep_nan", "holed_sphere", "all_nan_triangle", "two_triangles_nan", "two_triangles_inf"):
        assert c.inactive.any() and not c.inactive.all()
        assert np.ptp(np.flatnonzero(c.inactive)) >= len(c.f) // 2 or c.inactive.sum() <= 11 or len(c.f) == 2      # spread over the ids
    if name in ("faraway", "denormal", "unreferenced_nan_vertex"):
        assert not c.inactive.any()
    if name in ("all_inactive", "one_triangle_nan", "one_triangle_inf"):
        assert c.inactive.all()
    if name == "unreferenced_nan_vertex":
        assert np.isnan(c.v).any() and np.isfinite(c.v[c.f]).all()
    B, _ = host_structure(c)
    assert np.all(np.isinf(B.frame[:3])) == (name in INFINITE_FRAME), B.frame
    if name == "deep_nan":
        assert B.depth > 32 and B.key_mode == 1, B.depth
    if name == "denormal":
        assert np.abs(c.v).max() < np.finfo(np.float32).tiny and np.abs(c.v).max() > 0
    keep = M.same_anchor(name, seed)
    # (a single active triangle has a flat frame that most rays start far from: a fifth of its hits stay comparable)
    need = 50 if name.startswith("two_triangles") else 0.9 * hit.sum()
    assert int((hit & keep).sum()) >= need, "the rule about the active faces must cover a good part of the hits"
    # the far-away triangles are ordinary triangles that no ray of these batches reaches within tmax = 1e7
    assert set(np.unique(tri[hit])) <= set(np.flatnonzero(~c.inactive))


@CASES
def test_oracle_bvh_mode_returns_the_brute_force_bits(name, seed):
    brute, bvh = M.oracle(name, seed, 0), M.oracle(name, seed, 1)
    for k, (a, b) in enumerate(zip(brute["closest"], bvh["closest"])):
        assert M._same(a, b), f"closest output {k}"
    assert np.array_equal(brute["count"], bvh["count"])
    for a, b in zip(brute["location"] + (brute["location_t"],), bvh["location"] + (bvh["location_t"],)):
        assert M._same(a, b), "location lists"


@CASES
def test_oracle_keeps_the_rules(name, seed):
    c, exp, alone, keep = M.case(name, seed), M.oracle(name, seed), M.oracle_active(name, seed), M.same_anchor(name, seed)
    M.check_rules(c, "closest", exp["closest"], alone["closest"], keep, "oracle")
    M.check_rules(c, "first", exp["closest"][2], alone["closest"][2], keep, "oracle")
    M.check_rules(c, "count", exp["count"], alone["count"], keep, "oracle")
    M.check_rules(c, "any", exp["count"] > 0, alone["count"] > 0, keep, "oracle")
    M.check_rules(c, "location", exp["location"], alone["location"], keep, "oracle")
    assert np.array_equal(exp["closest"][0], exp["count"] > 0)


@CASES
def test_host_simulation_returns_the_brute_force_bits(name, seed):
    import sim
    from sim import SimBVH
    c, exp, keep = M.case(name, seed), M.oracle(name, seed), M.same_anchor(name, seed)
    fa, _ = M.active_faces(c.v, c.f)
    try:
        for label, fused, unordered in SIM_MODES:
            sim.use_fused(fused)
            sim.use_unordered(unordered)
            B = SimBVH(c.v, c.f)
            if fused == 6 and B.depth > 32:          # the 32-bit state of mode 6 holds 32 levels
                continue
            A = SimBVH(c.v, fa) if len(fa) else None
            what = f"{label} / {c.name}"
            for query, q in (("closest", 2), ("count", 3), ("any", 0), ("first", 1)):
                got = B.query(q, c.o, c.d)
                alone = A.query(q, c.o, c.d) if A is not None else None
                if query == "closest":
                    got, alone = (tuple(r[k] for k in ("hit", "front", "tri", "loc", "uv")) if r is not None else None for r in (got, alone))
                    for key, g, e in zip(("hit", "front", "tri", "loc", "uv"), got, exp["closest"]):
                        assert M._same(g.reshape(e.shape), e), f"{what}: closest {key}"
                else:
                    key = {"count": "count", "any": "hit", "first": "tri"}[query]
                    got, alone = got[key], (alone[key] if alone is not None else None)
                    e = {"count": exp["count"], "any": exp["count"] > 0, "first": exp["closest"][2]}[query]
                    assert np.array_equal(got, e), f"{what}: {query}"
                if alone is not None:
                    M.check_rules(c, query, got, alone, keep, f"{what}, the simulation's own outputs")
            cnt, ltri, lt = B.location(c.o, c.d)
            rows = np.arange(8)[None, :] < np.minimum(cnt, 8)[:, None]
            assert np.array_equal(cnt, exp["count"]) and np.array_equal(ltri[rows], exp["location"][2]) and M._same(lt[rows], exp["location_t"]), f"{what}: location"
            assert np.isfinite(lt[rows]).all() and not c.inactive[ltri[rows]].any(), f"{what}: location"
    finally:
        sim.use_fused(0)
        sim.use_unordered(False)


@CASES
def test_nearest_walk_returns_the_brute_force_bits(name, seed):
    import nearest_cases as NC
    import nearest_sim
    from sim import SimBVH
    c = M.case(name, seed)
    fa, _ = M.active_faces(c.v, c.f)
    brute = nearest_sim.brute(c.v, c.f, c.p)
    M.check_nearest_rules(c, brute, nearest_sim.brute(c.v, fa, c.p), f"brute force / {c.name}")
    assert (brute[2] >= 0).all() == (not c.inactive.all())
    B = SimBVH(c.v, c.f)
    for entries in (0, 1):
        got = nearest_sim.walk(B, c.p, entries, want_lost=True)
        NC.assert_same_bits(got[:3], brute, f"walk with stack_entries {entries} / {c.name}")
        assert got[3].all() == (entries == 1 and len(c.f) > 2), "one entry must overflow on every walk of a hierarchy"
    # the independent numpy evaluation agrees that the winner is a minimiser among the active triangles (not where active
    # coordinates reach FLT_MAX or are all denormal: its tolerances, in units of the largest coordinate, say nothing there)
    if name not in ("denormal", "faraway", "faraway_nonfinite") and len(fa):
        NC.check_against_numpy(c.v, c.f, c.p, *brute, c.name)


@CASES
def test_points_routine_matches_the_oracle(name, seed):
    import points_sim
    from oracle.oracle import OracleIntersector
    from sim import SimBVH
    c = M.case(name, seed)
    B = SimBVH(c.v, c.f)
    R = OracleIntersector(c.v, c.f, 0)
    box = (np.float32([-1.25] * 3), np.float32([1.25] * 3)) if name != "denormal" else (np.float32([-1.25e-39] * 3), np.float32([1.25e-39] * 3))
    for d in (DEFAULT_DIRECTION, np.array([-0.3, 0.2, 0.9], np.float32)):
        got = points_sim.contains(B, c.p, d, box)
        dirs = np.tile(d, (len(c.p), 1))
        cp, cm = R.intersects_count(c.p, dirs), R.intersects_count(c.p, -dirs)
        assert np.array_equal(got["counts"], np.stack([cp, cm])), c.name
        odd = (cp & 1).astype(bool) & (cm & 1).astype(bool)
        in_box = (c.p > box[0]).all(1) & (c.p < box[1]).all(1)
        assert np.array_equal(got["inside"], in_box & odd) and np.array_equal(got["broken"], ~odd & ((cp == 0) | (cm == 0))), c.name
    if name in M.FAMILIES or name in ("all_nan_triangle", "unreferenced_nan_vertex", "denormal"):
        assert 0.1 < got["inside"].mean() < 0.9, c.name            # the sphere is closed: its inside is found


@CASES
def test_fused_box_tests_contain_the_contracts(name, seed):
    c = M.case(name, seed)
    B, _ = host_structure(c)
    if len(c.f) < 2:
        return
    bad, pairs, fused, contract = B.check_fused(c.o, c.d)
    assert pairs >= len(c.o) * (len(c.f) - 1) and bad == 0 and fused >= contract, (bad, pairs, fused, contract)
    badw, pairsw, fw, cw = B.check_fused_wide(c.o, c.d)
    assert pairsw > 0 and badw == 0 and fw >= cw, (badw, pairsw, fw, cw)


@CASES
def test_host_construction_passes_the_structure_checks(name, seed):
    c = M.case(name, seed)
    B, info = host_structure(c)
    K.check_structure(c.v, c.f, B.nodes, B.links, B.tris, B.qnodes, B.frame, info, ref_frame=B.frame)
    assert B.depth <= 64
