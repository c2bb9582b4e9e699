"""The float top of the stealing grid-node launch (csrc/tr_bvh.h: tr_top_rec, tr_top_fill, tr_top_test, tr_top_build_slot;
csrc/kernels_direct.inc: the table loop in front of the uniform top of wave_traverse_steal): per octant of the ray directions
a heap of the top levels of the tree whose records hold the twelve planes of a grid node as floats, already chosen as entry
and exit planes.  The loop must change NOTHING: (float)q of a 16-bit q is exact, so a record's plane has the bits the
conversion gives, and every lane visits the nodes it visited, on the same trips.

Checked here, on the host (tests/host_sim/float_top_model.cpp: the product's own functions, rays in groups of 64):
  (a) the planes of a record against the definition, bit for bit, and the three compares of tr_top_test against those of
      tr_uniform_test, on random grid nodes with 0 and 65535 among the planes, for all eight octants;
  (b) table loop + uniform top + phase + general loop against uniform top + phase + general loop (uniform_top_sim's
      UNIFORM_TOP), wave by wave: every output bit for bit, node visits, leaf tests and the lost flag per ray, every trip
      count per wave -- on the hierarchies of tests/test_uniform_top_cpu.py (two triangles: a root of two leaves; three: a root
      with a leaf child), with tables deeper than the tree, of the default depth and of three levels (the hand-over to the
      generic loop below the table);
  (c) that the comparison has bite: three deliberately wrong forms inside the model are reported."""
import numpy as np
import pytest

import float_top_sim as F
import uniform_top_cases as C
import uniform_top_sim as U
from sim import SimBVH

Q_ANY, Q_FIRST, Q_CLOSEST = 0, 1, 2
QUERIES = (Q_ANY, Q_FIRST, Q_CLOSEST)
OUTPUTS = {Q_ANY: ("hit",), Q_FIRST: ("tri",), Q_CLOSEST: ("hit", "front", "tri", "loc", "uv")}
LOOP, TABLE = 4, 6      # columns of per_group (F.PER_GROUP)

_SCENES = {}


def scene(case):
    if case not in _SCENES:
        v, f, o, d = C.CASES[case]()
        _SCENES[case] = (v, f, SimBVH(v, f), o, d)
    return _SCENES[case]


def differences(q, a, b):
    bad = [k for k in OUTPUTS[q] if a[k].tobytes() != b[k].tobytes()]
    for j, name in enumerate(F.PER_RAY):
        if not np.array_equal(a["per_ray"][:, j], b["per_ray"][:, j]):
            bad.append(name)
    if a["lost"] != b["lost"]:
        bad.append("lost rays")
    if not np.array_equal(a["per_group"][:, :6], b["per_group"][:, :6]):
        bad.append("per_group")
    return bad


# ---- (a) planes ------------------------------------------------------------------------------------------------------------
def _random_qnodes(n, seed):
    """grid nodes {lo.x | lo.y << 16, lo.z | hi.z << 16, hi.x | hi.y << 16} x 2 children, lo <= hi, with 0 and 65535 among
    the planes"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 65536, (n, 2, 3, 2), dtype=np.int64)
    a[rng.random(a.shape) < 0.08] = 0
    a[rng.random(a.shape) < 0.08] = 65535
    lo, hi = a.min(-1), a.max(-1)                      # (n, child, axis)
    q = np.zeros((n, 8), np.uint32)
    for c in (0, 1):
        q[:, 3 * c + 0] = lo[:, c, 0] | (lo[:, c, 1] << 16)
        q[:, 3 * c + 1] = lo[:, c, 2] | (hi[:, c, 2] << 16)
        q[:, 3 * c + 2] = hi[:, c, 0] | (hi[:, c, 1] << 16)
    q[:, 6] = rng.integers(1, 1000, n)
    q[:, 7] = (~rng.integers(0, 1000, n)).astype(np.int32).view(np.uint32)
    return q, lo, hi


def test_record_planes_are_the_converted_planes_bit_for_bit():
    q, lo, hi = _random_qnodes(256, 5)
    assert (lo == 0).any() and (hi == 65535).any() and (lo == 65535).any() and (hi == 0).any()
    for o in range(8):
        neg = [(o >> ax) & 1 for ax in range(3)]
        for k in range(len(q)):
            rec = F.record(q[k], o)
            want = np.zeros(12, np.float32)
            for c in (0, 1):
                en = [hi[k, c, ax] if neg[ax] else lo[k, c, ax] for ax in range(3)]
                ex = [lo[k, c, ax] if neg[ax] else hi[k, c, ax] for ax in range(3)]
                want[6 * c:6 * c + 6] = [en[0], en[1], ex[0], ex[1], en[2], ex[2]]
            assert rec[:12].tobytes() == want.view(np.uint32).tobytes(), (o, k)
            assert rec[12] == q[k, 6] and rec[13] == q[k, 7] and rec[14] == 0 and rec[15] == 0


@pytest.mark.parametrize("best_t", [np.inf, 1.0])
def test_both_tests_give_the_same_three_compares(best_t):
    q, _, _ = _random_qnodes(64, 6)
    frame = np.float32([-1, -1, -1, 2.0 ** -15, 2.0 ** -15, 2.0 ** -15])
    rng = np.random.default_rng(7)
    seen = np.zeros((8, 3, 2), bool)        # octant, compare, value
    for o in range(8):
        sign = np.float32([-1 if (o >> ax) & 1 else 1 for ax in range(3)])
        d = (rng.random((96, 3)).astype(np.float32) + np.float32(0.05)) * sign
        target = rng.random((96, 3)).astype(np.float32) * 2 - 1
        org = (target - d * np.float32(1.5)).astype(np.float32)
        for k in range(len(q)):
            planes, octant, uni, top = F.tests(q[k], frame, org, d, best_t)
            assert (octant == o).all(), (o, octant[:4])
            assert planes.view(np.uint32).tobytes() == np.tile(F.record(q[k], o)[:12], (len(d), 1)).tobytes()
            assert np.array_equal(uni, top), (o, k)
            for j in range(3):
                seen[o, j, 0] |= (~top[:, j]).any(); seen[o, j, 1] |= top[:, j].any()
    assert seen.all(), "a compare never took one of its values: the rays do not reach the case"


# ---- (b) agreement ---------------------------------------------------------------------------------------------------------
def same_through_the_table(B, o, d, levels, steal_min=F.STEAL_MIN):
    last = None
    for q in QUERIES:
        u = U.query(B, q, o, d, U.UNIFORM_TOP, steal_min)
        t = F.query(B, q, o, d, F.FLOAT_TOP, steal_min, levels=levels)
        u["per_group"] = np.concatenate([u["per_group"], np.zeros((len(u["per_group"]), 1), np.int32)], 1)
        assert differences(q, u, t) == [], (q, levels, differences(q, u, t))
        G = t["per_group"]
        assert (G[:, TABLE] <= np.minimum(G[:, LOOP], levels)).all()
        assert (G[:, TABLE] == np.minimum(G[:, LOOP], levels)).all()      # the table loop runs every trip of the top it has a slot for
        last = t
    return last


@pytest.mark.parametrize("case,levels", [(c, n) for c in C.CASES for n in (F.LEVELS, 3, 1)
                                         if n == F.LEVELS or c != "dense soup"])      # (the large hierarchy once)
def test_the_table_loop_changes_nothing(case, levels):
    v, f, B, o, d = scene(case)
    t = same_through_the_table(B, o, d, levels)
    G = t["per_group"]
    if case == "one triangle":
        assert (G[:, TABLE] == 0).all()
    if case in ("two triangles", "three triangles"):
        assert (G[:, TABLE] == 1).all()                      # the root's leaf child ends the loop on the table's first record
    if case in ("sphere from outside", "64 identical rays", "one 8 x 8 tile"):
        assert (G[:, TABLE] > 0).all() and G[:, TABLE].max() == min(levels, G[:, LOOP].max())
        if levels == 3:
            assert (G[:, LOOP] > G[:, TABLE]).any()          # the generic loop goes on below the table
    if case == "mixed octants":
        assert G[0, TABLE] == 0


def test_absent_slots_are_zero_and_present_ones_are_the_nodes_records():
    v, f, B, o, d = scene("three triangles")                 # a root with a leaf child: half the heap is absent
    top = F.table(B.qnodes, 4).view(np.uint32).reshape(8, 15, 16)
    root = B.qnodes[0]
    kids = root[6:8].view(np.int32)
    assert (kids < 0).sum() == 1
    inner = int(np.argmax(kids >= 0))
    for o8 in range(8):
        assert np.array_equal(top[o8, 0], F.record(root, o8))
        assert np.array_equal(top[o8, 1 + inner], F.record(B.qnodes[kids[inner]], o8))
        assert not top[o8, 2 - inner].any()
        assert not top[o8, 3:].any()                         # the inner child's children are leaves


@pytest.mark.parametrize("steal_min", C.STEAL_MINS)
@pytest.mark.parametrize("case", ["sphere from outside", "64 identical rays", "lane 0 invalid"])
def test_the_give_away_threshold_ends_the_table_loop(case, steal_min):
    v, f, B, o, d = scene(case)
    t = same_through_the_table(B, o, d, F.LEVELS, steal_min)
    assert (t["per_group"][:, TABLE] <= steal_min).all()


# ---- (c) mutants -----------------------------------------------------------------------------------------------------------
def _moved(v):
    """vertices moved as a refit moves them: not an affine map, so the planes on the grid change"""
    w = v.copy()
    w[:, 2] *= (np.float32(1.0) + np.float32(0.35) * w[:, 0])
    w[:, 1] += np.float32(0.2) * w[:, 0] * w[:, 0]
    return w.astype(np.float32)


def test_the_comparison_has_bite():
    caught = {}
    for case, wrong in (("sphere from outside", F.WRONG_OCTANT_0_FOR_ALL), ("sphere from inside", F.WRONG_OCTANT_0_FOR_ALL),
                        ("sphere from outside", F.WRONG_STALE_TABLE),
                        ("rays that miss the root box", F.WRONG_GOES_ON_INTO_AN_ABSENT_SLOT),
                        ("three triangles", F.WRONG_GOES_ON_INTO_AN_ABSENT_SLOT)):
        v, f, B, o, d = scene(case)
        stale = F.table(SimBVH(_moved(v), f).qnodes) if wrong == F.WRONG_STALE_TABLE else None
        for q in QUERIES:
            u = F.query(B, q, o, d, F.UNIFORM_TOP)
            w = F.query(B, q, o, d, wrong, top=stale)
            if differences(q, u, w) != []:
                caught.setdefault(wrong, []).append((case, q))
    for wrong in (F.WRONG_OCTANT_0_FOR_ALL, F.WRONG_STALE_TABLE, F.WRONG_GOES_ON_INTO_AN_ABSENT_SLOT):
        assert caught.get(wrong), f"wrong form {wrong} was not reported by any case"
    # the closest-hit query reports each of them
    assert all(any(q == Q_CLOSEST for _, q in caught[w]) for w in caught)
