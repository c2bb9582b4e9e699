"""The box, triangle and plane predicates (csrc/tr_boxes.h, tr_tris.h, tr_planes.h, built for the host: tests/host_sim/*_sim.brute)
against EXACT arithmetic on ordinary float32 inputs -- full mantissas, nothing on a lattice (tests/offgrid_cases.py).

The GPU tests compare the kernels bit for bit with these brute forces, which are the same headers compiled with g++: a mistake
in a header is made on both sides.  The lattice tests (test_boxes_cpu.py, test_tris_cpu.py, test_planes_cpu.py) hold the headers
to geometry only where float64 -- and much of float32 -- rounds nothing.  Here float64 rounds: the queries touch a face within
+-2 float32 steps, on meshes at unit scale, far from the origin, at both ends of the float32 range, scaled per axis, denormal,
and exactly coplanar off the lattice.  A header that takes a difference or a product in float32, or is built with contraction
on, fails here (DESIGN.md section 9 has the counts).

Recorded on the shipped headers: boxes agree with the exact tables on every pair of every family (591 600 pairs, 0 left out);
triangles on every pair (609 600) but 3 exact ties of `flat` -- a line p .. q whose rounded ends leave a vertex of the face
EXACTLY on it, which the float64 axis n x f calls apart; planes: 0 pairs below the bound, 0 rows on ill-conditioned edges, the
largest distance of a crossing point from the exact rational point 0.49999919 float32 steps (profiles/offgrid_planes.jsonl)."""
import json
import os

import numpy as np
import pytest

import boxes_cases as BC
import offgrid_cases as OC
import planes_cases as PC
import tris_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.float32(np.finfo(np.float32).max)


# ---- 1. float32 values as integers -------------------------------------------------------------------------------------------
def test_exact_ints_round_trip_at_the_ends_of_the_range():
    tiny = np.float32(2.0 ** -149)
    a = np.float32([FLT_MAX, -FLT_MAX, 1.0, 0.0, -0.0])
    b = np.float32([[tiny, -tiny, 3 * tiny], [np.float32(2.0 ** -126), np.float32(2.0 ** -127), np.float32(-1.5 * 2.0 ** -140)]])
    A, B, e = OC.exact_ints(a, b)
    assert e == -149 and A.shape == a.shape and B.shape == b.shape and A.dtype == object
    assert all(type(k) is int for k in A.tolist()) and all(type(k) is int for row in B.tolist() for k in row)
    assert A.tolist() == [(2 ** 24 - 1) << (104 + 149), -((2 ** 24 - 1) << (104 + 149)), 1 << 149, 0, 0]
    assert B.tolist() == [[1, -1, 3], [1 << 23, 1 << 22, -(3 << 8)]]
    # 2^-149 next to 1.0: one scale for both, differences and products of the integers are exact
    one, least, e = OC.exact_ints(np.float32([1.0]), np.float32([tiny]))
    assert (one[0], least[0], e) == (1 << 149, 1, -149) and one[0] - least[0] == (1 << 149) - 1
    # the scale is the smallest exponent present, no smaller: small integers for ordinary inputs
    x, e = OC.exact_ints(np.float32([0.75, -2.5, 4096.0]))
    assert e == -2 and x.tolist() == [3, -10, 16384]
    z, e = OC.exact_ints(np.zeros((2, 3), np.float32))
    assert e == 0 and z.tolist() == [[0, 0, 0], [0, 0, 0]]
    for bad in (np.float32([np.nan]), np.float32([np.inf]), np.float64([1.0])):
        with pytest.raises(AssertionError):
            OC.exact_ints(bad)


def test_families_are_off_the_lattice_and_without_degenerate_faces():
    for name in OC.FAMILIES:
        v, f = OC.family(name)                                    # (asserts that no face is degenerate under the exact normal)
        assert v.dtype == np.float32 and np.isfinite(v).all() and len(f) == (60 if name == "flat" else 80)
        V, _ = OC.exact_ints(v[:, :2] if name == "flat" else v)
        # significant bits from the first to the last set one: 24 at the most, about 19 for the denormal values near 2^-130
        bits = [abs(k).bit_length() - ((k & -k).bit_length() - 1) for row in V.tolist() for k in row if k]
        assert np.median(bits) >= 17, f"{name}: the mantissas are not full"
    assert (OC.family("flat")[0][:, 2] == OC.FLAT_Z).all()
    d = np.abs(OC.family("denormal")[0])
    assert d.max() < np.finfo(np.float32).tiny and (d > 0).sum() > 100


# ---- 2. boxes and triangles -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.FAMILIES)
def test_generated_boxes_and_triangles_meet_their_conditions(name):
    """valid queries, 20 % .. 80 % of the aimed pairs of every kind meet, a series of every kind flips between k = -2 and
    k = +2, and on `flat` every aimed pair is exactly coplanar"""
    for sort in ("triangles", "boxes"):
        stats = OC.check_inputs(name, sort)
        print(f"{name}, {sort}: (aimed pairs, of which meet, series that flip) per kind: {stats}")


@pytest.mark.parametrize("name", OC.FAMILIES)
def test_triangles_equal_exact_geometry(name):
    import tris_sim
    v, f = OC.family(name)
    tri = OC.tri_queries(name).data
    res = tris_sim.brute(v, f, tri)
    TC.check_identities(res, f"{name}, triangles")
    left = OC.check_sets(name, "triangles", TC.listed(res, len(tri), len(f)), res)
    want = OC.tri_table(name)
    print(f"{name}, triangles: {want.size} pairs, {int(want.sum())} meet, {left} exact ties left out")


@pytest.mark.parametrize("name", OC.FAMILIES)
def test_boxes_equal_exact_geometry(name):
    import boxes_sim
    v, f = OC.family(name)
    lo, hi = OC.box_queries(name).data
    res = boxes_sim.brute(v, f, lo, hi)
    BC.check_identities(res, f"{name}, boxes")
    left = OC.check_sets(name, "boxes", BC.listed(res, len(lo), len(f)), res)
    want = OC.box_table(name)
    print(f"{name}, boxes: {want.size} pairs, {int(want.sum())} meet, {left} exact ties left out")


def test_what_counts_as_an_exact_tie():
    """tri_tie / box_tie on pairs whose class is known: touching pairs are ties, crossing pairs and pairs apart are not, and a
    coplanar pair whose interiors overlap is none although everything projects to one point on its normal"""
    t = ((0, 0, 0), (4, 0, 0), (0, 4, 0))
    assert OC.tri_tie(t, ((4, 0, 0), (8, 0, 0), (4, 4, 3)))                     # a shared vertex
    assert OC.tri_tie(t, ((1, 1, 0), (1, 1, 5), (2, 1, 5)))                     # a vertex on the interior
    assert OC.tri_tie(t, ((2, 2, 0), (6, 2, 0), (2, 6, 0)))                     # coplanar, a vertex on an edge
    assert not OC.tri_tie(t, ((1, 1, 0), (3, 1, 0), (1, 3, 0)))                 # coplanar, one inside the other
    assert not OC.tri_tie(t, ((1, 1, -2), (1, 1, 5), (2, 1, 5)))                # through the interior
    assert not OC.tri_tie(t, ((1, 1, 1), (1, 1, 5), (2, 1, 5)))                 # apart
    assert OC.box_tie((1, 1, 0), (2, 2, 3), t)                                  # a box standing on the face
    assert OC.box_tie((4, -1, -1), (5, 1, 1), t)                                # a box face through a vertex
    assert not OC.box_tie((1, 1, -1), (2, 2, 3), t)                             # through the interior
    assert not OC.box_tie((1, 1, 1), (2, 2, 3), t)                              # apart


# ---- 3. planes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.FAMILIES)
def test_planes_equal_exact_signs_and_crossing_points(name):
    """both predicates on every decisive pair, vertex ends by their bits, crossing points within one float32 step of the exact
    rational point (the derivation: offgrid_cases.check_planes); the reference's own rows all run along (face normal) x (plane
    normal) (asserted where it is built).  The largest error is compared with the recorded one only for being no larger than
    the bound: the bound is derived, the record is a measurement."""
    import planes_sim
    stats = OC.check_plane_inputs(name)
    v, f = OC.family(name)
    o, nr = OC.plane_queries(name).data
    met, cut = planes_sim.brute(v, f, o, nr, cut=False), planes_sim.brute(v, f, o, nr, cut=True)
    for res in (met, cut):
        PC.check_identities(res, f"{name}, planes")
    left, ill, rows, worst = OC.check_planes(name, met, cut, PC.listed)
    print(f"{name}, planes: (queries, aimed s > 0, aimed s == 0) per kind {stats}; {left} pairs below the bound, {ill} rows on "
          f"ill-conditioned edges, {rows} rows compared, the largest crossing error {worst:.8f} float32 steps")


def test_the_recorded_plane_figures_are_those_of_the_families():
    """profiles/offgrid_planes.jsonl holds one line per family: what test_planes_equal_exact_signs_and_crossing_points printed
    when it was recorded.  The counts are properties of the generated inputs and the exact reference alone and must still hold;
    the error is a record, bounded by one step"""
    with open(os.path.join(ROOT, "profiles", "offgrid_planes.jsonl")) as fh:
        lines = [json.loads(x) for x in fh if x.strip()]
    assert [x["family"] for x in lines] == list(OC.FAMILIES)
    for x in lines:
        ref = OC.planes_reference(x["family"])
        assert x["pairs"] == ref.meets.size and x["meet"] == int(ref.meets.sum()) and x["cut"] == int(ref.cut.sum())
        assert x["below_the_bound"] == int((~ref.decisive).sum()) == 0
        assert 0 < x["largest_crossing_error_steps"] <= 1
