"""The oracle (brute force and BVH) and the host simulation of the product headers against the integer-arithmetic
reference of tests/exact_ref.py, on scenes made of exact ties and of near-ties.

Section (a), lattice scenes: integer vertices, origins and directions below 2^11, where the float64 part of the contract
(csrc/tr_math.h, contract 3) is exact -- count, any-hit, the hit list, the nearest triangle, front and uv must EQUAL
what the ideal rule gives, ray by ray, on every ray the anchor leaves in place.  Section (b), near-degenerate scenes,
where float64 rounds: from an origin that exact_ref.star_shaped proves, every ray crosses the surface exactly once; from
outside an even number of times; and every returned triangle lies within the rounding band of its ray (exact_ref's
docstring derives the band from the source text of tr_woop64_xyz).

test_the_corpora_bite is the condition under which the rest means anything: section (a) is made of ties (every tie
code under both orientations), section (b) of pairs where float64 really rounds -- edge functions that float64 calls
zero and that are not, and ones within the band that float64 keeps.  Tie code 7 (U = V = W = 0: the ray lies in the
triangle's plane) has det = 0 and therefore no orientation and never a hit; it is required to occur, once."""
import numpy as np
import pytest

import exact_checks as K
import exact_ref as X
import sim
from oracle.oracle import OracleIntersector
from sim import SimBVH

Q_ANY, Q_FIRST, Q_CLOSEST, Q_COUNT = 0, 1, 2, 3
LATTICE = [s["name"] for s in X.lattice_scenes()]
DEGENERATE = [r["name"] for r in X.degenerate_scenes()]


def sim_results(v, f, o, d):
    B = SimBVH(v, f)
    c = B.query(Q_CLOSEST, o, d)
    cnt, ltri, _ = B.location(o, d)
    ray, col = np.nonzero(np.arange(8)[None, :] < np.minimum(cnt, 8)[:, None])
    return dict(count=B.query(Q_COUNT, o, d)["count"], any=B.query(Q_ANY, o, d)["hit"], first=B.query(Q_FIRST, o, d)["tri"],
                hit=c["hit"], front=c["front"], tri=c["tri"], loc=c["loc"], uv=c["uv"], list_ray=ray.astype(np.int32),
                list_tri=ltri[ray, col])


def implementations(v, f, o, d):
    """(name, results) of the oracle's two modes; they and the host simulation must agree bit for bit (the simulation
    walks a fan of 2 000 slivers around one point node by node: there it gets every fourth ray)"""
    brute = K.oracle_results(OracleIntersector(v, f, 0), o, d)
    bvh = K.oracle_results(OracleIntersector(v, f, 1), o, d)
    K.assert_same(bvh, brute, "oracle BVH")
    step = 4 if len(f) > 1000 else 1
    sub = K.oracle_results(OracleIntersector(v, f, 0), o[::step], d[::step]) if step > 1 else brute
    K.assert_same(sim_results(v, f, o[::step], d[::step]), sub, "host simulation")
    return [("oracle brute force", brute), ("oracle BVH", bvh)]


@pytest.mark.parametrize("name", LATTICE)
def test_lattice_scene_equals_the_ideal_rule(name):
    s = next(s for s in X.lattice_scenes() if s["name"] == name)
    anchored = K.anchored_mask(OracleIntersector(s["v"], s["f"], 0), s["o"], s["d"])
    for impl, res in implementations(s["v"], s["f"], s["o"], s["d"]):
        K.check_lattice(s, res, anchored, f"{name} / {impl}")


@pytest.mark.parametrize("name", DEGENERATE)
def test_near_degenerate_scene_has_one_crossing_from_inside(name):
    run = next(r for r in X.degenerate_scenes() if r["name"] == name)
    for o in run["stars"]:
        assert X.star_shaped(run["v"], run["f"], o), f"{name}: not star-shaped from {o}"
    for impl, res in implementations(run["v"], run["f"], run["o"], run["d"]):
        K.check_degenerate(run, res, f"{name} / {impl}")


@pytest.mark.parametrize("name", [s["name"] for s in X.lattice_scenes() if s["closed"]] + [n for n in DEGENERATE if n.startswith("tetra")])
def test_oracle_contains_points_on_closed_scenes(name):
    """integer points and points at odd multiples of 1/2 against the parity of ideal crossings along an axis"""
    s = next(s for s in X.lattice_scenes() + X.degenerate_scenes() if s["name"] == name)
    p, inside = X.lattice_points(s) if name in LATTICE else X.tetra_points(s)
    assert 0.1 < inside.mean() < 0.9
    for mode in (0, 1):
        got = OracleIntersector(s["v"], s["f"], mode).contains_points(p, _retry_dirs=iter([np.float32([0.3, -0.2, 0.45])] * 4))
        assert np.array_equal(got, inside), f"{name} mode {mode}: {int((got != inside).sum())} points"


def test_the_corpora_bite():
    rays = ties = 0
    codes = np.zeros(16, np.int64)
    for s in X.lattice_scenes():
        I = X.lattice_ideal(s["name"])
        rays += len(I.tie)
        ties += int(I.tie.sum())
        codes += I.codes
    assert ties >= 0.3 * rays, f"(a): {ties} of {rays} rays have an exact tie"
    assert all(codes[c] > 0 and codes[c | 8] > 0 for c in range(1, 7)) and codes[7] > 0, f"(a): tie codes seen {codes.tolist()}"
    zero_not = in_band = 0
    for run in X.degenerate_scenes():
        oa = OracleIntersector(run["v"], run["f"], 0).anchor(run["o"], run["d"])
        c = X.pairs(run["v"], run["f"], oa, run["d"], run["tri"])
        uvw, code = sim.woop_pairs(oa, run["d"], run["v"][run["f"][run["tri"]]].reshape(-1, 9))
        signs = np.stack([c["sU"], c["sV"], c["sW"]], 1)
        # where float64 is exact the two agree in every sign and in the tie code
        for k in range(3):
            zero_not += int(np.count_nonzero((uvw[:, k] == 0) & (signs[:, k] != 0)))
            in_band += int(np.count_nonzero((uvw[:, k] != 0) & X.in_band(c, k)))
    assert zero_not >= 1000, f"(b): {zero_not} edge functions are zero in float64 and not in integers"
    assert in_band >= 1000, f"(b): {in_band} edge functions within the rounding band are kept by float64"


def test_host_export_equals_the_integer_reference_where_float64_is_exact():
    """tr_woop64's U, V, W and tie code against the integer ones on the lattice scenes (every product below 2^53)"""
    for s in X.lattice_scenes()[:6]:
        rng = np.random.default_rng(len(s["f"]))
        i = rng.integers(0, len(s["o"]), 4000)
        t = rng.integers(0, len(s["f"]), 4000)
        c = X.pairs(s["v"], s["f"], s["o"][i], s["d"][i], t)
        uvw, code = sim.woop_pairs(s["o"][i], s["d"][i], s["v"][s["f"][t]].reshape(-1, 9))
        for k, key in enumerate(("U", "V", "W")):
            assert np.array_equal(uvw[:, k], c[key].astype(np.float64)), (s["name"], key)
        want = np.where((c["sU"] == 0) & (c["sV"] == 0) & (c["sW"] == 0), 7, c["code"])
        assert np.array_equal(code, want), s["name"]
