"""What tests/test_exact_cpu.py and tests/test_gpu_exact.py assert about one implementation's outputs on the corpora of
tests/exact_ref.py (a helper, not a test module).  An implementation is handed over as `res`, a dict of numpy arrays on
the flattened rays: count, any, first, hit, front, tri, uv (intersects_closest) and list_ray, list_tri (the rows of
intersects_location at cap 8)."""
import functools

import numpy as np

import exact_ref as X
from oracle.oracle import OracleIntersector

ORACLE_KEYS = ("count", "any", "first", "hit", "front", "tri", "loc", "uv", "list_loc", "list_ray", "list_tri")


def oracle_results(R, o, d):
    hit, front, tri, loc, uv, _ = R.closest_raw(o, d)
    cnt = R.intersects_count(o, d)
    ll, lr, lt = R.intersects_location(o, d)
    return dict(count=cnt, any=cnt > 0, first=tri.copy(), hit=hit, front=front, tri=tri, loc=loc, uv=uv, list_loc=ll,
                list_ray=lr, list_tri=lt)


def assert_same(res, exp, what, keys=ORACLE_KEYS):
    for k in keys:
        if k in res:
            g, e = np.asarray(res[k]), np.asarray(exp[k])
            assert g.shape == e.shape and np.array_equal(g, e, equal_nan=g.dtype.kind == "f"), f"{what}: {k} differs from the oracle"


def anchored_mask(R, o, d):
    return (R.anchor(o, d) != o).any(1)


def check_lattice(s, res, anchored, what):
    """section (a): the contract's float64 part is exact on these scenes, so every output equals the ideal rule on the
    rays that stay where they are; the rays the anchor moves no longer run through the lattice and keep the parity"""
    I = X.lattice_ideal(s["name"])
    na = ~anchored
    n, nf = len(na), len(s["f"])
    whole = [not anchored[s["origin_of"] == k].any() for k in range(len(s["origins"]))]
    assert sum(whole) >= 3, f"{what}: only {sum(whole)} origins are compared exactly in full"
    cnt = res["count"]
    bad = np.flatnonzero(na & (cnt != I.count))
    assert len(bad) == 0, f"{what}: count differs from the ideal rule on {len(bad)} rays, the first: o {s['o'][bad[0]]} d {s['d'][bad[0]]}: {cnt[bad[0]]} != {I.count[bad[0]]}"
    assert np.array_equal(res["any"][na], I.count[na] > 0), f"{what}: any"
    assert np.array_equal(res["hit"][na], I.count[na] > 0), f"{what}: closest hit"
    # the list: per ray the set of triangle ids (8 kept: a ray with more hits must list 8 of its ideal set)
    got = np.unique(res["list_ray"].astype(np.int64) * nf + res["list_tri"])
    assert len(got) == len(res["list_ray"]), f"{what}: a triangle is listed twice for one ray"
    full = np.flatnonzero(na & (I.count <= 8))
    want = np.concatenate([r * nf + I.sets[r].astype(np.int64) for r in full] + [np.zeros(0, np.int64)])
    sel = np.isin(got // nf, full)
    assert np.array_equal(got[sel], np.sort(want)), f"{what}: hit lists differ from the ideal sets"
    over = np.flatnonzero(na & (I.count > 8))
    per_ray = np.bincount(res["list_ray"], minlength=n)
    assert np.all(per_ray[over] == 8), f"{what}: a ray with more than 8 hits does not list 8"
    ideal_over = np.concatenate([r * nf + I.sets[r].astype(np.int64) for r in over] + [np.zeros(0, np.int64)])
    assert np.all(np.isin(got[np.isin(got // nf, over)], ideal_over)), f"{what}: a listed triangle is not in the ideal set"
    # the nearest: the smaller face id on exactly equal t; either of two whose exact t differ by less than 2^-20 relative
    assert np.count_nonzero(I.alt >= 0) <= 0.05 * n, f"{what}: {np.count_nonzero(I.alt >= 0)} rays have two nearest distances within 2^-20"
    for key in ("first", "tri"):
        t = res[key]
        ok = (t == I.nearest) | ((I.alt >= 0) & (t == I.alt))
        bad = np.flatnonzero(na & ~ok)
        assert len(bad) == 0, f"{what}: {key} differs from the ideal nearest on {len(bad)} rays, the first: o {s['o'][bad[0]]} d {s['d'][bad[0]]}: {t[bad[0]]} != {I.nearest[bad[0]]}"
    exact_near = na & (res["tri"] == I.nearest) & (I.nearest >= 0)
    assert np.array_equal(res["front"][exact_near], I.front[exact_near]), f"{what}: front"
    q = I.uv[exact_near]
    err = np.abs(res["uv"][exact_near].astype(np.float64) - q)
    assert np.all(err <= np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)), f"{what}: uv off by more than an ulp ({err.max()})"
    # anchored rays: the parity of the ideal count, 0 <-> 2 at a silhouette; a ray through the rim of an open patch
    # has no parity to keep (the moved ray may pass on either side of the rim)
    a = anchored & ~I.border
    diff = np.abs(cnt[a] - I.count[a])
    assert np.all(cnt[a] % 2 == I.count[a] % 2) and np.all((diff == 0) | (diff == 2)), f"{what}: anchored rays {np.unique(diff)}"


@functools.lru_cache(maxsize=None)
def _band_checked(name, tri_bytes):
    """the band check of one run for one set of returned triangles (every implementation returns the same bits, so
    this runs once per run): -> (pairs checked, pairs that meet BAND_K's precondition)"""
    run = next(r for r in X.degenerate_scenes() if r["name"] == name)
    tri = np.frombuffer(tri_bytes, np.int32)
    R = OracleIntersector(run["v"], run["f"], 0)
    oa = R.anchor(run["o"], run["d"])
    hi = np.flatnonzero(tri >= 0)
    c = X.pairs(run["v"], run["f"], oa[hi], run["d"][hi], tri[hi])
    pre = c["pre"]
    assert pre[run["inside"][hi]].all(), f"{name}: a ray from inside leaves the precondition of the band"
    ok = X.above_band(c)
    bad = np.flatnonzero(pre & ~ok)
    assert len(bad) == 0, (f"{name}: {len(bad)} returned triangles lie outside their ray by more than the rounding band, the "
                           f"first: ray {hi[bad[0]]} triangle {tri[hi[bad[0]]]}")
    return len(hi), int(pre.sum())


def check_degenerate(run, res, what):
    """section (b): exactly one crossing from an origin that star_shaped proves, an even number from outside, and every
    returned triangle within the rounding band of its ray"""
    ins = run["inside"]
    cnt = res["count"]
    bad = np.flatnonzero(ins & (cnt != 1))
    assert len(bad) == 0, (f"{what}: {len(bad)} rays from inside a star-shaped solid do not count 1, the first: o {run['o'][bad[0]].tolist()} "
                           f"d {run['d'][bad[0]].tolist()} counts {cnt[bad[0]]}")
    assert res["any"][ins].all() and (res["first"][ins] >= 0).all() and res["hit"][ins].all(), f"{what}: a ray from inside misses"
    bad = np.flatnonzero(~ins & (cnt % 2 != 0))
    assert len(bad) == 0, (f"{what}: {len(bad)} rays from outside count an odd number, the first: o {run['o'][bad[0]].tolist()} "
                           f"d {run['d'][bad[0]].tolist()} counts {cnt[bad[0]]}")
    assert np.array_equal(res["first"], res["tri"]), f"{what}: first != closest tri"
    return _band_checked(run["name"], np.ascontiguousarray(res["tri"], np.int32).tobytes())
