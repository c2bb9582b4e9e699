"""Every launch flavour on rays at the ends of the float range (tests/hostile_rays.py builds them).

The flavour matrix (tests/test_gpu_kernel_matrix.py) compares every kernel with the oracle on ordinary rays.  What
tr_ray_setup, tr_inv and tr_ray_anchor (csrc/tr_math.h) and tr_fuse_axis (csrc/tr_bvh.h) promise for everything else --
a non-finite component misses, a zero or denormal direction component gets a clamped reciprocal, beyond M = 1e30 an axis is
ignored, kd = inf beyond 2^40 -- is where a gfx950 build and an x86 build of the same header are most likely to part:
NaN operands of fminf / fmaxf chains that the compiler folds into three-operand forms, denormal reciprocals and hit
distances under -fno-gpu-flush-denormals-to-zero, products that overflow in the packed-fma node test, selector words taken
from the sign of a clamped reciprocal.  And the work distribution (stealing, hand-over, streaming refill, 8-wide) meets
whole waves of rays that are dead from the start, and dead rays beside live ones, on hierarchies of more than one node.

Per case (query x addressing x launch shape, as in the flavour matrix), scene (soup, shells, deep tree) and layout
(interleaved, blocked), two launches -- the second on the learned order -- each checked for
  * the oracle's bits on every ray and every output;
  * the launch record (direct shapes) or its absence (streaming);
  * the rules of hostile_rays.check_rules, which need no oracle: invalid rays return the miss and own no list rows, the
    ordinary rays return what the same flavour returns for them alone, a direction scaled by 2^k (k >= -10) returns the
    unscaled ray's bits, no output holds a non-finite float;
  * the float64 geometry of tests/geom64.py on the robust rays -- more than 0.9 of each family it covers: the ordinary
    rays, scale:k for k >= -10, comp:*, all:3e38 (the two 3e38 families with the direction rescaled by 2^-126 in float64,
    hostile_rays.F64_RESCALED); far:* and origin:* are exempt (origins of 2^60 and more leave float64 no robust rays).
The record forms and contains_points follow once each.

The CPU part (no marker) pins the same on the oracle and on the host simulation of the product headers, so that the GPU
part rests on something a machine without a GPU has checked: the conditions on the batch, the rules, the oracle's BVH mode
against its brute-force mode, the float64 geometry, and the fused box tests on families 3 to 5."""
import numpy as np
import pytest

import hostile_rays as H
from launch_options import options
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)
from test_gpu_kernel_matrix import ADDRESSING, QUERIES, SHAPES, check_query, expect_launch, run_query

SCENES_OF = {"compact": ("soup", "shells"), "deep": ("deep",), "generic": ("soup", "shells", "deep")}
LAYOUTS = ("interleaved", "blocked")


def T(x, dev):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to(dev)           # (a copy: the shared batches are read-only)


def host(got):
    """what a query returned, as numpy arrays in the form hostile_rays.check_rules takes"""
    return tuple(g.cpu().numpy() for g in got) if isinstance(got, (tuple, list)) else got.cpu().numpy()


def check_everything(name, layout, query, got, alone, what):
    batch, exp = H.expected(name, layout)
    check_query(query, got, exp, what)
    g = host(got)
    H.check_rules(batch, query, g, alone, what)
    if query in ("any", "first", "closest"):
        hit, tri, loc = (g, None, None) if query == "any" else (None, g, None) if query == "first" else (g[0], g[2], g[3])
        H.check_geometry(H.geometry_f64(name, layout), hit, tri, loc, what)


# ---- GPU part ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("addressing", list(ADDRESSING))
@pytest.mark.parametrize("query", QUERIES)
def test_flavour_on_hostile_rays(device, query, addressing, shape):
    import torch
    opts, queries, flavours, why = SHAPES[shape]
    if query not in queries or addressing not in flavours:
        pytest.skip(why)
    from triro.ray.ray_optix import RayMeshIntersector
    streaming = shape.startswith("stream")

    def record(r, what, carried=0):
        if streaming:
            with pytest.raises(ValueError, match="no direct launch"):
                r.as_wrapper.last_launch()
            return None
        li = expect_launch(r, query, shape, addressing, what)
        assert carried is None or li["sort_carried"] == carried, f"{what}: {li}"
        return li

    for name in SCENES_OF[addressing]:
        v, f, o, d = H.scene(name)[:4]
        for layout in LAYOUTS:
            batch, _ = H.expected(name, layout)
            what = f"{query} / {addressing} / {shape} / {name} / {layout}"
            with options(compact=0 if addressing == "generic" else 1, **opts):
                r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
                depth = r.bvh_info()["depth"]
                assert depth > 32 if addressing == "deep" else (depth <= 32 or addressing == "generic"), (name, depth)
                # the ordinary rays alone, in the same flavour
                alone = host(run_query(r, query, T(o, device), T(d, device)))
                record(r, f"{what}, the ordinary rays alone", carried=None)
                ot, dt = T(batch.o, device), T(batch.d, device)
                if shape == "sort_carried":
                    # the deferred sort of the learned order rides in a later launch of the same batch shape: every launch
                    # is checked until one has carried it
                    for k in range(16):
                        check_everything(name, layout, query, run_query(r, query, ot, dt), alone, f"{what} launch {k}")
                        if record(r, f"{what} launch {k}", carried=None)["sort_carried"]:
                            break
                    else:
                        raise AssertionError(f"{what}: no launch of 16 carried the sort")
                    continue
                for k in range(2):                    # the second launch runs on the learned order
                    check_everything(name, layout, query, run_query(r, query, ot, dt), alone, f"{what} launch {k}")
                    record(r, f"{what} launch {k}")
                torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_record_forms_on_hostile_rays(device, layout):
    """packed records in face and slot form and bare slots, expanded with and without row_length: the dense call's bits,
    which are the oracle's.  Whole batch (16 rays per row: no 8 x 8 tiles over 1031 rows) and its first 16384 rays as 512
    rows of 32 (tiled)."""
    import torch
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = H.scene("soup")[:2]
    batch, exp = H.expected("soup", layout)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    for m, width in ((batch.n, 16), (16384, 32)):
        assert m % width == 0 and m <= batch.n
        ot, dt = T(batch.o[:m], device), T(batch.d[:m], device)
        dense = r.intersects_closest(ot, dt)
        for name_, g, e in zip(("hit", "front", "tri", "loc", "uv"), dense, exp["closest"]):
            assert np.array_equal(g.cpu().numpy(), e[:m]), f"{layout}, {m} rays: closest {name_} against the oracle"
        rec_f, rec_s = r.intersects_closest_packed(ot, dt), r.intersects_closest_packed(ot, dt, slots=True)
        slot = r.intersects_closest_slots(ot, dt)
        dead = torch.from_numpy(batch.mask(*H.INVALID)[:m]).to(device)
        assert bool((slot[dead] == -1).all()) and bool((rec_f[dead][:, 0] < 0).all()) and bool((rec_s[dead][:, 0] < 0).all())
        forms = {"faces": r.closest_expand(rec_f), "slot records": r.closest_expand(rec_s, slots=True),
                 "slot records in rows": r.closest_expand(rec_s, slots=True, row_length=width),
                 "slots": r.closest_from_slots(ot, dt, slot), "slots in rows": r.closest_from_slots(ot, dt, slot, row_length=width)}
        for form, got in forms.items():
            for name_, a, e in zip(("hit", "front", "tri", "loc", "uv"), got, dense):
                assert torch.equal(a, e), f"{layout}, {m} rays, {form}: {name_} differs from the dense call"


def hostile_points():
    """4096 hash points around the shells, every fourth with one component at an end of the float range
    -> (points, which are hostile)"""
    import workloads as W
    p = W.hash_rays(4096, 63, [-1.1] * 3, [1.1] * 3)[0]
    values = np.array([np.nan, 0.0, np.inf, -np.inf, 3.4e38, -3.4e38], np.float32)
    values[1] = np.uint32(0xFFC00000).view(np.float32)          # NaN with the sign bit
    bad = np.arange(0, len(p), 4)
    p[bad, np.arange(len(bad)) % 3] = values[(np.arange(len(bad)) // 3) % len(values)]
    mask = np.zeros(len(p), bool)
    mask[bad] = True
    return p, mask


RETRY = (0.3, -0.45, 0.2)        # in place of the reference's random retry direction, for the oracle and the GPU alike


def oracle_contains(points):
    from oracle.oracle import OracleIntersector
    v, f = H.scene("shells")[:2]
    return OracleIntersector(v, f, 1).contains_points(points, _retry_dirs=iter([np.array(RETRY, np.float32)] * 4))


@pytest.mark.gpu
def test_contains_points_with_hostile_points(device):
    import torch
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = H.scene("shells")[:2]
    p, bad = hostile_points()
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    retry = torch.tensor(RETRY, dtype=torch.float32)
    got = r.contains_points(T(p, device), _retry_direction=retry).cpu().numpy()
    alone = r.contains_points(T(p[~bad], device), _retry_direction=retry).cpu().numpy()
    want = oracle_contains(p)
    assert 0.1 < want[~bad].mean() < 0.9
    assert not got[bad].any(), "a point with a non-finite or 3.4e38 component is reported inside"
    assert np.array_equal(got[~bad], alone), "ordinary points differ from what they return alone"
    assert np.array_equal(got, want), "contains_points differs from the oracle"


# ---- CPU part: the oracle and the host simulation of the product headers --------------------------------------------------
ALL_SCENES = ("soup", "shells", "deep")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ALL_SCENES)
def test_oracle_keeps_the_rules_on_hostile_rays(name, layout):
    """H.expected asserts the conditions on the batch (hit shares, family sizes); here: the rules on the oracle's own
    outputs, its BVH mode against its brute-force mode on every ray, and the float64 geometry"""
    from oracle.oracle import OracleIntersector
    v, f, _, _, _, alone = H.scene(name)
    batch, exp = H.expected(name, layout)
    what = f"oracle / {name} / {layout}"
    H.check_rules(batch, "closest", exp["closest"], alone["closest"], what)
    H.check_rules(batch, "first", exp["closest"][2], alone["closest"][2], what)
    H.check_rules(batch, "count", exp["count"], alone["count"], what)
    H.check_rules(batch, "any", exp["count"] > 0, alone["count"] > 0, what)
    H.check_rules(batch, "location", exp["location"], alone["location"], what)
    assert np.array_equal(exp["closest"][0], exp["count"] > 0)
    H.check_geometry(H.geometry_f64(name, layout), exp["closest"][0], exp["closest"][2], exp["closest"][3], what)
    if layout == "interleaved":                      # (the same rays in both layouts)
        brute = OracleIntersector(v, f, 0)
        for k, (a, b) in enumerate(zip(brute.closest_raw(batch.o, batch.d)[:5], exp["closest"])):
            assert H._same(a, b), f"{what}: closest output {k}, brute force against the BVH mode"
        assert np.array_equal(brute.intersects_count(batch.o, batch.d), exp["count"])
        for a, b in zip(brute.intersects_location(batch.o, batch.d), exp["location"]):
            assert H._same(a, b), f"{what}: location lists, brute force against the BVH mode"


def test_contains_points_rules_on_the_oracle():
    p, bad = hostile_points()
    want = oracle_contains(p)
    assert not want[bad].any() and 0.1 < want[~bad].mean() < 0.9
    assert np.array_equal(want[~bad], oracle_contains(p[~bad]))


# host simulation: (name, sim.use_fused mode, unordered schedule); the 32-bit state of mode 6 holds 32 levels: not the deep tree
# ... and 65 rays per finite family: a ray with a denormal reciprocal walks most of the grid nodes (the cost cliff),
# which the single-threaded simulation pays for four queries and the lists
SIM_PER = 65
SIM_MODES = (("generic", 0, False), ("fused 1", 1, False), ("fused 5", 5, False), ("fused 6", 6, False), ("unordered schedule", 0, True))


SIM_CASES = [(name, mode) for name in ALL_SCENES for mode in SIM_MODES if not (name == "deep" and mode[1] == 6)]


@pytest.mark.parametrize("name,mode", SIM_CASES, ids=[f"{name}-{mode[0]}" for name, mode in SIM_CASES])
def test_host_simulation_returns_the_oracles_bits_on_hostile_rays(name, mode):
    """the product headers, compiled for the host, on the interleaved batch: every output of every query is the oracle's,
    and the simulation's own outputs keep the rules (the miss rule, the ordinary rays as alone, the scaling identity, no
    non-finite float).  The simulation's lists hold (count, tri, t) per ray, no locations: these against the oracle's."""
    import sim
    from oracle.oracle import OracleIntersector
    from sim import SimBVH
    v, f, o, d = H.scene(name)[:4]
    batch, exp = H.expected(name, "interleaved", per=SIM_PER)
    sim.use_fused(mode[1])
    sim.use_unordered(mode[2])
    try:
        B = SimBVH(v, f)
        what = f"{mode[0]} / {name}"
        for query, q in (("closest", 2), ("count", 3), ("any", 0), ("first", 1)):
            got, alone = B.query(q, batch.o, batch.d), B.query(q, o, d)
            if query == "closest":
                got, alone = (tuple(r[k] for k in ("hit", "front", "tri", "loc", "uv")) for r in (got, alone))
                for key, g, e in zip(("hit", "front", "tri", "loc", "uv"), got, exp["closest"]):
                    assert H._same(g.reshape(e.shape), e), f"{what}: closest {key}"
            else:
                key = {"count": "count", "any": "hit", "first": "tri"}[query]
                got, alone = got[key], alone[key]
                e = {"count": exp["count"], "any": exp["count"] > 0, "first": exp["closest"][2]}[query]
                assert np.array_equal(got, e), f"{what}: {query}"
            H.check_rules(batch, query, got, alone, f"{what}, the simulation's own outputs")
        cnt, ltri, lt = B.location(batch.o, batch.d)
        keep = np.arange(8)[None, :] < np.minimum(cnt, 8)[:, None]
        _, _, tri_o, t_o = OracleIntersector(v, f, 1).intersects_location(batch.o, batch.d, with_t=True)
        assert np.array_equal(cnt, exp["count"]) and np.array_equal(ltri[keep], tri_o) and H._same(lt[keep], t_o), f"{what}: location"
        assert not cnt[batch.mask(*H.INVALID)].any() and np.isfinite(lt[keep]).all(), f"{what}: location"
    finally:
        sim.use_fused(0)
        sim.use_unordered(False)


@pytest.mark.parametrize("name", ALL_SCENES)
def test_fused_box_tests_contain_the_contracts_on_the_finite_families(name):
    """check_fused / check_fused_wide (the fused grid-node and 8-wide box tests against the contract's on the same boxes)
    on families 3 to 5: reciprocals beyond M = 1e30 and kmax, denormal reciprocals, origins at 2^60 ... 3.4e38 -- none of
    which tests/test_host_sim.py's _nasty_rays reaches"""
    from sim import SimBVH
    v, f = H.scene(name)[:2]
    batch, _ = H.expected(name, "interleaved")
    m = batch.mask("scale:", "comp:", "all:", "far:", "origin:")
    assert m.sum() >= 21 * 64
    B = SimBVH(v, f)
    stride = max(1, len(f) // 1500)
    bad, pairs, fused, contract = B.check_fused(batch.o[m], batch.d[m], node_stride=stride)
    assert pairs > 1_000_000 and bad == 0 and fused >= contract, (bad, pairs, fused, contract)
    badw, pairsw, fw, cw = B.check_fused_wide(batch.o[m], batch.d[m], node_stride=stride)
    assert pairsw > 300_000 and badw == 0 and fw >= cw, (badw, pairsw, fw, cw)
