"""Every traversal kernel flavour, every multi-hit cap and the scan / compaction edges against exact references.

test_flavour_matches_the_oracle crosses the five queries with the three addressing flavours of a query launch
(csrc/launch_policy.inc, `addr32` / `compact` / `deep` of launch_query: compact = 32-bit offsets and trail, deep = 32-bit
offsets and a 64-bit trail for hierarchies of more than 32 levels, generic = 64-bit, forced on small meshes by
compact = 0) and the launch shapes the live
options select.  A combination that launch_policy.inc cannot produce is skipped with the function (and variable) of that
file that rules it out.
Each case compares every output with the oracle bit for bit and, for a direct launch, checks that tr_bvh_last_launch
reports the (query, shape, node flavour, addressing, sort carried) the case claims.  Streaming launches leave no
record: their flavour follows from the options (stream = 2 always streams) and the hierarchy's depth, which the
test asserts, and the absence of a record shows that no direct launch ran instead.

The multi-hit tests run both protocols of the C ABI (count_topk -> hits_scan -> location_fill_slots and
count -> hits_scan -> location_fill) at caps from 1 to TR_MAX_HITS_CAP = 32 on rays with more hits than the cap and
with exact ties at the cap boundary.  The scan tests cover the three levels of scan_impl (tiles of 4096, one
workgroup over the partials in chunks of 1024)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import workloads as W
from launch_options import options
from oracle.oracle import OracleIntersector
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)

pytestmark = pytest.mark.gpu

QUERIES = ("any", "first", "closest", "count", "location")
QID = {q: k for k, q in enumerate(QUERIES)}
PRUNING = ("any", "first", "closest")
ADDRESSING = {"compact": 1, "deep": 2, "generic": 0}      # tr_launch_info.addressing
# addressing -> scenes: image-shaped rays on the bunny stand-in and on six nested shells (rays through the centre cross
# twelve surfaces: more than the 8 a list keeps), flat hash rays on a soup and on the deep tree (rays down the pile of
# 3000 identical triangles: 3000 exact ties)
SCENES_OF = {"compact": ("bunny", "shells", "soup"), "deep": ("deep",), "generic": ("shells", "soup", "deep")}


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(v, f, o, d, oracle results on the flattened rays)"""
    if name == "bunny":
        v, f = W.bunny_standin()
        o, d = W.pinhole_grid(320, 240, distance=2.8)
    elif name == "shells":
        v, f = W.nested_shells(4, radii=(1.0, 0.85, 0.7, 0.55, 0.4, 0.25))
        o, d = W.pinhole_grid(256, 208, distance=2.5)
    elif name == "soup":
        v, f = W.random_soup(20000, seed=5)
        o, d = W.hash_rays(120_000, 61, [-1.3] * 3, [1.3] * 3)
    else:
        v, f = W.deep_tree_mesh(3000)
        o, d = W.hash_rays(60_000, 62, [-0.2] * 3, [1.2] * 3)
        o[:1500] = [1e-10, 1e-10, 1.0]
        d[:1500] = [0.0, 0.0, -1.0]
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    R = OracleIntersector(v, f, 1)
    of, df = o.reshape(-1, 3), d.reshape(-1, 3)
    exp = {"closest": R.closest_raw(of, df)[:5], "count": R.intersects_count(of, df),
           "location": R.intersects_location(of, df)}
    return v, f, o, d, exp


def run_query(r, q, ot, dt):
    if q == "location":
        return r.intersects_location(ot, dt)
    return getattr(r, "intersects_" + q)(ot, dt)


def check_query(q, got, exp, what):
    if q == "closest":
        for name, g, e in zip(("hit", "front", "tri", "loc", "uv"), got, exp["closest"]):
            g = g.cpu().numpy().reshape(e.shape)
            assert np.array_equal(g, e), f"{what}: closest {name}, {int(np.sum(np.any((g != e).reshape(len(e), -1), 1)))} rays differ"
        return
    if q == "location":
        for name, g, e in zip(("loc", "ray", "tri"), got, exp["location"]):
            g = g.cpu().numpy()
            assert g.shape == e.shape and np.array_equal(g, e), f"{what}: location {name} ({g.shape} vs {e.shape})"
        return
    g = got.cpu().numpy().reshape(-1)
    e = {"first": exp["closest"][2], "count": exp["count"], "any": exp["count"] > 0}[q]
    assert np.array_equal(g, e), f"{what}: {q}, {int(np.sum(g != e))} rays differ"


# launch shape -> (options, applicable queries, addressing flavours, why the others do not exist)
SHAPES = {
    "plain": (dict(stream=0, steal=0, wide_direct=0), PRUNING, ("compact", "deep", "generic"),
              "launch_direct (unord): the plain shape, its last else, exists for the pruning queries only"),
    "steal_exact": (dict(stream=0, steal=2, grid_nodes=0, wide_direct=0), PRUNING, ("compact", "deep", "generic"),
                    "decide_direct_shape (steal): stealing exists for the pruning queries only"),
    "steal_grid": (dict(stream=0, steal=2, grid_nodes=1, sort_inline=0, wide_direct=0), PRUNING, ("compact", "deep"),
                   "launch_direct (qn_used): grid nodes in stealing launches of the pruning queries with 32-bit offsets only"),
    "sort_carried": (dict(stream=0, steal=2, grid_nodes=1, usteal=1, sort_inline=1, wide_direct=0), PRUNING + ("count",),
                     ("compact", "deep"),
                     "launch_direct (can_carry): the sort rides in stealing grid-node / stealing count launches with 32-bit offsets only"),
    "unord": (dict(stream=0, usteal=0, wide_direct=0), ("count", "location"), ("compact", "deep", "generic"),
                  "launch_direct (unord): the unordered schedule is the one of count and location"),
    "usteal": (dict(stream=0, usteal=1, sort_inline=0, wide_direct=0), ("count",), ("compact", "deep", "generic"),
               "decide_direct_shape (usteal): hand-over between lanes of the unordered schedule exists for count only"),
    "stream": (dict(stream=2, wide=0), PRUNING + ("count",), ("compact", "deep", "generic"),
               "decide_streaming: the location query has no streaming launch"),
    "stream_wide": (dict(stream=2, wide=1), PRUNING + ("count",), ("compact", "deep"),
                    "decide_streaming / launch_streaming (wn): no streaming location launch; 8-wide nodes with 32-bit offsets only"),
    "wide_direct": (dict(stream=0, wide_direct=3), QUERIES, ("compact", "deep"),
                    "decide_direct_shape (use_wd): the direct launch on 8-wide nodes exists with 32-bit offsets only"),
}
# tr_launch_info.shape of each direct shape: 0 plain, 1 stealing, 2 unordered, 3 unordered with hand-over, 4 8-wide
SHAPE_ID = {"plain": 0, "steal_exact": 1, "steal_grid": 1, "unord": 2, "usteal": 3, "wide_direct": 4}


def expect_launch(r, q, shape, addressing, what):
    li = r.as_wrapper.last_launch()
    want_shape = (3 if q == "count" else 1) if shape == "sort_carried" else SHAPE_ID[shape]
    # the grid-node flag: stealing pruning launches on grid nodes, and every unordered launch (count / location walk the
    # 32-byte nodes); never the 8-wide direct launch
    want_gn = 0 if shape in ("plain", "steal_exact", "wide_direct") else 1
    got = (li["query"], li["shape"], li["grid_nodes"], li["addressing"])
    assert got == (QID[q], want_shape, want_gn, ADDRESSING[addressing]), f"{what}: last launch {li}"
    return li


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("addressing", list(ADDRESSING))
@pytest.mark.parametrize("query", QUERIES)
def test_flavour_matches_the_oracle(device, query, addressing, shape):
    opts, queries, flavours, why = SHAPES[shape]
    if query not in queries or addressing not in flavours:
        pytest.skip(why)
    from triro.ray.ray_optix import RayMeshIntersector
    streaming = shape.startswith("stream")
    for name in SCENES_OF[addressing]:
        v, f, o, d, exp = scene(name)
        what = f"{query} / {addressing} / {shape} / {name}"
        with options(compact=0 if addressing == "generic" else 1, **opts):
            r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
            depth = r.bvh_info()["depth"]
            if addressing == "deep":
                assert depth > 32, (name, depth)
            elif addressing == "compact":
                assert depth <= 32, (name, depth)
            ot, dt = T(o, device), T(d, device)
            if shape == "sort_carried":
                # the deferred sort of the learned order rides in a later launch of the same batch shape: every launch
                # is compared until one has carried it
                carried = False
                for k in range(16):
                    check_query(query, run_query(r, query, ot, dt), exp, f"{what} launch {k}")
                    li = expect_launch(r, query, shape, addressing, f"{what} launch {k}")
                    if li["sort_carried"]:
                        carried = True
                        break
                assert carried, f"{what}: no launch of 16 carried the sort"
                continue
            for k in range(2):                    # the second launch runs on the learned order
                check_query(query, run_query(r, query, ot, dt), exp, f"{what} launch {k}")
                if streaming:
                    with pytest.raises(ValueError, match="no direct launch"):
                        r.as_wrapper.last_launch()
                else:
                    li = expect_launch(r, query, shape, addressing, f"{what} launch {k}")
                    assert li["sort_carried"] == 0, f"{what}: {li}"
            torch.cuda.synchronize()


# ---- multi-hit lists at every cap ----------------------------------------------------------------------------------
CAPS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32)


def _check(rc):
    import triro.backend.ops as hops
    hops._check(rc)


def multi_hit(r, ot, dt, cap, fused, ray_base=0, scan_cap=None):
    """one multi-hit protocol of the C ABI at `cap` -> (loc, ray, tri, count) on the host"""
    import triro.backend.ops as hops
    lib = hops.get_module()
    dev = ot.device
    n = ot.numel() // 3
    h = r.as_wrapper._inner
    rays = hops.make_rays(ot, dt)
    stream = torch.cuda.current_stream(dev).cuda_stream
    count = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if fused:
        slots = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)       # tr_hit_entry {t_key, slot}
        _check(lib.tr_intersects_count_topk(h, C.byref(rays), cap, count.data_ptr(), slots.data_ptr(), stream))
    else:
        _check(lib.tr_intersects_count(h, C.byref(rays), count.data_ptr(), stream))
    offsets = torch.empty(n, dtype=torch.int64, device=dev)
    total_d = torch.empty(1, dtype=torch.int64, device=dev)
    total = C.c_int64(-1)
    _check(lib.tr_hits_scan(count.data_ptr(), n, cap if scan_cap is None else scan_cap, offsets.data_ptr(),
                            total_d.data_ptr(), C.byref(total), stream))
    nh = int(total.value)
    assert nh == int(total_d.item())
    loc = torch.full((nh, 3), 7.0, dtype=torch.float32, device=dev)
    ray = torch.full((nh,), -7, dtype=torch.int32, device=dev)
    tri = torch.full((nh,), -7, dtype=torch.int32, device=dev)
    if fused:
        _check(lib.tr_location_fill_slots(h, C.byref(rays), cap, count.data_ptr(), offsets.data_ptr(), slots.data_ptr(),
                                          loc.data_ptr(), ray.data_ptr(), tri.data_ptr(), ray_base, stream))
    else:
        _check(lib.tr_intersects_location_fill(h, C.byref(rays), cap, offsets.data_ptr(), loc.data_ptr(), ray.data_ptr(),
                                               tri.data_ptr(), ray_base, stream))
    torch.cuda.synchronize()
    return loc.cpu().numpy(), ray.cpu().numpy(), tri.cpu().numpy(), count.cpu().numpy()


def tie_scene():
    """Three stacked integer-grid height fields (every triangle ten times: ten exact ties per crossing, at face indices
    F apart) under lattice rays through vertices, edges and cell diagonals: 30 crossings per vertical ray, each tie
    group straddling the caps 7..9, 15..17, 31"""
    gn = 20
    g = np.arange(gn, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    vs, fs = [], []
    for L in range(3):
        Z = ((X * (L + 2) + Y * (2 * L + 1)) % 3).astype(np.float32) * np.float32(0.25) + np.float32(3 * L)
        idx = np.arange(gn * gn).reshape(gn, gn) + L * gn * gn
        qa, qb, qc, qd = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
        vs.append(np.stack([X, Y, Z], -1).reshape(-1, 3))
        fs.append(np.concatenate([np.stack([qa, qb, qc], 1), np.stack([qa, qc, qd], 1)]))
    v, f = np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)
    f = np.concatenate([f] * 10)
    h = np.arange(-0.5, gn - 0.5 + 1e-3, 0.25, dtype=np.float32)
    gx, gy = np.meshgrid(h, h, indexing="ij")
    dirs = np.array([[0, 0, -1], [1, 1, -2], [2, 1, -4], [1, -1, -1]], np.float32)
    o = np.repeat(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 12.0, np.float32)], -1), len(dirs), 0)
    d = np.tile(dirs, (gx.size, 1))
    return v, f, o.astype(np.float32), d.astype(np.float32)


def many_surfaces_scene():
    """21 nested shells: rays through the centre cross 42 surfaces"""
    v, f = W.nested_shells(3, radii=tuple(1.0 - 0.045 * k for k in range(21)))
    o, d = W.pinhole_grid(192, 160, distance=2.5)
    return v, f, np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))


@pytest.mark.parametrize("which", ["shells42", "ties"])
def test_multi_hit_lists_match_the_oracle_at_every_cap(device, which):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d = many_surfaces_scene() if which == "shells42" else tie_scene()
    R = OracleIntersector(v, f, 1)
    cnt = R.intersects_count(o, d)
    assert cnt.max() >= (40 if which == "shells42" else 30)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    ot, dt = T(o, device), T(d, device)
    with options(stream=0, wide_direct=0):
        for cap in CAPS:
            el, er, et = R.intersects_location(o, d, cap=cap)
            assert len(er) == int(np.minimum(cnt, cap).sum())
            for fused in (True, False):
                loc, ray, tri, count = multi_hit(r, ot, dt, cap, fused)
                what = f"{which} cap {cap} {'fused' if fused else 'two-pass'}"
                assert np.array_equal(count, cnt), f"{what}: counts"
                assert len(ray) == len(er), f"{what}: {len(ray)} rows, the oracle {len(er)}"
                assert np.array_equal(ray, er), f"{what}: ray_idx"
                assert np.array_equal(tri, et), f"{what}: tri_idx, {int(np.sum(tri != et))} rows differ"
                assert np.array_equal(loc, el), f"{what}: loc"


def test_multi_hit_cap_range_and_ray_base(device):
    """cap 0 and 33 are refused where the C ABI says so; location_fill at cap 0 writes nothing; ray_base is added to
    every ray index; a scan cap above the fill cap leaves the fill's rows where the scan put them"""
    import triro.backend.ops as hops
    from triro.ray.ray_optix import RayMeshIntersector
    v, f, o, d = many_surfaces_scene()
    o, d = np.ascontiguousarray(o[::7][:4096]), np.ascontiguousarray(d[::7][:4096])      # (rows through the centre: 42 hits)
    R = OracleIntersector(v, f, 1)
    r = RayMeshIntersector(vertices=T(v, device), faces=T(f, device))
    ot, dt = T(o, device), T(d, device)
    lib = hops.get_module()
    h = r.as_wrapper._inner
    rays = hops.make_rays(ot, dt)
    n = len(o)
    s = torch.cuda.current_stream(device).cuda_stream
    count = torch.empty(n, dtype=torch.int32, device=device)
    slots = torch.zeros((n, 33, 2), dtype=torch.int32, device=device)
    offsets = torch.zeros(n, dtype=torch.int64, device=device)
    out = [torch.full((n * 33, 3), 7.0, device=device), torch.full((n * 33,), -7, dtype=torch.int32, device=device),
           torch.full((n * 33,), -7, dtype=torch.int32, device=device)]
    ptrs = [x.data_ptr() for x in out]
    for cap in (0, 33):
        assert lib.tr_intersects_count_topk(h, C.byref(rays), cap, count.data_ptr(), slots.data_ptr(), s) == 1
        assert lib.tr_location_fill_slots(h, C.byref(rays), cap, count.data_ptr(), offsets.data_ptr(), slots.data_ptr(),
                                          *ptrs, 0, s) == 1
    assert lib.tr_intersects_location_fill(h, C.byref(rays), 33, offsets.data_ptr(), *ptrs, 0, s) == 1
    total = C.c_int64(0)
    assert lib.tr_hits_scan(count.data_ptr(), n, -1, offsets.data_ptr(), offsets.data_ptr(), C.byref(total), s) == 1
    # cap 0: accepted by the two-pass fill, nothing written
    assert lib.tr_intersects_location_fill(h, C.byref(rays), 0, offsets.data_ptr(), *ptrs, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == 7.0).all()) and bool((out[1] == -7).all()) and bool((out[2] == -7).all())
    # ray_base is added to every ray index, in both protocols
    for cap in (1, 8, 32):
        el, er, et = R.intersects_location(o, d, cap=cap)
        for fused in (True, False):
            loc, ray, tri, _ = multi_hit(r, ot, dt, cap, fused, ray_base=123_456_789)
            assert np.array_equal(ray, er + 123_456_789) and np.array_equal(tri, et) and np.array_equal(loc, el), (cap, fused)
    # the scan clamps at ITS cap: scanned at 32, filled at 8, every ray's rows start at its offset and the rest stay untouched
    loc, ray, tri, cnt = multi_hit(r, ot, dt, 8, False, scan_cap=32)
    offs = np.concatenate([[0], np.cumsum(np.minimum(cnt, 32))[:-1]])
    el, er, et = R.intersects_location(o, d, cap=8)
    m = np.concatenate([offs[i] + np.arange(min(cnt[i], 8)) for i in range(n)]).astype(np.int64)
    assert np.array_equal(ray[m], er) and np.array_equal(tri[m], et) and np.array_equal(loc[m], el)
    rest = np.ones(len(ray), bool)
    rest[m] = False
    assert rest.any() and (ray[rest] == -7).all() and (tri[rest] == -7).all()


# ---- scans and compaction -------------------------------------------------------------------------------------------
SCAN_SIZES = (1, 4095, 4096, 4097, 1024 * 4096 - 1, 1024 * 4096 + 1, 5_000_011)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scans_match_an_int64_cumsum(device, n):
    """tr_hits_scan (counts clamped at the cap) and tr_mask_scan against numpy.cumsum in int64, at the tile edge (4096),
    at the edge of the partials loop's second chunk (1024 tiles) and beyond; the total on the device with and without
    the host copy"""
    import triro.backend.ops as hops
    lib = hops.get_module()
    rng = np.random.default_rng(n)
    cnt = rng.integers(0, 41, n).astype(np.int32)
    cnt[rng.random(n) < 0.4] = 0
    cnt[-1] = 40
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    s = torch.cuda.current_stream(device).cuda_stream
    ct, mt = T(cnt, device), T(mask, device)
    for cap in ((0, 1, 8, 32) if n in (1, 4097) else (8,)):
        want = np.cumsum(np.minimum(cnt, cap).astype(np.int64))
        for with_host in (True, False):
            off = torch.full((n,), -1, dtype=torch.int64, device=device)
            tot = torch.full((1,), -1, dtype=torch.int64, device=device)
            h = C.c_int64(-1)
            _check(lib.tr_hits_scan(ct.data_ptr(), n, cap, off.data_ptr(), tot.data_ptr(), C.byref(h) if with_host else None, s))
            torch.cuda.synchronize()
            got = off.cpu().numpy()
            assert got[0] == 0 and np.array_equal(got[1:], want[:-1]), (cap, with_host, int(np.argmax(got[1:] != want[:-1])))
            assert int(tot.item()) == int(want[-1]), (cap, with_host)
            assert int(h.value) == (int(want[-1]) if with_host else -1)
    want = np.cumsum(mask.astype(np.int64))
    for with_host in (True, False):
        off = torch.full((n,), -1, dtype=torch.int64, device=device)
        tot = torch.full((1,), -1, dtype=torch.int64, device=device)
        h = C.c_int64(-1)
        _check(lib.tr_mask_scan(mt.data_ptr(), n, off.data_ptr(), tot.data_ptr(), C.byref(h) if with_host else None, s))
        torch.cuda.synchronize()
        got = off.cpu().numpy()
        assert got[0] == 0 and np.array_equal(got[1:], want[:-1]), with_host
        assert int(tot.item()) == int(want[-1]) and int(h.value) == (int(want[-1]) if with_host else -1)


@pytest.mark.parametrize("n", [1, 4097, 300_001])
def test_compact_closest_with_a_ray_base(device, n):
    """tr_mask_scan + tr_compact_closest (hops.compact_closest) == boolean-mask gathers, ray indices offset by ray_base"""
    import triro.backend.ops as hops
    rng = np.random.default_rng(7 + n)
    hit = rng.random(n) < 0.6
    hit[0] = True
    front = rng.random(n) < 0.5
    tri = rng.integers(-1, 1 << 20, n).astype(np.int32)
    loc = rng.standard_normal((n, 3)).astype(np.float32)
    uv = rng.random((n, 2)).astype(np.float32)
    base = 1_000_003
    got = hops.compact_closest(*(T(x, device) for x in (hit, front, tri, loc, uv)), ray_base=base)
    fo, ro, to, lo, uo = [x.cpu().numpy() for x in got]
    assert np.array_equal(ro, np.flatnonzero(hit).astype(np.int32) + base)
    assert np.array_equal(fo, front[hit]) and np.array_equal(to, tri[hit])
    assert np.array_equal(lo, loc[hit]) and np.array_equal(uo, uv[hit])
    # outputs left out are not written, the ray indices still are
    _, ro2, to2, lo2, _ = hops.compact_closest(T(hit, device), None, T(tri, device), None, None, ray_base=base)
    assert np.array_equal(ro2.cpu().numpy(), ro) and np.array_equal(to2.cpu().numpy(), to) and lo2 is None
