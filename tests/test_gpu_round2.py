"""GPU tests added in round 2 (VERDICT r01 "Next round" items 1, 7, 8 and ADVICE r01):

* the work-stealing merge with rays that start exactly on the mesh (t_key = -0.0 / +0.0 ties),
  forced steal thresholds, against the BRUTE-FORCE oracle;
* C-ABI hardening: face indices outside [0, nv) are reported, not dereferenced; queries refuse
  rays on another device; save/load after a shrinking update_raw; a failed build leaves an
  empty (not a dangling) handle; options may change while other threads query;
* every launch shape reachable through tr_set_option (the streaming launch on binary and 8-wide
  nodes, the direct launch on 8-wide nodes; the unordered two-phase schedule with and without
  hand-over between lanes, and its vote threshold) against the oracle.
"""
import threading

import numpy as np
import pytest
import torch

import workloads as W
from launch_options import options, restore_defaults
from oracle.oracle import OracleIntersector
import poison
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)

pytestmark = pytest.mark.gpu


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def make(v, f, dev):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, dev), faces=T(f, dev))


def assert_closest_bitexact(got, exp, what=""):
    hit, front, tri, loc, uv = [g.cpu().numpy() for g in got]
    eh, ef, et, el, eu = exp[:5]
    assert np.array_equal(hit, eh), f"{what}: hit mask, {np.sum(hit != eh)} rays differ"
    assert np.array_equal(tri, et), f"{what}: tri_idx, {np.sum(tri != et)} rays differ"
    assert np.array_equal(front, ef), f"{what}: front"
    assert np.array_equal(loc, el) and np.array_equal(uv, eu), f"{what}: loc/uv bits"


def on_surface_rays(v, f, r, dev, n_each=2500, seed=0):
    """Origins exactly at mesh vertices, at edge midpoints and at `loc` values returned by a first
    trace (secondary rays); directions +-normal, +-vertex direction, towards other vertices and
    random.  Rays that start in the plane of a triangle give t_key = +-0.0."""
    rng = np.random.default_rng(seed)
    nv, nf = len(v), len(f)
    vi = rng.integers(0, nv, n_each)
    fi = rng.integers(0, nf, n_each)
    tri = v[f[fi]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float32)
    mid = (np.float32(0.5) * tri[:, 0] + np.float32(0.5) * tri[:, 1]).astype(np.float32)
    # secondary rays from the hit points of a camera trace
    o1, d1 = W.pinhole_grid(96, 96, distance=2.5 * float(np.abs(v).max()))
    hit, _, _, loc, _ = r.intersects_closest(T(o1, dev), T(d1, dev))
    sec = loc[hit].cpu().numpy()
    sec = sec[rng.integers(0, len(sec), n_each)] if len(sec) else v[vi]
    vdir = v[vi] / np.maximum(np.linalg.norm(v[vi], axis=1, keepdims=True), 1e-20)
    origins = [v[vi], v[vi], v[vi], v[vi], mid, mid, mid, sec, sec, v[f[fi, 0]], v[f[fi, 1]]]
    dirs = [vdir, -vdir, v[rng.integers(0, nv, n_each)] - v[vi], rng.normal(size=(n_each, 3)),
            nrm, -nrm, rng.normal(size=(n_each, 3)), rng.normal(size=(n_each, 3)),
            -sec, nrm, -nrm]
    o = np.concatenate(origins).astype(np.float32)
    d = np.concatenate(dirs).astype(np.float32)
    return o, d


@pytest.mark.parametrize("threshold", [2, 8])
@pytest.mark.parametrize("mesh", ["shells4", "bunny"])
def test_steal_merge_with_rays_starting_on_the_mesh(device, threshold, mesh):
    """the 64-bit LDS-min key of the stealing merge ordered t_key = -0.0
    (bits 0x80000000) above every positive distance.  Closest + first vs the brute-force oracle
    with stealing forced from trip 2 / 8 on, origins exactly on vertices / edges / hit points."""
    import triro.backend.ops as hops
    v, f = W.nested_shells(4) if mesh == "shells4" else W.bunny_standin()
    r = make(v, f, device)
    o, d = on_surface_rays(v, f, r, device)
    R = OracleIntersector(v, f, 0)                       # brute force
    exp = R.closest_raw(o, d)
    # the case must really contain the dangerous keys: zero-distance hits with farther hits behind
    zero_t = exp[0] & (exp[5] == 0)
    assert zero_t.sum() > 500, "test input lost its bite"
    assert (R.intersects_count(o, d)[zero_t] > 1).sum() > 300
    ot, dt = T(o, device), T(d, device)
    try:
        for steal in (threshold, 0, 1):
            hops.set_option("steal", steal)
            for _ in range(2):
                assert_closest_bitexact(r.intersects_closest(ot, dt), exp, f"steal={steal}")
            assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy(), exp[2]), f"first steal={steal}"
    finally:
        hops.set_option("steal", 1)


@pytest.mark.parametrize("split,split_steal", [(1, 8), (2, 0), (3, 2), (4, 64)])
def test_split_blocks_of_the_learned_order_match_the_oracle(device, split, split_steal):
    """Block splitting (k_sched_sort): from the second launch of a batch on the most expensive blocks
    run as two / four launch slots of half / quarter density whose idle lanes steal from the first
    trips on.  Image-shaped (8x8 tiles) and flat batches, the stealing queries (closest, first, any;
    count with stealing forced), several launches each (learn -> split -> re-measure), interleaved
    with count / location launches of the same batch, which keep their own order."""
    import triro.backend.ops as hops
    v, f = W.icosphere(5)
    v = W.displaced(v, seed=3, amplitude=0.05)
    r = make(v, f, device)
    R = OracleIntersector(v, f, 1)
    o_img, d_img = W.pinhole_grid(384, 256, distance=2.5)            # 98 304 rays = 768 blocks
    o_on, d_on = on_surface_rays(v, f, r, device, n_each=1500, seed=5)   # +-0.0 keys through split waves
    cases = [("image", o_img, d_img), ("flat", o_img.reshape(-1, 3), d_img.reshape(-1, 3)), ("on-surface", o_on, d_on)]
    try:
        hops.set_option("split", split)
        hops.set_option("split_steal", split_steal)
        for name, o, d in cases:
            exp = R.closest_raw(o.reshape(-1, 3), d.reshape(-1, 3))
            cnt = R.intersects_count(o.reshape(-1, 3), d.reshape(-1, 3))
            ot, dt = T(o, device), T(d, device)
            for rep in range(6):
                got = [g.reshape((-1,) + tuple(g.shape[o.ndim - 1:])) for g in r.intersects_closest(ot, dt)]
                assert_closest_bitexact(got, exp, f"{name} split={split} launch {rep}")
                assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy().reshape(-1), exp[2])
                assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy().reshape(-1), cnt > 0)
                assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy().reshape(-1), cnt)
                if rep >= 2 and name in ("image", "flat") and split > 0:
                    # a flat batch with split slots never left the plain launch shape (no order, no split);
                    # from the third launch on every stealing batch shape runs with its learned, split order
                    r.intersects_closest(ot, dt)
                    li = r.as_wrapper.last_launch()
                    assert li["learned_order"] == 1 and li["split_blocks"] > 0, (name, rep, li)
            hops.set_option("steal", 16)        # count through the stealing shape, split as well
            for rep in range(3):
                assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy().reshape(-1), cnt)
                assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy().reshape(-1), exp[2])
            hops.set_option("steal", 1)
    finally:
        for k, val in (("split", 1), ("split_steal", 8), ("steal", 1)):
            hops.set_option(k, val)


def test_bad_face_indices_are_reported_not_dereferenced(device):
    """VERDICT r01 weak #8 / ADVICE: out-of-range vertex indices -> ValueError naming the first
    bad face (the reference hands the index buffer to optixAccelBuild unchecked, ray.cpp:44-58)."""
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(3)
    o, d = W.readme_perspective(32)
    ot, dt = T(o, device), T(d, device)
    for bad_value in (len(v), -1, 2**31 - 1, -2**31):
        f2 = f.copy()
        f2[777, 1] = bad_value
        f2[900, 0] = bad_value
        with pytest.raises(ValueError, match="face 777"):
            RayMeshIntersector(vertices=T(v, device), faces=T(f2, device))
    # nv == 0 with faces: every face is bad
    with pytest.raises(ValueError, match="face 0"):
        RayMeshIntersector(vertices=torch.zeros((0, 3), device=device), faces=T(f[:4], device))
    # a failed update_raw leaves an EMPTY handle behind (misses), never a half-built tree
    r = make(v, f, device)
    ref = r.intersects_first(ot, dt)
    assert (ref >= 0).any()
    f2 = f.copy()
    f2[5, 2] = len(v) + 3
    with pytest.raises(ValueError, match="face 5"):
        r.update_raw(T(v, device), T(f2, device))
    assert r.bvh_info()["num_tris"] == 0
    assert not r.intersects_any(ot, dt).any() and int(r.intersects_count(ot, dt).sum()) == 0
    r.update_raw(T(v, device), T(f, device))                 # and the handle is still usable
    assert torch.equal(r.intersects_first(ot, dt), ref)
    # refit with a bad index
    with pytest.raises(ValueError, match="face 5"):
        r.as_wrapper.refit(T(v, device), T(f2, device))
    assert r.bvh_info()["num_tris"] == 0
    r.update_raw(T(v, device), T(f, device))
    assert torch.equal(r.intersects_first(ot, dt), ref)
    # single-triangle mesh goes through the same check
    with pytest.raises(ValueError, match="face 0"):
        RayMeshIntersector(vertices=T(v[:3], device), faces=T(np.array([[0, 1, 3]], np.int32), device))


def test_rays_on_another_device_are_refused(device):
    v, f = W.icosphere(2)
    r = make(v, f, device)
    o, d = W.readme_perspective(16)
    ot, dt = T(o, device), T(d, device)
    assert r.as_wrapper.device_index == device.index == r.bvh_info()["device"]
    r.as_wrapper.device_index = device.index + 1      # pretend the arena lives elsewhere
    try:
        for q in (r.intersects_any, r.intersects_first, r.intersects_closest, r.intersects_count,
                  r.intersects_location):
            with pytest.raises(ValueError, match="acceleration structure lives on"):
                q(ot, dt)
    finally:
        r.as_wrapper.device_index = device.index
    assert r.intersects_any(ot, dt).any()


def test_save_load_after_shrinking_update_raw(device, tmp_path):
    """the arena keeps its larger capacity after update_raw to a smaller
    mesh; the blob must hold only the bytes the current mesh uses and load() must accept it."""
    from triro.ray.ray_optix import RayMeshIntersector
    big_v, big_f = W.icosphere(5)
    v, f = W.icosphere(3)
    r = make(big_v, big_f, device)
    cap = r.bvh_info()["arena_bytes"]
    r.update_raw(T(v, device), T(f, device))
    assert r.bvh_info()["arena_bytes"] == cap                      # capacity kept
    blob = r.as_wrapper.serialize()
    fresh = make(v, f, device)
    assert blob.nbytes == fresh.as_wrapper.serialize().nbytes < cap
    path = str(tmp_path / "shrunk.npz")
    r.save(path)
    r2 = RayMeshIntersector.load(path, device=device)
    o, d = W.pinhole_grid(128, 96)
    ot, dt = T(o, device), T(d, device)
    R = OracleIntersector(v, f, 1)
    exp = R.closest_raw(o, d)
    assert_closest_bitexact(r2.intersects_closest(ot, dt), exp, "loaded")
    assert_closest_bitexact(r.intersects_closest(ot, dt), exp, "shrunk original")
    for a, b in zip(r2.as_wrapper.download(), fresh.as_wrapper.download()):
        assert np.array_equal(a, b)
    for a, b in zip(r2.as_wrapper.download_qnodes(), fresh.as_wrapper.download_qnodes()):
        assert np.array_equal(a, b)


def test_options_may_change_while_other_threads_query(device):
    """tr_set_option stores relaxed atomics and every launch works from one snapshot: flipping
    knobs from another thread never changes results."""
    import triro.backend.ops as hops
    v, f = W.bunny_standin()
    r = make(v, f, device)
    o, d = W.pinhole_grid(256, 256, distance=2.5 * 1.12)
    ot, dt = T(o, device), T(d, device)
    ref = [x.clone() for x in r.intersects_closest(ot, dt)]
    stop = threading.Event()

    def flipper():
        k = 0
        while not stop.is_set():
            k += 1
            hops.set_option("steal", (0, 1, 2, 8)[k % 4])
            hops.set_option("adaptive", k & 1)
            hops.set_option("grid_nodes", (0, 1, 2)[k % 3])
            hops.set_option("xcd_chunk", (0, 16, 128)[k % 3])
            hops.set_option("tile", k % 3)

    th = threading.Thread(target=flipper)
    th.start()
    try:
        for _ in range(40):
            got = r.intersects_closest(ot, dt)
            for a, b in zip(got, ref):
                assert torch.equal(a, b)
    finally:
        stop.set()
        th.join()
        restore_defaults()
    with pytest.raises(ValueError):
        hops.set_option("stream_rays", 7)           # out of range
    for retired, value in (("block_size", 100), ("lds_top", 2)):     # retired in round 5: accepted and ignored, like every retired name
        hops.set_option(retired, value)
    with pytest.raises(ValueError):
        hops.set_option("no_such_option", 1)


SHAPES = [
    dict(stream=2, wide=0),
    dict(stream=2, wide=1),
    dict(stream=0, wide_direct=3),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_optional_launch_shapes_match_the_oracle(device, shape):
    """every kernel reachable through tr_set_option is compared with the
    oracle (not with another GPU launch): the streaming launch forced on binary and on 8-wide nodes, and the direct
    launch on 8-wide nodes for every query, on coherent and incoherent batches.  (The per-lane refill
    kernel of round 1 was deleted: the randomised sweep found a mismatch in it and it was 4x
    slower than the direct launch.)"""
    cases = [
        (W.bunny_standin(), W.hash_rays(600_000, 31, [-1.6] * 3, [1.6] * 3)),
        (W.nested_shells(4), tuple(x.reshape(-1, 3) for x in W.pinhole_grid(800, 768))),
        (W.deep_tree_mesh(3000), W.hash_rays(530_000, 32, [-0.2] * 3, [1.2] * 3)),
    ]
    with options(**shape):
        for (v, f), (o, d) in cases:
            r = make(v, f, device)
            R = OracleIntersector(v, f, 1)
            ot, dt = T(o, device), T(d, device)
            exp = R.closest_raw(o, d)
            cnt = R.intersects_count(o, d)
            for _ in range(2):
                assert_closest_bitexact(r.intersects_closest(ot, dt), exp, str(shape))
            assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy(), exp[2])
            assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), cnt)
            assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy(), cnt > 0)


@pytest.mark.parametrize("usteal,leaf_vote", [(0, 16), (1, 1), (1, 16), (1, 64), (2, 8), (2, 64)])
def test_unordered_schedule_matches_the_oracle(device, usteal, leaf_vote):
    """count / location / any through the unordered two-phase schedule (leaves queued in LDS, tested
    in wave-voted leaf phases) -- count without (usteal = 0) and with hand-over between lanes (1: from the
    policy's trip, 2: forced from the second trip) --, every vote threshold from "always" to "only when forced", against
    the oracle: multi-layer scene with > 8 hits per ray (list replacement), incoherent rays on a
    soup, the deep tree (64-bit trail), image-shaped batches (8x8 tiles) and flat ones."""
    import triro.backend.ops as hops
    cases = [
        (W.nested_shells(4, radii=(1.0, 0.8, 0.6, 0.4, 0.3)), W.pinhole_grid(256, 192)),
        (W.random_soup(6000, seed=13), W.hash_rays(150_000, 41, [-1.3] * 3, [1.3] * 3)),
        (W.deep_tree_mesh(3000), W.hash_rays(40_000, 42, [-0.2] * 3, [1.2] * 3)),
        (W.bunny_standin(), tuple(x.reshape(-1, 3) for x in W.pinhole_grid(320, 200))),
    ]
    with options(usteal=usteal, leaf_vote=leaf_vote):
        for (v, f), (o, d) in cases:
            r = make(v, f, device)
            R = OracleIntersector(v, f, 1)
            ot, dt = T(o, device), T(d, device)
            cnt = R.intersects_count(o, d)
            for _ in range(2):
                assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), cnt)
            assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy(), cnt > 0)
            loc, ray, tri = [x.cpu().numpy() for x in r.intersects_location(ot, dt)]
            el, er, et = R.intersects_location(o, d)
            assert np.array_equal(ray, er) and np.array_equal(tri, et) and np.array_equal(loc, el)


@pytest.mark.parametrize("rays_per_wave,refill,dynamic", [(64, 1, 1), (100, 16, 1), (256, 32, 1), (512, 16, 0), (512, 64, 1),
                                                          (4096, 32, 0), (64, 40, 0), (4096, 8, 1)])
def test_streaming_launch_with_ray_refill_matches_the_oracle(device, rays_per_wave, refill, dynamic):
    """The streaming launch (a wave takes ranges of rays -- from a work counter, or one static range --
    and refills its idle lanes from them)
    forced on at sizes and shapes where the automatic policy would not use it: closest / first /
    any / count against the oracle on incoherent and coherent rays, ragged tails (n not a
    multiple of the range), strided and broadcast inputs, a single-triangle mesh, invalid rays."""
    import triro.backend.ops as hops
    cases = [
        (W.bunny_standin(), W.hash_rays(200_001, 51, [-1.6] * 3, [1.6] * 3)),
        (W.random_soup(5000, seed=17), W.hash_rays(77_777, 52, [-1.3] * 3, [1.3] * 3)),
        (W.deep_tree_mesh(3000), W.hash_rays(30_000, 53, [-0.2] * 3, [1.2] * 3)),
        (W.nested_shells(4), W.pinhole_grid(200, 136)),
    ]
    try:
        hops.set_option("stream", 2)
        hops.set_option("stream_rays", rays_per_wave)
        hops.set_option("stream_refill", refill)
        hops.set_option("stream_dynamic", dynamic)
        for (v, f), (o, d) in cases:
            r = make(v, f, device)
            R = OracleIntersector(v, f, 1)
            ot, dt = T(o, device), T(d, device)
            exp = R.closest_raw(o, d)
            cnt = R.intersects_count(o, d)
            for _ in range(2):
                assert_closest_bitexact(r.intersects_closest(ot, dt), exp, "stream")
            assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy(), exp[2])
            assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), cnt)
            assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy(), cnt > 0)
        # strided directions + broadcast origin + NaN rays + a single triangle
        v, f = W.icosphere(4)
        r = make(v, f, device)
        R = OracleIntersector(v, f, 1)
        rng = np.random.default_rng(5)
        base = (rng.random((3000, 6)).astype(np.float32) * 2 - 1)
        base[::97, 1] = np.nan
        d_t = T(base, device)[:, ::2]
        o_t = torch.tensor([0.1, 0.2, 2.5], device=device).expand(3000, 3)
        exp = R.closest_raw(np.broadcast_to(np.array([0.1, 0.2, 2.5], np.float32), (3000, 3)), base[:, ::2])
        assert_closest_bitexact(r.intersects_closest(o_t, d_t), exp, "stream strided")
        r1 = make(v[f[0]], np.array([[0, 1, 2]], np.int32), device)
        R1 = OracleIntersector(v[f[0]], np.array([[0, 1, 2]], np.int32), 0)
        o1, d1 = W.hash_rays(5000, 54, [-1.5] * 3, [1.5] * 3)
        d1 = (v[f[0]].mean(0) - o1 + rng.normal(0, 0.02, o1.shape)).astype(np.float32)
        assert_closest_bitexact(r1.intersects_closest(T(o1, device), T(d1, device)), R1.closest_raw(o1, d1), "one triangle")
    finally:
        hops.set_option("stream", 1)
        hops.set_option("stream_rays", 256)
        hops.set_option("stream_refill", 0)
        hops.set_option("stream_dynamic", 1)


def test_large_flat_batches_probe_and_both_launch_shapes(device):
    """Flat batches of >= 2 M rays are enqueued in both launch shapes behind the coherence probe
    (k_probe_coherence).  Whatever it selects -- direct for a flattened image, streaming for hash
    rays -- and whatever is forced, the answers are the oracle's."""
    import triro.backend.ops as hops
    v, f = W.bunny_standin()
    r = make(v, f, device)
    R = OracleIntersector(v, f, 1)
    o1, d1 = W.pinhole_grid(1536, 1408, distance=2.5 * 1.12)
    o1, d1 = np.ascontiguousarray(o1).reshape(-1, 3), d1.reshape(-1, 3)          # coherent, flat, 2.16 M rays
    o2, d2 = W.hash_rays(2_200_001, 61, v.min(0) * 1.5, v.max(0) * 1.5)           # incoherent
    o3, d3 = W.hash_rays(2_228_224, 62, v.min(0) * 1.5, v.max(0) * 1.5)           # incoherent but "image-shaped"
    o3, d3 = o3.reshape(17, 131072, 3), d3.reshape(17, 131072, 3)
    o4, d4 = W.pinhole_grid(1536, 1408, distance=2.5 * 1.12)                     # a real image (tiles)
    try:
        for o, d in ((o1, d1), (o2, d2), (o3, d3), (np.ascontiguousarray(o4), d4)):
            ot, dt = T(o, device), T(d, device)
            exp = R.closest_raw(o, d)
            cnt = R.intersects_count(o, d)
            for stream in (1, 0, 2):
                hops.set_option("stream", stream)
                assert_closest_bitexact(r.intersects_closest(ot, dt), exp, f"stream={stream}")
                assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy(), cnt > 0)
                assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), cnt)
            hops.set_option("stream", 1)
            st = hops.trace_stats(r.as_wrapper, ot, dt, "closest")              # the instrumented launch takes the same path
            assert st["rays"] == o.size // 3 and st["node_visits"] > 0
    finally:
        hops.set_option("stream", 1)


def test_queries_can_be_captured_in_a_hip_graph(device):
    """The query entry points allocate nothing and never synchronise once the per-(handle, stream)
    scheduling buffers exist, so a warmed-up call can be captured with torch.cuda.graph and replayed
    (HIP graph): same results as the eager call, also after the rays in the captured buffers change."""
    v, f = W.bunny_standin()
    r = make(v, f, device)
    o, d = W.pinhole_grid(256, 256, distance=2.5 * 1.12)
    ot, dt = T(o, device), T(d, device)
    R = OracleIntersector(v, f, 1)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(3):                       # warm-up on the capture stream: creates its hint buffers
            r.intersects_closest(ot, dt)
            r.intersects_count(ot, dt)
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = r.intersects_closest(ot, dt)
        cnt = r.intersects_count(ot, dt)
    for k in range(3):
        ot.copy_(T(o, device) + 0.01 * k)        # new rays in the captured input buffers
        g.replay()
        torch.cuda.synchronize()
        poison.assert_written(*out, cnt, what=f"graph replay {k}")      # (the captured fill re-poisons before every replay)
        exp = R.closest_raw((o + np.float32(0.01 * k)).astype(np.float32), d)
        assert_closest_bitexact(out, exp, f"graph replay {k}")
        assert np.array_equal(cnt.cpu().numpy(), R.intersects_count((o + np.float32(0.01 * k)).astype(np.float32), d))
    # The learned launch order is per (handle, stream) and rewritten by every measuring launch: launches
    # of ANOTHER batch size on the capture stream, between replays, leave an order written for another
    # grid behind (and a replay leaves its own for them).  The kernels check the stamp of the order and
    # fall back to the static launch order -- results never depend on it.
    o2, d2 = W.pinhole_grid(384, 320, distance=2.5 * 1.12)
    o2t, d2t = T(o2, device), T(d2, device)
    exp2 = R.closest_raw(o2, d2)
    cnt2 = R.intersects_count(o2, d2)
    ot.copy_(T(o, device))
    exp = R.closest_raw(o, d)
    for k in range(4):
        with torch.cuda.stream(side):
            for _ in range(1 + k % 2):
                got2 = r.intersects_closest(o2t, d2t)
                c2 = r.intersects_count(o2t, d2t)
        side.synchronize()
        assert_closest_bitexact(got2, exp2, f"eager launch of another size after replay {k}")
        assert np.array_equal(c2.cpu().numpy(), cnt2)
        g.replay()
        torch.cuda.synchronize()
        poison.assert_written(*out, cnt, what=f"graph replay after another batch size {k}")
        assert_closest_bitexact(out, exp, f"graph replay after another batch size {k}")
        assert np.array_equal(cnt.cpu().numpy(), R.intersects_count(o, d))


@pytest.mark.parametrize("subdiv", [10, 11])
def test_large_meshes_deep_trees_and_arrays_above_4gib(device, subdiv):
    """Size-independent properties at sizes the oracle cannot reach: 21 M triangles (a hierarchy of
    more than 32 levels with 32-bit addressing: the DEEP kernel variants) and, opt-in with
    TRIRO_TEST_HUGE=1, 84 M triangles (node and triangle arrays above 4 GiB: 64-bit addressing).
    first == closest's triangle, any == hit == (count > 0), loc is the barycentric point of the
    reported triangle, the multi-hit rows add up, a second build gives the same bits."""
    import os
    if subdiv == 11 and os.environ.get("TRIRO_TEST_HUGE") != "1":
        pytest.skip("84 M triangles: set TRIRO_TEST_HUGE=1 (about 20 s and 15 GB of device memory)")
    v, f = W.headline_mesh(subdiv)
    vt, ft = T(v, device), T(f, device)
    r = make(v, f, device)
    rad = float(np.linalg.norm(v[::997], axis=1).max())
    o, d = W.pinhole_grid(512, 512, distance=2.5 * rad)
    ot, dt = T(o, device), T(d, device)
    for _ in range(3):                                         # learned order, split blocks
        hit, front, tri, loc, uv = r.intersects_closest(ot, dt)
    assert 0.5 < float(hit.float().mean()) < 0.99 and int(tri.max()) < len(f)
    first, anyh, cnt = r.intersects_first(ot, dt), r.intersects_any(ot, dt), r.intersects_count(ot, dt)
    assert torch.equal(first, tri) and torch.equal(anyh, hit) and torch.equal(cnt > 0, hit)
    tv = vt[ft[tri[hit].long()].long()]
    w0, w1 = uv[hit][:, 0:1], uv[hit][:, 1:2]
    rec = w0 * tv[:, 0] + w1 * tv[:, 1] + (1 - w0 - w1) * tv[:, 2]
    assert float((rec - loc[hit]).abs().max()) <= 1e-5 * rad
    l3, ridx, tidx = r.intersects_location(ot, dt)
    assert len(ridx) == int(cnt.clamp(max=8).sum()) and torch.equal(torch.bincount(ridx.long(), minlength=cnt.numel()), cnt.clamp(max=8).reshape(-1).long())
    o2, d2 = W.hash_rays_torch(4_500_000, 5, v.min(0) * 1.5, v.max(0) * 1.5, device=device)   # streaming launch (above STEAL_MAX_RAYS; binary nodes below 8 M rays)
    h2 = r.intersects_closest(o2, d2)
    assert torch.equal(h2[0], r.intersects_any(o2, d2)) and torch.equal(h2[2], r.intersects_first(o2, d2))
    # the same batch through the streaming launch on the BINARY nodes (option wide = 0: the instantiations for hierarchies
    # of more than 32 levels, which run at a forced occupancy with a few spilled registers since round 5) and through the
    # direct launch (stream = 0): the same bits
    from triro.backend import ops as hops
    c2 = r.intersects_count(o2, d2)
    for name, val in (("wide", 0), ("stream", 0)):
        hops.set_option(name, val)
        try:
            g2 = r.intersects_closest(o2, d2)
            assert all(torch.equal(a, b) for a, b in zip(g2, h2)), name
            assert torch.equal(r.intersects_any(o2, d2), h2[0]) and torch.equal(r.intersects_first(o2, d2), h2[2])
            assert torch.equal(r.intersects_count(o2, d2), c2)
        finally:
            hops.set_option(name, 2 if name == "wide" else 1)
    r2 = make(v, f, device)
    hit2, front2, tri2, loc2, uv2 = r2.intersects_closest(ot, dt)
    assert torch.equal(tri2, tri) and torch.equal(loc2, loc) and torch.equal(uv2, uv) and torch.equal(front2, front)
    # what a sharded run exchanges: the slot forms of the records exist while the triangle array stays below 2 GiB
    # (32-bit byte offsets in the expansion); above that the tracer says so and the face form carries on
    assert r.packed_slots == (len(f) * 48 < (1 << 31)) and r.slot_records == r.packed_slots
    rec = r.intersects_closest_packed(ot, dt, slots=r.packed_slots)
    for a, e in zip(r2.closest_expand(rec, batch_shape=ot.shape[:-1], slots=r.packed_slots), (hit, front, tri, loc, uv)):
        assert torch.equal(a, e)
    if r.slot_records:
        for a, e in zip(r2.closest_from_slots(ot, dt, r.intersects_closest_slots(ot, dt)), (hit, front, tri, loc, uv)):
            assert torch.equal(a, e)


def test_last_launch_reports_the_shape_and_the_measured_node_flavour(device):
    """tr_bvh_last_launch: shape of the last direct launch; with grid_nodes = 0 / 2 the stealing closest
    launch reports the exact / grid nodes, with 1 it settles on one of them after the timed launches,
    and every flavour gives the oracle's answers."""
    import triro.backend.ops as hops
    v, f = W.icosphere(5)
    v = W.displaced(v, seed=11, amplitude=0.08)
    r = make(v, f, device)
    R = OracleIntersector(v, f, 1)
    o, d = W.pinhole_grid(320, 256, distance=2.5)
    ot, dt = T(o, device), T(d, device)
    exp = R.closest_raw(o.reshape(-1, 3), d.reshape(-1, 3))
    try:
        for gn in (0, 2, 1):
            hops.set_option("grid_nodes", gn)
            for rep in range(14):
                got = [g.reshape((-1,) + tuple(g.shape[2:])) for g in r.intersects_closest(ot, dt)]
                assert_closest_bitexact(got, exp, f"grid_nodes={gn} launch {rep}")
                assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy().reshape(-1), exp[2])
            torch.cuda.synchronize()
            r.intersects_closest(ot, dt)
            li = r.as_wrapper.last_launch()
            assert li["rays"] == 320 * 256 and li["blocks"] == 640 and li["query"] == 2 and li["shape"] == 1
            assert li["learned_order"] == 1 and li["slots"] >= li["blocks"] and li["addressing"] in (1, 2)
            if gn == 0: assert li["grid_nodes"] == 0
            if gn >= 1: assert li["grid_nodes"] == 1      # (round 5: no tuner, grid nodes from the first launch on)
        r.intersects_count(ot, dt)
        li = r.as_wrapper.last_launch()
        # (shape 3 = the unordered schedule with hand-over between lanes, round 3; 2 with usteal = 0)
        assert li["query"] == 3 and li["shape"] == 3 and li["grid_nodes"] == 1 and li["tile_rows_lg"] == 3
    finally:
        hops.set_option("grid_nodes", 1)
