"""The net of tests/poison.py has bite.

CPU part: fake launches into tensors that come through the allocation seam of triro.backend.ops -- one that writes
everything passes, one that skips a block, leaves bool bytes behind or hands back a poisoned packed record is reported.
GPU part: a real launch that is handed only the first half of a batch, with pointers into full-size poisoned outputs,
must leave exactly the second half flagged; the observation this module exists for -- how often the caching
allocator hands a steady-state launch a block an earlier launch of the loop already filled -- is printed; and the
places where a launch is most likely to leave something unwritten (ragged batches in the learned, split and tiled
steady state that tr_bvh_last_launch confirms, images no tile shape takes, streaming launches repeated on one handle, meshes without a hierarchy, rays that cannot hit, zero rays, the
record expansions on shapes the tiled kernel does not take) are swept against the oracle on poisoned outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import poison
import workloads as W
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

N = 1024
CPU = torch.device("cpu")


def new_outputs(n, device=CPU):
    """the five closest-hit outputs, allocated the way ops.intersects_closest allocates them"""
    import triro.backend.ops as ops
    return (ops._new_output((n,), torch.bool, device), ops._new_output((n,), torch.bool, device),
            ops._new_output((n,), torch.int32, device), ops._new_output((n, 3), torch.float32, device),
            ops._new_output((n, 2), torch.float32, device))


def fake_launch(outs, lo, hi):
    """writes rays [lo, hi) the way a launch in which every ray misses does: zeros, and -1 for the triangle"""
    hit, front, tri, loc, uv = outs
    hit[lo:hi] = False
    front[lo:hi] = False
    tri[lo:hi] = -1
    loc[lo:hi] = 0.0
    uv[lo:hi] = 0.0


def test_the_seam_is_swapped_and_restored():
    import triro.backend.ops as ops
    import triro.ray.sharded as sharded
    assert poison.installed() and ops._new_output is poison.poisoned and sharded._new_output is poison.poisoned
    assert getattr(ops.intersects_closest, "__wrapped_by_poison__", False)
    poison.uninstall()
    try:
        assert ops._new_output is not poison.poisoned and sharded._new_output is not poison.poisoned
        assert not hasattr(ops.intersects_closest, "__wrapped_by_poison__")
        assert ops._new_output((3,), torch.int32, CPU).shape == (3,)
    finally:
        poison.install()
    # the sharded module's own allocator (what its tests count) goes through the seam
    assert int(sharded.ShardedRayMeshIntersector._alloc((4,), torch.int32, CPU)[0]) == poison.INT32


def test_every_type_is_born_poisoned_bit_for_bit():
    outs = new_outputs(N)
    assert np.all(outs[0].view(torch.uint8).numpy() == 0xA5)
    assert np.all(outs[2].numpy().view(np.uint32) == 0xA5A5A5A5)
    assert np.all(outs[3].numpy().view(np.uint32) == 0x7FA5A5A5) and np.all(np.isnan(outs[3].numpy()))
    import triro.backend.ops as ops
    off = ops._new_output((7,), torch.int64, CPU)
    assert np.all(off.numpy().view(np.uint64) == 0xA5A5A5A5A5A5A5A5) and int(off[0]) < 0
    for t in (*outs, off):
        assert bool(poison.stale_mask(t).all())
        with pytest.raises(AssertionError, match=f"{t.numel()} of {t.numel()} elements"):
            poison.assert_written(t)
    # a computed NaN (0 * inf: the default quiet NaN) is not the poison: compared as bits, not with isnan
    nan = torch.tensor([float("inf")]) * 0.0
    assert bool(torch.isnan(nan).all())
    poison.assert_written(nan)
    poison.assert_written(torch.zeros((0, 3)), None, torch.zeros(0, dtype=torch.bool))       # empty and absent outputs


def test_a_launch_that_writes_everything_passes():
    outs = new_outputs(N)
    fake_launch(outs, 0, N)
    poison.assert_written(*outs, what="fake launch")


def test_a_launch_that_skips_one_block_is_reported_with_its_size():
    outs = new_outputs(N)
    fake_launch(outs, 0, 384)
    fake_launch(outs, 512, N)            # block 3 of 8 (128 rays) is never dealt
    with pytest.raises(AssertionError) as err:
        poison.assert_written(*outs, what="fake launch")
    assert "fake launch[0]" in str(err.value) and "128 of 1024 elements" in str(err.value) and "flat index 384" in str(err.value)
    for k, per_ray in ((2, 1), (3, 3), (4, 2)):
        with pytest.raises(AssertionError, match=f"{128 * per_ray} of {N * per_ray} elements.*flat index {384 * per_ray}"):
            poison.assert_written(outs[k], what="fake launch")
        mask = poison.stale_mask(outs[k]).reshape(N, -1)
        assert bool(mask[384:512].all()) and int(mask.sum()) == 128 * per_ray


def test_true_over_a_poisoned_bool_buffer_needs_the_raw_byte_check():
    import triro.backend.ops as ops
    hit = ops._new_output((N,), torch.bool, CPU)
    hit[:N - 5] = True
    # what a comparison with the expected mask sees: a byte of 0xA5 read as bool is True
    assert np.array_equal(hit.numpy(), np.ones(N, bool))
    with pytest.raises(AssertionError, match=f"5 of {N} elements.*flat index {N - 5}"):
        poison.assert_written(hit, what="hit")
    hit[N - 5:] = True
    poison.assert_written(hit, what="hit")


def test_the_int32_poison_is_not_a_miss_and_a_miss_is_not_poison():
    assert poison.INT32 == -1515870811 and poison.INT32 != -1 and poison.INT64 < 0
    outs = new_outputs(1)
    fake_launch(outs, 0, 1)              # one ray that misses: zeros, tri -1
    poison.assert_written(*outs, what="a miss")
    assert outs[2].tolist() == [-1] and outs[3].tolist() == [[0.0, 0.0, 0.0]]
    zeros = torch.zeros(16, dtype=torch.int32)      # counts of rays that cross nothing
    poison.assert_written(zeros, zeros.to(torch.int64), zeros.to(torch.bool), zeros.to(torch.float32))


def test_a_poisoned_packed_record_is_reported_not_expanded_as_a_miss():
    import triro.backend.ops as ops
    rec = ops._new_output((N, 3), torch.int32, CPU)
    rec[:N - 1] = torch.tensor([5, 0, 0], dtype=torch.int32)
    # by the ABI (tr_packed_hit) bit 31 of the first word says "miss" and the other words are ignored: an expansion of
    # the stale record would give the zeros and the -1 of a plausible miss
    assert int(rec[N - 1, 0]) & 0x80000000
    with pytest.raises(AssertionError, match=f"3 of {3 * N} elements.*flat index {3 * (N - 1)}"):
        poison.assert_written(rec, what="packed records")
    rec[N - 1] = -1                       # the record the kernel writes for a miss
    poison.assert_written(rec, what="packed records")


def test_outs_handed_in_are_checked_when_the_caller_poisoned_them():
    buf = torch.full((N,), -7, dtype=torch.int32)
    poison.assert_written(buf)            # the caller's own pre-fill is none of this module's business
    poison.fill(buf[256:])
    with pytest.raises(AssertionError, match=f"{N - 256} of {N} elements"):
        poison.assert_written(buf)
    rows = torch.zeros((8, 3))
    poison.fill(rows[2:4])                # a row slice: a view, filled in place
    assert int(poison.stale_mask(rows).sum()) == 6


# ---- GPU part ------------------------------------------------------------------------------------------------------
def _scene(device):
    from oracle.oracle import OracleIntersector
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(5)
    v = W.displaced(v, seed=8, amplitude=0.05)
    o, d = W.hash_rays(200_000, 31, v.min(0) * 1.5, v.max(0) * 1.5)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    r = RayMeshIntersector(vertices=torch.from_numpy(v).to(device), faces=torch.from_numpy(f).to(device))
    return r, OracleIntersector(v, f, 1), o, d


@pytest.mark.gpu
def test_a_launch_on_half_a_batch_leaves_exactly_the_other_half_flagged(device):
    """tr_intersects_closest on the first half of the rays, with pointers into full-size poisoned outputs (valid, fully
    allocated: nothing is out of bounds): the first half holds the oracle's bits, the second half -- and nothing else --
    is reported.  What a launch that deals only half of its blocks would look like to the net."""
    import triro.backend.ops as ops
    r, R, o, d = _scene(device)
    n, half = len(o), len(o) // 2
    ot, dt = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    outs = new_outputs(n, device)
    rays = ops.make_rays(ot[:half], dt[:half])
    ops._check(ops.get_module().tr_intersects_closest(r.as_wrapper._inner, C.byref(rays), *(t.data_ptr() for t in outs),
                                                      torch.cuda.current_stream(device).cuda_stream))
    torch.cuda.synchronize()
    exp = R.intersects_closest(o[:half], d[:half])[:5]
    assert 0.05 < float(np.mean(exp[0])) < 0.95          # hits and misses: the zeros of a miss are written, too
    for name, t, e, per_ray in zip(("hit", "front", "tri", "loc", "uv"), outs, exp, (1, 1, 1, 3, 2)):
        mask = poison.stale_mask(t).reshape(n, -1).cpu().numpy()
        assert not mask[:half].any(), f"{name}: {int(mask[:half].sum())} elements of the traced half still hold the poison"
        assert mask[half:].all(), f"{name}: {int((~mask[half:]).sum())} elements beyond the traced half were written"
        with pytest.raises(AssertionError, match=f"{(n - half) * per_ray} of {n * per_ray} elements.*flat index {half * per_ray}"):
            poison.assert_written(t, what=name)
        poison.assert_written(t[:half], what=name)
        got = t[:half].view(torch.uint8).cpu().numpy() if t.dtype == torch.bool else t[:half].cpu().numpy()
        assert np.array_equal(got, e.astype(np.uint8) if t.dtype == torch.bool else e), f"{name}: the traced half differs from the oracle"
    # the whole batch through the wrapped entry point: checked there, and nothing is left
    poison.assert_written(*r.intersects_closest(ot, dt), what="the whole batch")


@pytest.mark.gpu
def test_the_allocator_recycles_the_outputs_of_a_steady_state_loop(device, capsys):
    """The premise of the net, observed (never asserted: the allocator's behaviour is not this project's to pin): with
    the fixture OFF, the loop shape of test_gpu_round3.steady_state -- `got = r.intersects_closest(o, d)` again and
    again -- and which launches were handed an output block an earlier launch of the loop had filled.  MEASURED on an
    MI355X (torch 2.x caching allocator): see RECYCLED in the printed line; the last figure is quoted in DESIGN.md."""
    r, R, o, d = _scene(device)
    ot, dt = torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)
    poison.uninstall()
    try:
        seen, recycled, got = set(), [], None
        for k in range(6):
            got = r.intersects_closest(ot, dt)
            ptrs = [t.data_ptr() for t in got]
            recycled.append(sum(p in seen for p in ptrs))
            seen.update(ptrs)
        torch.cuda.synchronize()
    finally:
        poison.install()
    launches = sum(1 for c in recycled if c)
    with capsys.disabled():
        print(f"\nRECYCLED: {launches} of 6 steady-state launches were handed output blocks an earlier launch of the loop had "
              f"filled ({sum(recycled)} of {5 * 6} output tensors; per launch {recycled})")
    assert len(recycled) == 6


# ---- where a launch is most likely to leave something unwritten: every result below comes back through the wrapped entry
# points (checked for poison there) and is compared with the oracle bit for bit ---------------------------------------------
def _dev(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)        # (a copy: contiguous, and writable also when x is a 1 x 1 broadcast)


def _all_queries_match(r, R, o, d, device, what, location=True):
    """every query family on one batch (numpy, flat or image-shaped) against the oracle; results arrive poison-checked"""
    ot, dt = _dev(o, device), torch.from_numpy(d).to(device)        # (a pinhole origin keeps its stride-0 broadcast on the host only)
    for name, g, e in zip(("hit", "front", "tri", "loc", "uv"), r.intersects_closest(ot, dt), R.intersects_closest(o, d)[:5]):
        assert np.array_equal(g.cpu().numpy(), e, equal_nan=True), f"{what}: closest {name}"
    cnt = R.intersects_count(o, d)
    assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), cnt), f"{what}: count"
    assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy(), cnt > 0), f"{what}: any"
    assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy(), R.intersects_first(o, d)), f"{what}: first"
    if location:
        for name, g, e in zip(("loc", "ray", "tri"), r.intersects_location(ot, dt), R.intersects_location(o.reshape(-1, 3), d.reshape(-1, 3))):
            assert np.array_equal(g.cpu().numpy(), e), f"{what}: location {name}"


# (what, width, height, rays of the flattened image that are traced -- None: the image as [H, W, 3] --, tile rows (log2) and
# whether split slots exist in the steady state).  The mesh has 81 920 triangles: below 655 360 rays its triangles count as
# small on screen (8 x 8 tiles with split slots), from there on as large (flat tiles, no split slots).  128 rays per block.
RAGGED = (
    # 520 000 rays = 4062.5 blocks: 8 x 8 tiles over whole rows, the last block half beyond the batch
    ("8 x 8 tiles and split slots, half a last block", 1000, 520, None, 3, True),
    # 517 rows: the block -> ray map is laid over 520 rows, three tile rows of every last tile lie beyond the batch
    ("8 x 8 tiles over rows padded to whole tiles", 1000, 517, None, 3, True),
    # 200 001 flat rays = 1562 blocks and 65 rays: split slots without tiles
    ("flat batch, split slots, half a last block", 1000, 520, 200_001, 0, True),
    # 656 832 rays: 2 x 32 tiles, over 622 rows padded to 624; 5131.5 blocks
    ("2 x 32 tiles over padded rows, half a last block", 1056, 622, None, 1, False),
)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RAGGED, ids=[c[0] for c in RAGGED])
def test_ragged_batches_in_the_learned_split_and_tiled_steady_state_leave_nothing_unwritten(device, case):
    """Batches whose last block, last tile row or both reach beyond the batch, in shapes the launch policy really tiles,
    pads and splits (tr_bvh_last_launch says so, as in test_gpu_round3): twelve closest-hit launches from the cold one
    to the steady state, then every other query on the same handle, each launch against the oracle on poisoned outputs."""
    from oracle.oracle import OracleIntersector
    from triro.ray.ray_optix import RayMeshIntersector
    what, width, height, flat_n, rows_lg, split = case
    v, f = W.icosphere(6)
    v = W.displaced(v, seed=8, amplitude=0.05)
    assert len(f) == 81920
    r = RayMeshIntersector(vertices=_dev(v, device), faces=_dev(f, device))
    R = OracleIntersector(v, f, 1)
    o, d = W.pinhole_grid(width, height, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    o = np.array(np.broadcast_to(o, d.shape), order="C")
    if flat_n is not None:
        o, d = o.reshape(-1, 3)[:flat_n].copy(), d.reshape(-1, 3)[:flat_n].copy()
    n = o.size // 3
    assert n % 128 != 0                                             # the last block is ragged
    ot, dt = _dev(o, device), _dev(d, device)
    exp = R.intersects_closest(o, d)[:5]
    cnt = R.intersects_count(o, d)
    assert 0.2 < float(np.mean(exp[0])) < 0.98
    infos = []
    for launch in range(12):
        got = r.intersects_closest(ot, dt)
        infos.append(r.as_wrapper.last_launch())
        for name, g, e in zip(("hit", "front", "tri", "loc", "uv"), got, exp):
            assert np.array_equal(g.cpu().numpy(), e), f"{what}: closest {name}, launch {launch} ({infos[-1]})"
    padded_rows = (height + 7) // 8 * 8 if (flat_n is None and height % 8) else height
    blocks = ((padded_rows * width if flat_n is None else n) + 127) // 128
    assert infos[0]["learned_order"] == 0 and infos[0]["split_blocks"] == 0, infos[0]      # the cold launch
    for li in infos[-4:]:                                           # a measuring launch and the three that follow it
        assert li["rays"] == n and li["blocks"] == blocks and li["query"] == 2 and li["shape"] == 1, (what, li)
        assert li["learned_order"] == 1 and li["tile_rows_lg"] == rows_lg and (li["split_blocks"] > 0) == split, (what, li)
        assert (li["slots"] > li["blocks"]) == split, (what, li)
    # the other queries on the same handle: any / first share the closest launches' order, count learns its own
    for q, want in (("any", cnt > 0), ("first", exp[2]), ("count", cnt)):
        for launch in range(8):
            got = getattr(r, "intersects_" + q)(ot, dt)
            li = r.as_wrapper.last_launch()
            assert np.array_equal(got.cpu().numpy(), want), f"{what}: {q}, launch {launch} ({li})"
        assert li["rays"] == n and li["blocks"] == blocks and li["learned_order"] == 1, (what, q, li)
        if q != "count":
            assert li["tile_rows_lg"] == rows_lg and (li["split_blocks"] > 0) == split, (what, q, li)
    for name, g, e in zip(("loc", "ray", "tri"), r.intersects_location(ot, dt), R.intersects_location(o.reshape(-1, 3), d.reshape(-1, 3))):
        assert np.array_equal(g.cpu().numpy(), e), f"{what}: location {name}"
    # ... and closest again, after the other queries have used the handle's scheduling state
    for launch in range(4):
        got = r.intersects_closest(ot, dt)
        li = r.as_wrapper.last_launch()
        for name, g, e in zip(("hit", "front", "tri", "loc", "uv"), got, exp):
            assert np.array_equal(g.cpu().numpy(), e), f"{what}: closest {name} after the other queries, launch {launch} ({li})"
    assert li["learned_order"] == 1 and li["tile_rows_lg"] == rows_lg and (li["split_blocks"] > 0) == split, (what, li)


@pytest.mark.gpu
def test_images_that_no_tile_shape_takes_leave_nothing_unwritten(device):
    """image batches whose width is no multiple of 8, 16 or 32 (rows of 64 pixels, no tiles, no padding), down to one
    pixel: every query, six rounds on one handle; the closest launch of each round reports the untiled shape and, from
    the second round on, the learned order wherever the batch is large enough to have one (more than 64 blocks)"""
    from oracle.oracle import OracleIntersector
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(6)
    v = W.displaced(v, seed=8, amplitude=0.05)
    r = RayMeshIntersector(vertices=_dev(v, device), faces=_dev(f, device))
    R = OracleIntersector(v, f, 1)
    for width, height in ((203, 101), (1021, 517), (33, 7), (1, 1)):
        o, d = W.pinhole_grid(width, height, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
        for launch in range(6):
            what = f"{width} x {height} launch {launch}"
            ot, dt = _dev(o, device), _dev(d, device)
            got = r.intersects_closest(ot, dt)
            li = r.as_wrapper.last_launch()
            assert li["query"] == 2 and li["rays"] == width * height and li["tile_rows_lg"] == 0 and li["split_blocks"] == 0, (what, li)
            if launch >= 2 and li["blocks"] > 64:
                assert li["learned_order"] == 1, (what, li)
            for name, g, e in zip(("hit", "front", "tri", "loc", "uv"), got, R.intersects_closest(o, d)[:5]):
                assert np.array_equal(g.cpu().numpy(), e), f"{what}: closest {name}"
            _all_queries_match(r, R, o, d, device, what, location=launch in (0, 5))


@pytest.mark.gpu
def test_streaming_launches_repeated_on_one_handle_leave_nothing_unwritten(device):
    """the streaming launch hands out ray ranges from a work counter that every launch has to find reset: a ragged flat
    batch, four launches per query on one handle, on the binary and on the 8-wide nodes"""
    from launch_options import options
    from oracle.oracle import OracleIntersector
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(5)
    v = W.displaced(v, seed=8, amplitude=0.05)
    R = OracleIntersector(v, f, 1)
    o, d = W.hash_rays(200_001, 31, v.min(0) * 1.5, v.max(0) * 1.5)
    for wide in (0, 1):
        with options(stream=2, wide=wide):
            r = RayMeshIntersector(vertices=_dev(v, device), faces=_dev(f, device))
            for launch in range(4):
                _all_queries_match(r, R, o, d, device, f"streaming, wide={wide}, launch {launch}", location=False)
            with pytest.raises(ValueError, match="no direct launch"):      # (they were streaming launches)
                r.as_wrapper.last_launch()


@pytest.mark.gpu
def test_meshes_without_a_hierarchy_and_rays_that_cannot_hit_leave_nothing_unwritten(device):
    """one triangle (num_tris < 2 skips the traversal), two triangles, NaN / Inf / zero-direction rays, zero rays: misses
    are WRITTEN (zeros, -1), in every query, in the direct and in the streaming launch"""
    from launch_options import options
    from oracle.oracle import OracleIntersector
    from triro.ray.ray_optix import RayMeshIntersector
    v = np.array([[0.5, -0.5, 0.0], [0.0, 0.5, 0.0], [-0.5, -0.5, 0.0], [0.5, -0.5, -1.0], [0.0, 0.5, -1.0], [-0.5, -0.5, -1.0]], np.float32)
    o, d = W.hash_rays(70_001, 5, [-1.0, -1.0, 0.5], [1.0, 1.0, 2.0])
    d[:, 2] = -np.abs(d[:, 2]) - np.float32(0.2)          # downwards: a good share hits
    o[::11, 0] = np.nan
    d[::13, 1] = np.inf
    d[::17] = 0.0
    for nt in (1, 2):
        f = np.arange(3 * nt, dtype=np.int32).reshape(nt, 3)
        R = OracleIntersector(v, f, 1)
        assert 0.02 < float(np.mean(R.intersects_count(o, d) > 0)) < 0.9
        for opts in (dict(), dict(stream=2), dict(stream=0, steal=0), dict(stream=0, steal=2)):
            with options(**opts):
                r = RayMeshIntersector(vertices=_dev(v, device), faces=_dev(f, device))
                for launch in range(2):
                    _all_queries_match(r, R, o, d, device, f"{nt} triangle(s), {opts}, launch {launch}")
                _all_queries_match(r, R, o[:1], d[:1], device, f"{nt} triangle(s), {opts}, one ray")
                _all_queries_match(r, R, o[:0], d[:0], device, f"{nt} triangle(s), {opts}, zero rays")
                # the records of a sharded run and their expansions, rows-tiled where the shape allows and linear where not
                for rows, width in ((64, 32), (5, 32), (8, 33)):
                    m = rows * width
                    ot, dt = _dev(o[:m], device), _dev(d[:m], device)
                    exp = r.intersects_closest(ot, dt)
                    rec_s, rec_f = r.intersects_closest_packed(ot, dt, slots=True), r.intersects_closest_packed(ot, dt)
                    slot = r.intersects_closest_slots(ot, dt)
                    for got in (r.closest_expand(rec_f), r.closest_expand(rec_s, slots=True), r.closest_expand(rec_s, slots=True, row_length=width),
                                r.closest_from_slots(ot, dt, slot), r.closest_from_slots(ot, dt, slot, row_length=width)):
                        for a, e in zip(got, exp):
                            assert torch.equal(a, e), (nt, opts, rows, width)
