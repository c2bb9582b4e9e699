"""GPU tests added in round 3.

VERDICT r02 weak #1b: the launch state `bench.py` times -- learned per-XCD order, split launch
slots, 8x8 tiles, the measured node flavour -- had only met the oracle on toy meshes.  Here the
BASELINE configs are launched 14 times on one stream at FULL size and EVERY launch is compared
bit for bit with the oracle; afterwards `tr_bvh_last_launch` must report the steady-state shape.
"""
import numpy as np
import pytest
import torch

import workloads as W
from launch_options import options
from oracle.oracle import OracleIntersector
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)

pytestmark = pytest.mark.gpu
LAUNCHES = 14


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def make(v, f, dev):
    from triro.ray.ray_optix import RayMeshIntersector
    return RayMeshIntersector(vertices=T(v, dev), faces=T(f, dev))


def rotate_y(x, deg):
    a = np.radians(deg)
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    out = x.copy()
    out[..., 0] = c * x[..., 0] + s * x[..., 2]
    out[..., 2] = -s * x[..., 0] + c * x[..., 2]
    return out


def assert_closest_exact(got, exp, what):
    hit, front, tri, loc, uv = [g.cpu().numpy() for g in got]
    assert np.array_equal(hit, exp[0]), f"{what}: hit mask, {int(np.sum(hit != exp[0]))} rays differ"
    assert np.array_equal(tri, exp[2]), f"{what}: tri_idx, {int(np.sum(tri != exp[2]))} rays differ"
    assert np.array_equal(front, exp[1]), f"{what}: front"
    # the contract is bit-exact for loc / uv as well (north_star asks for 1e-5 relative)
    assert np.array_equal(loc, exp[3]), f"{what}: loc bits, max |diff| {np.abs(loc - exp[3]).max()}"
    assert np.array_equal(uv, exp[4]), f"{what}: uv bits"


def steady_state(r, R, o, d, device, what):
    """14 launches of one batch on one stream, each against the oracle; returns the launch infos"""
    exp = R.closest_raw(o, d)
    shp = o.shape[:-1]
    exp = [exp[0].reshape(shp), exp[1].reshape(shp), exp[2].reshape(shp), exp[3].reshape(*shp, 3), exp[4].reshape(*shp, 2)]
    ot, dt = T(o, device), T(d, device)
    infos = []
    for k in range(LAUNCHES):
        got = r.intersects_closest(ot, dt)
        infos.append(r.as_wrapper.last_launch())
        assert_closest_exact(got, exp, f"{what} launch {k}")
    return infos


@pytest.fixture(scope="module")
def headline(device):
    v, f = W.headline_mesh(8)
    return v, f, make(v, f, device), OracleIntersector(v, f, 1)


def test_c5i_steady_state_launches_match_the_oracle(headline, device):
    """C5(i), the metric's config: every launch from the cold first one to the learned, split,
    tiled, grid-node steady state that bench.py times."""
    v, f, r, R = headline
    assert len(f) == 1310720
    o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    infos = steady_state(r, R, o, d, device, "C5(i)")
    last = infos[-1]
    assert infos[0]["learned_order"] == 0 and infos[0]["split_blocks"] == 0      # the cold call
    assert last["learned_order"] == 1 and last["split_blocks"] > 0, last
    assert last["tile_rows_lg"] == 3 and last["shape"] == 1 and last["blocks"] == 8192, last
    assert last["slots"] > last["blocks"]
    # round 5: no node-flavour tuner any more -- the grid nodes (fused box test) from the first launch on
    assert {i["grid_nodes"] for i in infos} == {1}, [i["grid_nodes"] for i in infos]


def test_c5i_moving_camera_sequence_matches_the_oracle(headline, device):
    """bench.py's moving-camera companion: the camera orbits by 0.25 degrees per step (8 frames,
    ping-pong), so the learned order and the split set are always one frame stale."""
    v, f, r, R = headline
    o0, d0 = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    frames = [(rotate_y(np.ascontiguousarray(o0), 0.25 * k), rotate_y(d0, 0.25 * k)) for k in range(8)]
    exps = []
    for o, d in frames:
        e = R.closest_raw(o, d)
        exps.append([e[0].reshape(1024, 1024), e[1].reshape(1024, 1024), e[2].reshape(1024, 1024),
                     e[3].reshape(1024, 1024, 3), e[4].reshape(1024, 1024, 2)])
    dev_frames = [(T(o, device), T(d, device)) for o, d in frames]
    seq = list(range(8)) + list(range(6, 0, -1))
    for k in range(2 * len(seq)):
        j = seq[k % len(seq)]
        assert_closest_exact(r.intersects_closest(*dev_frames[j]), exps[j], f"moving camera step {k} (frame {j})")
    last = r.as_wrapper.last_launch()
    assert last["learned_order"] == 1 and last["split_blocks"] > 0 and last["tile_rows_lg"] == 3, last


def test_c2_steady_state_launches_match_the_oracle(device):
    v, f, _label = W.bunny_mesh()
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    infos = steady_state(r, R, o, d, device, "C2")
    assert infos[-1]["learned_order"] == 1 and infos[-1]["shape"] == 1, infos[-1]


def test_c4_closest_steady_state_launches_match_the_oracle(device):
    v, f = W.nested_shells(7)
    r, R = make(v, f, device), OracleIntersector(v, f, 1)
    o, d = W.pinhole_grid(1024, 1024)
    infos = steady_state(r, R, o, d, device, "C4 closest")
    last = infos[-1]
    assert last["learned_order"] == 1 and last["split_blocks"] > 0 and last["tile_rows_lg"] == 3, last
    # count / location of the same batch learn their own order: 6 launches each against the oracle
    ot, dt = T(o, device), T(d, device)
    cnt = R.intersects_count(o.reshape(-1, 3), d.reshape(-1, 3)).reshape(1024, 1024)
    el, er, et = R.intersects_location(o, d)
    for k in range(6):
        assert np.array_equal(r.intersects_count(ot, dt).cpu().numpy(), cnt), f"C4 count launch {k}"
        loc, ray, tri = r.intersects_location(ot, dt)
        assert np.array_equal(ray.cpu().numpy(), er) and np.array_equal(tri.cpu().numpy(), et), f"C4 location launch {k}"
        assert np.array_equal(loc.cpu().numpy(), el), f"C4 location launch {k}: loc bits"


def test_packed_closest_expands_to_the_dense_outputs_bit_for_bit(headline, device):
    """tr_intersects_closest_packed (12 B/ray) + tr_closest_expand == tr_intersects_closest on C5(i), a
    C5(ii)-style hash batch (streaming launch) and C4 -- what a ray-sharded run sends over xGMI and what
    rank 0 rebuilds from it."""
    v, f, r, R = headline
    o, d = W.pinhole_grid(1024, 1024, distance=2.5 * float(np.linalg.norm(v, axis=1).max()))
    cases = [(r, T(o, device), T(d, device))]
    oh, dh = W.hash_rays_torch(3_000_001, 99, v.min(0) * 1.5, v.max(0) * 1.5, device=device)
    cases.append((r, oh, dh))
    v4, f4 = W.nested_shells(7)
    o4, d4 = W.pinhole_grid(1024, 1024)
    cases.append((make(v4, f4, device), T(o4, device), T(d4, device)))
    for rr, ot, dt in cases:
        dense = rr.intersects_closest(ot, dt)
        packed = rr.intersects_closest_packed(ot, dt)
        assert packed.shape == (ot.numel() // 3, 3) and packed.dtype == torch.int32
        got = rr.closest_expand(packed, batch_shape=ot.shape[:-1])
        for a, e in zip(got, dense):
            assert a.dtype == e.dtype and a.shape == e.shape and torch.equal(a, e)
        assert torch.equal(packed[:, 0] < 0, ~dense[0].reshape(-1))
        # expansion into row slices of preallocated outputs (how the gather pipeline uses it)
        n = packed.shape[0]
        outs = (torch.zeros(n, dtype=torch.bool, device=device), torch.zeros(n, dtype=torch.bool, device=device),
                torch.zeros(n, dtype=torch.int32, device=device), torch.zeros(n, 3, device=device), torch.zeros(n, 2, device=device))
        cut = n // 3
        rr.closest_expand(packed[:cut], outs=tuple(x[:cut] for x in outs))
        rr.closest_expand(packed[cut:], outs=tuple(x[cut:] for x in outs))
        for a, e in zip(outs, dense):
            assert torch.equal(a.reshape(e.shape), e)


@pytest.mark.timeout(600)
def test_sharded_exchange_on_rccl_world1():
    """the exchange code of triro.ray.sharded on the real backend (RCCL), one rank: tests/nccl_world1.py"""
    import os
    import subprocess
    import sys
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nccl_world1.py")
    from conftest import free_port
    p = subprocess.run([sys.executable, script, str(free_port())], capture_output=True, text=True, timeout=540, env=env)
    # (RCCL prints its version banner to stdout when the communicator is torn down)
    assert p.returncode == 0 and "OK" in p.stdout.split(), (p.stdout[-1500:], p.stderr[-3000:])


@pytest.mark.parametrize("usteal,split", [(1, 1), (2, 2), (4, 3), (64, 1), (0, 1)])
def test_unordered_count_with_stealing_matches_the_oracle(device, usteal, split):
    """count launches of the unordered schedule with hand-over between lanes (wave_count_unordered_steal),
    split launch slots for expensive blocks: forced thresholds, image / flat / on-surface batches, several launches each (cold ->
    learned order -> split slots), interleaved with closest launches of the same batch."""
    import triro.backend.ops as hops
    from test_gpu_round2 import on_surface_rays
    v, f = W.nested_shells(4, radii=(1.0, 0.8, 0.6, 0.45, 0.3))    # up to 10 hits per ray: beyond the cap of 8
    r = make(v, f, device)
    R = OracleIntersector(v, f, 1)
    o_img, d_img = W.pinhole_grid(512, 384)                       # 196 608 rays = 1 536 blocks
    o_on, d_on = on_surface_rays(v, f, r, device, n_each=6000, seed=7)
    lo, hi = v.min(0) * 1.2, v.max(0) * 1.2
    o_h, d_h = W.hash_rays(150_000, 5, lo, hi)
    cases = [("image", o_img, d_img), ("flat", o_img.reshape(-1, 3), d_img.reshape(-1, 3)), ("on-surface", o_on, d_on), ("hash", o_h, d_h)]
    try:
        hops.set_option("usteal", usteal)
        hops.set_option("split", split)
        hops.set_option("split_floor", 0)          # small test launches: let every candidate split
        for name, o, d in cases:
            cnt = R.intersects_count(o.reshape(-1, 3), d.reshape(-1, 3))
            tri = R.closest_raw(o.reshape(-1, 3), d.reshape(-1, 3))[2]
            e_loc, e_ray, e_tri = R.intersects_location(o.reshape(-1, 3), d.reshape(-1, 3))
            ot, dt = T(o, device), T(d, device)
            for rep in range(7):
                got = r.intersects_count(ot, dt).cpu().numpy().reshape(-1)
                assert np.array_equal(got, cnt), f"{name} usteal={usteal} split={split} launch {rep}: {int((got != cnt).sum())} rays differ"
                if rep % 3 == 2:
                    assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy().reshape(-1), tri)
                if rep % 2 == 1:       # the multi-hit list shared by the lanes that work on a ray
                    loc, ray, tri_l = r.intersects_location(ot, dt)
                    assert np.array_equal(ray.cpu().numpy(), e_ray) and np.array_equal(tri_l.cpu().numpy(), e_tri), f"{name} location launch {rep}"
                    assert np.array_equal(loc.cpu().numpy(), e_loc)
            if name == "image" and usteal:
                li = r.as_wrapper.last_launch()
                assert li["shape"] == 3 and li["learned_order"] == 1, li
        # contains_points runs on count
        pts = (np.random.default_rng(1).random((4000, 3)) * 2.2 - 1.1).astype(np.float32)
        assert np.array_equal(r.contains_points(T(pts, device)).cpu().numpy(), R.contains_points(pts))
    finally:
        for k, val in (("usteal", 1), ("split", 1), ("split_floor", 40)):
            hops.set_option(k, val)


# variant -> options.  (The test was written for the LDS-staged table of the top levels and for eight waves per SIMD, two
# launch variants that no longer exist; it keeps its name and its variant ids, and now runs the stealing launch on each
# node flavour it can take.)
NODE_VARIANTS = {
    1: dict(grid_nodes=1),                               # the 32-byte grid nodes
    2: dict(grid_nodes=0),                               # the exact 64-byte nodes
    -8: dict(grid_nodes=2, steal=4, split_floor=0),      # grid nodes, stealing forced from the fourth trip, no time floor for split blocks
}


@pytest.mark.parametrize("variant", list(NODE_VARIANTS))
def test_lds_staged_node_packets_match_the_oracle(device, variant):
    """The node flavours of the stealing closest / first launches (option grid_nodes, NODE_VARIANTS).
    Image (tiles), flat, on-surface and hash batches, several launches each, a refit and a rebuild in
    between (the grid nodes are derived data), a save / load round trip, and a mesh of a few dozen nodes."""
    from test_gpu_round2 import on_surface_rays
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = W.icosphere(5)
    v = W.displaced(v, seed=4, amplitude=0.07)
    r = make(v, f, device)
    o_img, d_img = W.pinhole_grid(384, 256, distance=2.5)
    grid_nodes = NODE_VARIANTS[variant]["grid_nodes"]
    with options(**NODE_VARIANTS[variant]):
        for step, (vv, how) in enumerate([(v, "build"), (W.displaced(v, seed=9, amplitude=0.03), "refit"), (v * np.float32(1.1), "update")]):
            if how == "refit":
                r.refit(T(vv, device))
            elif how == "update":
                r.update_raw(T(vv, device), T(f, device))
            R = OracleIntersector(vv, f, 1)
            o_on, d_on = on_surface_rays(vv, f, r, device, n_each=1200, seed=step)
            o_h, d_h = W.hash_rays(70_000, 11 + step, vv.min(0) * 1.3, vv.max(0) * 1.3)
            for name, o, d in (("image", o_img, d_img), ("flat", o_img.reshape(-1, 3), d_img.reshape(-1, 3)), ("on-surface", o_on, d_on), ("hash", o_h, d_h)):
                exp = R.closest_raw(o.reshape(-1, 3), d.reshape(-1, 3))
                ot, dt = T(o, device), T(d, device)
                for rep in range(4):
                    got = [g.reshape((-1,) + tuple(g.shape[o.ndim - 1:])) for g in r.intersects_closest(ot, dt)]
                    for g, e in zip(got, exp[:5]):
                        assert np.array_equal(g.cpu().numpy(), e), f"variant {variant} (grid_nodes={grid_nodes}) {how} {name} launch {rep}"
                    assert np.array_equal(r.intersects_first(ot, dt).cpu().numpy().reshape(-1), exp[2])
            li = r.as_wrapper.last_launch()
            assert li["grid_nodes"] == (1 if grid_nodes else 0) and li["shape"] == 1
        import tempfile, os
        with tempfile.TemporaryDirectory() as td:
            r.save(os.path.join(td, "m"))
            r2 = RayMeshIntersector.load(os.path.join(td, "m"), device=device)
        a, b2 = r.intersects_closest(T(o_img, device), T(d_img, device)), r2.intersects_closest(T(o_img, device), T(d_img, device))
        for x, y in zip(a, b2):
            assert torch.equal(x, y)
        # a mesh of a few dozen nodes
        vs, fs = W.icosphere(1)
        rs, Rs = make(vs, fs, device), OracleIntersector(vs, fs, 1)
        os_, ds_ = W.pinhole_grid(128, 128, distance=3.0)
        exp = Rs.closest_raw(os_.reshape(-1, 3), ds_.reshape(-1, 3))
        for rep in range(3):
            got = rs.intersects_closest(T(os_, device), T(ds_, device))
            for g, e in zip(got, exp[:5]):
                assert np.array_equal(g.cpu().numpy().reshape(e.shape), e)


@pytest.mark.timeout(900)
def test_bench_result_pipeline_on_rccl_one_rank():
    """bench.py's N > 1 step -- packed trace in chunks, asynchronous RCCL exchange, expansion on a side stream,
    double buffering, `verified` against the cold first call -- under torch.distributed.run with ONE rank
    (`--force-gather`): the multi-GPU code path on the real backend, as far as a single-GPU box can take it."""
    import json
    import os
    import subprocess
    import sys
    from conftest import free_port
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for extra in (["--workload", "c5i"], ["--workload", "c5i", "--scaling", "strong"],
                  ["--workload", "c5ii", "--total-rays", "7000001", "--chunks", "3"],
                  ["--workload", "c5i", "--records", "packed"],
                  ["--workload", "c5ii", "--total-rays", "7000001", "--chunks", "3", "--records", "packed"],
                  # round 6: the step as one C call (libtriro_rccl.so), preflighted like every rung
                  ["--workload", "c5i", "--exchange", "native"],
                  ["--workload", "c5ii", "--total-rays", "7000001", "--chunks", "3", "--exchange", "native"]):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "6",
               "--warmup", "2", "--min-warmup-ms", "0", "--full", "--no-cpu-baseline", "--no-companions", "--force-gather"] + extra
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-800:], p.stderr[-2500:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')][-1]
        r = json.loads(line)
        assert r["verified"] is True and r["n_gpus"] == 1 and r["value"] > 100
        want = "12 B/ray packed records over RCCL" if "packed" in extra else "4 B/ray slot records over RCCL"       # (round 4: rank 0 holds the rays by default)
        assert want in r["config"]["parallelism"] and "--force-gather" in r["config"]["parallelism"]
        if "native" in extra:
            assert r["config"]["exchange_mode_used"] == "native" and "tr_sharded_closest_step" in r["config"]["parallelism"], r["config"]


def test_packed_closest_edge_cases(device):
    """12-byte packed records on the inputs the dense path is tested with: a single-triangle mesh (no
    hierarchy), zero rays, NaN / Inf rays (miss), broadcast and strided ray tensors, three batch dims."""
    from triro.ray.ray_optix import RayMeshIntersector
    v1 = np.array([[0.5, -0.5, 0], [0, 0.5, 0], [-0.5, -0.5, 0]], np.float32)
    f1 = np.array([[0, 1, 2]], np.int32)
    r1 = RayMeshIntersector(vertices=T(v1, device), faces=T(f1, device))
    o = torch.tensor([[0, 0, 4.0], [10, 10, 10], [float("nan"), 0, 1], [0, 0, -4.0]], device=device)
    d = torch.tensor([[0, 0, -1.0], [0, 1, 0], [0, 0, -1], [0, 0, float("inf")]], device=device)
    dense = r1.intersects_closest(o, d)
    got = r1.closest_expand(r1.intersects_closest_packed(o, d))
    for a, e in zip(got, dense):
        assert torch.equal(a, e)
    assert dense[0].tolist() == [True, False, False, False] and got[2].tolist() == [0, -1, -1, -1]
    empty = r1.intersects_closest_packed(torch.zeros(0, 3, device=device), torch.zeros(0, 3, device=device))
    assert empty.shape == (0, 3)
    assert [tuple(x.shape) for x in r1.closest_expand(empty)] == [(0,), (0,), (0,), (0, 3), (0, 2)]
    v, f = W.icosphere(4)
    r = make(v, f, device)
    # stride-0 origin, three batch dims, non-contiguous directions
    dn = W.pinhole_grid(40, 24)[1].reshape(2, 12, 40, 3)
    big = torch.zeros(2, 12, 40, 6, device=device)
    big[..., ::2] = T(dn, device)
    dirs = big[..., ::2]
    assert not dirs.is_contiguous()
    org = torch.tensor([0.0, 0.0, 2.5], device=device).expand(2, 12, 40, 3)
    dense = r.intersects_closest(org, dirs)
    got = r.closest_expand(r.intersects_closest_packed(org, dirs), batch_shape=(2, 12, 40))
    for a, e in zip(got, dense):
        assert a.shape == e.shape and torch.equal(a, e)
    with pytest.raises(ValueError):
        r.closest_expand(torch.zeros(5, 3, device=device))                      # not int32
    with pytest.raises(ValueError):
        r.intersects_closest_packed(org, dirs, out=torch.zeros(7, 3, dtype=torch.int32, device=device))


def test_hip_path_reproduces_the_reference_s_published_readme_image(device):
    """README.md:31-53 run through the HIP path, statement for statement, against the reference's own
    published rendering of it (assets/location.png -> tests/golden/reference_readme_location_axes.npz):
    the one comparison with reference-PRODUCED data that exists (8-bit image precision)."""
    pytest.importorskip("PIL")
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from readme_image import assert_matches_reference_image, compare_with_reference_image
    from triro.ray.ray_optix import RayMeshIntersector

    class Mesh:                                   # any object with .vertices / .faces (trimesh is not installed)
        vertices, faces = W.icosphere(3)
    intersector = RayMeshIntersector(mesh=Mesh)
    y, x = torch.meshgrid([torch.linspace(1, -1, 800), torch.linspace(-1, 1, 800)], indexing='ij')
    z = -torch.ones_like(x)
    ray_directions = torch.stack([x, y, z], dim=-1).to(device)
    ray_origins = torch.Tensor([0, 0, 3]).to(device).broadcast_to(ray_directions.shape)
    hit, front, ray_idx, tri_idx, location, uv = intersector.intersects_closest(ray_origins, ray_directions, stream_compaction=True)
    locs = torch.zeros((800, 800, 3), device=device)
    locs[hit] = location
    assert_matches_reference_image(compare_with_reference_image(locs.cpu().numpy()))
