"""Round 6 GPU tests: batches beyond 2^31 / 2^32 rays (the 64-bit ray indexing SURVEY 7.3 claims), the int32 ray_idx
guard, the watertight contract on rays aimed at shared edges and vertices."""
import numpy as np
import pytest
import torch

import workloads as W
from oracle.oracle import OracleIntersector
from test_gpu_round2 import T, make
import poison
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(900)
def test_batches_of_more_than_2_to_the_32_rays(device):
    """VERDICT r05 "next" #5: the reference's getRay multiplies the flat index by 3 in `int` (shaders.cu:37) and is
    wrong from 715 827 883 rays on; this path claims 64-bit index math throughout -- here it is exercised: ONE call on
    a [65 600, 65 521, 3] batch = 4 298 177 600 rays (> 2^32; origins vary along the first batch dimension, directions
    along the second, both broadcast with stride 0 along the other: the tensors hold 0.8 MB each, the outputs 4.3 GB /
    17 GB), through intersects_any and intersects_first, compared row block by row block with the same rays traced as small
    explicit batches -- at the start, around flat indices 2^31 and 2^32, and at the end.  65 521 is prime: a flat index
    that wrapped at 2^31 or 2^32 would pair the wrong origin with the wrong direction."""
    free, _ = torch.cuda.mem_get_info(device)
    if free < 40 * (1 << 30):
        pytest.skip("needs ~25 GB of device memory for the int32 output of 4.3 G rays")
    v, f = W.icosphere(4)
    v = W.displaced(v, seed=6, amplitude=0.05)
    r = make(v, f, device)
    A, B = 65600, 65521
    assert A * B > (1 << 32)
    rng = np.random.default_rng(5)
    oa = (rng.standard_normal((A, 3)) * 0.15 + np.array([0.0, 0.0, 3.0])).astype(np.float32)      # a cloud of eye points
    db = rng.standard_normal((B, 3)).astype(np.float32) * np.float32(0.35) + np.array([0.0, 0.0, -1.0], np.float32)
    o_t = T(oa, device).reshape(A, 1, 3).expand(A, B, 3)
    d_t = T(db, device).reshape(1, B, 3).expand(A, B, 3)
    assert o_t.stride()[1] == 0 and d_t.stride()[0] == 0
    rows = sorted({0, 1, (1 << 31) // B - 1, (1 << 31) // B, (1 << 31) // B + 1, (1 << 32) // B - 1, (1 << 32) // B,
                   (1 << 32) // B + 1, A - 2, A - 1})
    ref_any, ref_first = {}, {}
    for a in rows:      # the same rays as explicit contiguous [B, 3] batches
        oo = T(np.broadcast_to(oa[a], (B, 3)).copy(), device)
        ref_any[a] = r.intersects_any(oo, T(db, device))
        ref_first[a] = r.intersects_first(oo, T(db, device))
    assert 0.05 < float(torch.stack(list(ref_any.values())).float().mean()) < 0.95          # a real mix of hits and misses
    got = r.intersects_any(o_t, d_t)
    assert got.shape == (A, B) and got.dtype == torch.bool
    for a in rows:
        assert torch.equal(got[a], ref_any[a]), f"intersects_any, row {a} (flat index {a * B})"
    # every row, against the row's own small batch, for a stride of rows: 128 more checks spread over the whole range
    for a in range(37, A, A // 128):
        oo = T(np.broadcast_to(oa[a], (B, 3)).copy(), device)
        assert torch.equal(got[a], r.intersects_any(oo, T(db, device))), f"intersects_any, row {a}"
    del got
    got = r.intersects_first(o_t, d_t)
    assert got.shape == (A, B) and got.dtype == torch.int32
    for a in rows:
        assert torch.equal(got[a], ref_first[a]), f"intersects_first, row {a} (flat index {a * B})"
    del got
    torch.cuda.empty_cache()


def test_queries_that_return_ray_indices_refuse_what_int32_cannot_index(device):
    """ray_idx is int32 by API (ray_optix.py:143-144, ray.cpp:352): intersects_location, intersects_id and
    intersects_closest(stream_compaction=True) raise ValueError at 2^31 rays and more -- before anything is traced or
    allocated -- instead of returning wrapped indices; one ray fewer is accepted (not run here: 56 GB of outputs)."""
    v, f = W.icosphere(2)
    r = make(v, f, device)
    o1 = torch.zeros(1, 1, 3, dtype=torch.float32, device=device)
    d1 = torch.tensor([[[0.0, 0.0, -1.0]]], dtype=torch.float32, device=device)
    big_o, big_d = o1.expand(1 << 16, 1 << 15, 3), d1.expand(1 << 16, 1 << 15, 3)        # 2^31 rays, 12 bytes of memory
    for call in (lambda: r.intersects_location(big_o, big_d),
                 lambda: r.intersects_id(big_o, big_d),
                 lambda: r.intersects_id(big_o, big_d, multiple_hits=False),
                 lambda: r.intersects_closest(big_o, big_d, stream_compaction=True)):
        with pytest.raises(ValueError, match="int32 ray_idx"):
            call()
    import triro.backend.ops as hops
    hops._check_ray_idx_range((1 << 31) - 1, 0, "x")          # the largest batch that is accepted
    hops._check_ray_idx_range(1 << 30, (1 << 30) - 1, "x")
    with pytest.raises(ValueError):
        hops._check_ray_idx_range(1 << 30, 1 << 30, "x")      # a shard's ray_base counts


def test_rays_aimed_at_shared_edges_and_vertices_never_slip_through(device):
    """The contract is watertight (round 6): rays aimed EXACTLY (in float32) at points of the shared edges and at the
    vertices of a closed mesh -- 2 % of the vertex rays pass through their vertex exactly: every edge function of the fan
    is zero -- from eye points inside the mesh ALWAYS hit, whatever query and launch family; from outside they hit
    unless they graze the silhouette; everything agrees with the oracle bit for bit (the oracle's brute force on a
    sample, too) and, in the hit mask, with the independent float64 watertight reference up to the rays that pass
    through a vertex exactly (where the owner rule of the contract and a sheared test with a rounded quotient may
    differ).  From inside, every ray counts exactly ONE hit -- an edge or a vertex belongs to one triangle."""
    v, f = W.icosphere(5)
    v = W.displaced(v, seed=3, amplitude=0.08)
    r = make(v, f, device)
    rng = np.random.default_rng(21)
    tri = v[f]                                                     # [F, 3, 3]
    k = rng.integers(0, len(f), 300_000)
    s = rng.random(300_000).astype(np.float32)
    on_edge = (tri[k, 0] * (1 - s[:, None]) + tri[k, 1] * s[:, None]).astype(np.float32)      # points on edges (rounded)
    targets = np.concatenate([on_edge, v[rng.integers(0, len(v), 100_000)]]).astype(np.float32)
    n = len(targets)
    eye_out = (rng.standard_normal((n, 3)) * 0.3 + np.array([0.0, 0.0, 4.0])).astype(np.float32)
    eye_in = (rng.standard_normal((n, 3)) * 0.05).astype(np.float32)
    R = OracleIntersector(v, f, mode=1)
    B = OracleIntersector(v, f, mode=0)
    for eye in (eye_out, eye_in):
        d = (targets - eye).astype(np.float32)
        o_t, d_t = T(eye, device), T(d, device)
        hit, front, tri_i, loc, uv = r.intersects_closest(o_t, d_t)
        cnt = r.intersects_count(o_t, d_t)
        eh, ef, et, el, eu = R.intersects_closest(eye, d)
        assert np.array_equal(hit.cpu().numpy(), eh) and np.array_equal(tri_i.cpu().numpy(), et)
        assert np.array_equal(front.cpu().numpy(), ef)
        assert np.array_equal(loc.cpu().numpy(), el) and np.array_equal(uv.cpu().numpy(), eu)
        ec = R.intersects_count(eye, d)
        assert np.array_equal(cnt.cpu().numpy(), ec)
        assert torch.equal(r.intersects_any(o_t, d_t), hit) and torch.equal(r.intersects_first(o_t, d_t), tri_i)
        sub = np.concatenate([np.arange(0, 300_000, 600), np.arange(300_000, 400_000, 200)])      # brute force: 1 000 rays
        bh, _, bt, _, _ = B.intersects_closest(eye[sub], d[sub])
        assert np.array_equal(bh, eh[sub]) and np.array_equal(bt, et[sub])
        assert np.array_equal(B.intersects_count(eye[sub], d[sub]), ec[sub])
        if eye is eye_in:
            assert bool(hit.all()), f"{int((~hit).sum())} rays slipped out of a closed mesh"
            assert np.all(ec % 2 == 1)          # (through edges AND vertices: an odd number of crossings from inside -- one owner per edge)
        else:
            assert float(hit.float().mean()) > 0.99
            assert np.all(ec % 2 == 0)          # (... and an even number from outside, the rays through vertices included)
        wtri, wt, wcnt = R.watertight(R.anchor(eye, d), d)
        # (edge rays: the same hit mask; vertex rays: at a vertex of the SILHOUETTE the contract's owner rule says none or both,
        # the sheared test one -- a handful of the 2 000 rays that run through their vertex exactly)
        assert int(((wtri >= 0) != eh).sum()) <= 48 and int(((wtri >= 0) != eh)[:300_000].sum()) == 0


@pytest.mark.timeout(600)
def test_native_step_matches_the_python_pipeline_and_runs_on_rccl(device):
    """VERDICT r05 "next" #3: tr_sharded_closest_step (include/triro_rccl.h) -- one C call per pipelined step -- gives
    the bits of the plain call and of the Python pipeline on the destination's side of a pretended 4-rank world, and its
    transfers run on real RCCL (one rank playing all four through ncclSend / ncclRecv): tests/native_step_world1.py."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "native_step_world1.py")], capture_output=True, text=True, env=env, timeout=540)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.timeout(300)
def test_native_step_that_nobody_answers_is_given_up_not_waited_for(device):
    """The native rung's safety net (sharded.py: _native_watchdog / _native_drop, tr_comm_abort): a step whose sends are
    left out (LOOPBACK | TEST_DROP_SEND) either fails on the host (RCCL refuses the unmatched receive) or is ended by
    ncclCommAbort from the watchdog's thread; afterwards the rung is gone (exchange_mode != "native"), the process and the
    GPU are fine and the tracer still gives its bits.  tests/native_abort_world1.py (a child process, under a timeout)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "native_abort_world1.py")], capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def test_tmax_counts_from_the_origin_for_rays_that_would_be_anchored(device):
    """the far end of the reference's interval [0, 1e7] under ray anchoring (tests/test_oracle.py has the scene and the reasoning):
    the HIP path against the oracle, every query"""
    sq = lambda x: [[x, -4, -4], [x, 4, -4], [x, 0, 4]]  # noqa: E731
    v = np.array(sq(5.0e6) + sq(9.9e6) + sq(1.00005e7) + sq(1.0001e7), np.float32)
    f = np.arange(12, dtype=np.int32).reshape(4, 3)
    o = np.array([[0, 0, 0], [5.5e6, 0, 0], [9.95e6, 0, 0], [0, 0, 0], [0, 1, 0], [2.0e6, -1, 1]], np.float32)
    d = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0], [1, 0, 0], [1, 1e-7, 0]], np.float32)
    r = make(v, f, device)
    R = OracleIntersector(v, f, 1)
    ot, dt = T(o, device), T(d, device)
    cnt = r.intersects_count(ot, dt).cpu().numpy()
    assert cnt.tolist() == R.intersects_count(o, d).tolist() and cnt[:4].tolist() == [2, 3, 2, 4]
    got = [x.cpu().numpy() for x in r.intersects_closest(ot, dt)]
    for g, e in zip(got, R.intersects_closest(o, d)[:5]):
        assert np.array_equal(g, e, equal_nan=True)
    assert np.array_equal(r.intersects_any(ot, dt).cpu().numpy(), R.intersects_any(o, d))
    loc, ridx, tidx = r.intersects_location(ot, dt)
    el, er, et = R.intersects_location(o, d)
    assert np.array_equal(ridx.cpu().numpy(), er) and np.array_equal(tidx.cpu().numpy(), et) and np.array_equal(loc.cpu().numpy(), el)


def test_graph_replay_follows_a_refit_that_moves_the_bounds(device):
    """A launch captured in a HIP graph freezes its kernel arguments -- the grid frame of the mesh among them, which the
    grid nodes' decode AND the rays' anchor depend on.  Since round 6 the kernels read the frame from device memory
    (TR_VIEW_LIVE), which refit / update_raw keep current: a replay after a refit that GROWS the mesh gives the new
    mesh's answers bit for bit -- stealing closest launch on the grid nodes, count, and the list query."""
    v, f = W.icosphere(5)
    v = W.displaced(v, seed=2, amplitude=0.05)
    r = make(v, f, device)
    o, d = W.pinhole_grid(256, 192, distance=3.5)
    ot, dt = T(np.ascontiguousarray(o), device), T(d, device)
    gs = torch.cuda.Stream(device)
    gs.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(gs):
        for _ in range(4):
            r.intersects_closest(ot, dt)
            r.intersects_count(ot, dt)
    torch.cuda.current_stream(device).wait_stream(gs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        out = r.intersects_closest(ot, dt)
        cnt = r.intersects_count(ot, dt)
    v2 = (W.displaced(v, seed=9, amplitude=0.08) * np.float32(1.35) + np.float32([0.2, -0.1, 0.15])).astype(np.float32)      # other bounds, other frame
    for vv in (v, v2, v):
        r.refit(T(vv, device))
        graph.replay()
        torch.cuda.synchronize()
        poison.assert_written(*out, cnt, what="graph replay after a refit")
        R = OracleIntersector(vv, f, mode=1)
        eh, ef, et, el, eu = R.intersects_closest(o, d)
        assert np.array_equal(out[0].cpu().numpy(), eh) and np.array_equal(out[2].cpu().numpy(), et)
        assert np.array_equal(out[3].cpu().numpy(), el) and np.array_equal(out[4].cpu().numpy(), eu)
        assert np.array_equal(cnt.cpu().numpy(), R.intersects_count(o, d))


def test_launch_policy_boundaries_come_from_the_device(device):
    """VERDICT r05 "next" #6: XCD count, L2 size and resident waves per CU are read from the device (attribute query,
    occupancy calculator), and the ray-count boundaries between the launch shapes are multiples of the device's resident
    lanes.  On an MI355X in SPX mode they are the values every profile of rounds 2-5 was taken with."""
    import triro.backend.ops as hops
    t = hops.device_topology(0)
    assert t["num_cus"] > 0 and t["num_xcd"] in (1, 2, 4, 8) and t["waves_per_cu"] >= 8
    assert t["resident_lanes"] == t["num_cus"] * t["waves_per_cu"] * 64
    assert t["steal_max_rays"] == t["resident_lanes"] * 32 // 3 and t["wide_min_rays"] == t["resident_lanes"] * 64 // 3
    assert t["count_stream_min_rays"] == t["resident_lanes"] * 128 // 3
    if t["num_cus"] == 256:          # the whole chip
        assert t["num_xcd"] == 8 and t["waves_per_cu"] == 24
        assert (t["steal_max_rays"], t["wide_min_rays"], t["count_stream_min_rays"]) == (1 << 22, 1 << 23, 1 << 24)
