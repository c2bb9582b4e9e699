#!/usr/bin/env python3
"""Headline benchmark: Mrays/s closest-hit, 1M-tri mesh, 1024^2 ray batch (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c5i|c5ii] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A step = one `RayMeshIntersector.intersects_closest` call (the reference's timed call,
test/performance_test.py:54-57); rays and BVH are resident in HBM before the timed region.

Workloads
  c5i  (default, the metric's config): one 1024x1024 pinhole ray batch per GPU against the
       1 310 720-triangle headline mesh.  N > 1: every rank owns a BVH replica and
       the job is N such batches per step -> "scaling": "weak" (the stack [N x 1024, 1024] is cut into row
       bands: even ones with `--dst-share 1`; by default rank 0, which also finishes everybody else's rays,
       takes a narrower band and the peers wider ones -- same total); `--scaling strong` cuts ONE 1024^2
       batch into N row bands instead.  For N > 1 the results are gathered to rank 0 INSIDE the timed region
       ("all outputs resident on the caller's GPU"; `--no-gather` leaves them in place):
       rank 0 holds the rays of the whole batch (as the reference's caller does), the peers send 4-byte
       records -- the arena slot of each ray's nearest triangle -- over RCCL and rank 0 finishes those rays
       from (ray, slot) (`--records packed`: 12-byte {slot, u, v} records, rank 0 needs no rays;
       triro.ray.sharded), step k's exchange overlapping step k+1's trace.
  c5ii (BASELINE.json config 5): ONE batch of 100 000 000 hash rays (seed 99) split into N
       contiguous shards (triro.ray.sharded.shard_bounds), BVH replicated, results gathered to
       rank 0 INSIDE the timed region -> "scaling": "strong".

A plain run sets up, warms up, times exactly `--steps` steps and prints the line (metric, value, unit,
ms_per_step, config).  `--full` adds what takes runs or checks of its own: the `--warmup`-exactly protocol
figure, the roofline (HIP event pairs), `verified` (last timed step == cold first call), the parity error
bars, the companions (cold / first launch / moving camera / reference shape / pipelined / traversal; the
other scaling for N > 1) and the CPU baseline.  `--dump-outputs DIR` writes the last timed step's outputs
(rank 0's) as DIR/<name>.npy.

`--gpus N` with N > 1 and no launcher environment: this process never touches the GPU; it checks
that N devices are visible, starts N ranks with `python -m torch.distributed.run` (one per GPU,
RCCL) as a child process and relays rank 0's JSON line.  Under a launcher (RANK/WORLD_SIZE set)
it is one of those ranks.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "trimesh-ray-optix_amd"))

HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E ~8 TB/s spec (6.29 TB/s achievable)
BYTES_PER_RAY_CLOSEST = 50      # 24 B in + 26 B out
# --dst-share auto: what finishing one ray somebody else traced costs the destination rank, in units of tracing one ray
# (expansion alone / trace, measured on one MI355X: profiles/r04_emulate_records.jsonl, + a margin for the receive):
# c5i: 0.2 ms per M pinhole rays against 0.0127 (4-byte records + the ray) / 0.0092 (12-byte records) ms per M records;
# c5ii: 0.137 ms per M incoherent rays against 0.0150 / 0.0132
# (round 5: the trace got 7 % faster -- the fused box test --, the expansion did not: the ratios moved accordingly, re-derived
# from the emulated rank-0 / peer steps of profiles/r05_emulate_final.jsonl and r05_emulate_records.jsonl; c5ii / slot once more after
# the streaming boundary of large meshes moved to 2.75 M rays: rank 0's 2.4 M incoherent rays then take the direct launch, which does not
# overlap with the expansion on the side stream -- a smaller shard (1.9 M rays) balances the step again: r05_emulate_final_tree.jsonl;
# with the early stealing of unrelated rays that shard's trace takes 0.33 ms: rank 0 1.68 ms, a peer 1.78 -- 6.6x / 6.2x)
# (round 6: finishing a ray from its slot now computes its barycentrics in float64 -- the expansion of 7.9 M records 0.093 -> 0.100 ms --
# and the trace changed with the contract: c5i / slot re-derived from profiles/r06_emulate_shares.txt -- share 0.39 / 0.30 / 0.22 / 0.15 ->
# rank 0 0.231 / 0.222 / 0.213 / 0.230 ms against a peer's 0.202-0.205: 0.22, i.e. rho = 0.115; c5ii / slot unchanged: rank 0 1.79-1.82 ms
# against a peer's 1.82-1.86 in six processes)
AUTO_RHO = {("c5i", "slot"): 0.115, ("c5i", "packed"): 0.064, ("c5ii", "slot"): 0.125, ("c5ii", "packed"): 0.101}


def resolve_share(args, world):
    """--dst-share as a number (None = even shards)"""
    share = args.dst_share
    if world < 2 or share is None:
        return None
    if share == "auto":
        from triro.ray.sharded import auto_dst_share
        return round(auto_dst_share(world, AUTO_RHO[(args.workload, args.records)]), 3)
    share = float(share)
    return None if share >= 1.0 else share
C5II_RAYS = 100_000_000


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", choices=["c5i", "c5ii"], default="c5i")
    ap.add_argument("--subdiv", type=int, default=8, help="icosphere subdivisions (8 = 1 310 720 tris)")
    ap.add_argument("--res", type=int, default=1024, help="c5i: ray grid is res x res")
    ap.add_argument("--rays", choices=["pinhole", "hash"], default="pinhole", help="c5i ray family")
    ap.add_argument("--total-rays", type=int, default=C5II_RAYS, help="c5ii: size of the one sharded batch")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="c5i with N > 1: weak = one res x res batch per GPU (default), strong = ONE res x res batch cut into N row bands")
    ap.add_argument("--gather", action="store_true", help="(default for N > 1) results are gathered to rank 0 inside the timed region")
    ap.add_argument("--no-gather", action="store_true", help="N > 1: leave every rank's results on its own GPU (no exchange)")
    ap.add_argument("--chunks", type=int, default=1,
                    help="N > 1: chunks per shard of the trace / gather pipeline (0 = the library's rule for ONE call, "
                         "triro.ray.sharded.default_chunks: ~3 M rays per chunk so that the exchange overlaps the trace inside "
                         "the call).  Default 1: bench.py keeps two steps in flight, step k's exchange already overlaps step "
                         "k+1's trace, and whole shards trace faster than pieces (emulated c5ii at 8 ranks: 1.91 against 2.47 ms)")
    ap.add_argument("--force-gather", action="store_true",
                    help="test aid: run the N > 1 result pipeline (packed trace, RCCL exchange, expansion on a side stream, "
                         "double buffering) in a communicator of ONE rank -- what a single-GPU box can check of it; the line is labelled")
    ap.add_argument("--min-warmup-ms", type=float, default=50.0, help="keep warming up until this much time has passed")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-companions", action="store_true", help="--full: skip the cold / moving-camera / gather-ceiling companions")
    ap.add_argument("--opt", action="append", default=[], help="library option name=value (tr_set_option)")
    ap.add_argument("--stats", action="store_true", help="also print traversal counters (diagnostic kernel)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="gloo = FUNCTIONAL runs (measure nothing): with --stub the launcher/sharding self-test on CPU; without, "
                         "the real tracer with N ranks sharing the visible GPU(s), device tensors staged through the host")
    ap.add_argument("--dst-share", default="auto",
                    help="N > 1: the destination rank of the gather (it also finishes everybody else's rays) traces this fraction "
                         "of an even shard: a float (1 = even shards), or 'auto' (default) = triro.ray.sharded.auto_dst_share with "
                         "the measured cost ratio of the workload and record form (AUTO_RHO).  Weak scaling: the stack of N "
                         "batches is cut at whole rows, rank 0 takes fewer of them")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="ONE GPU: the destination rank's side of an N-rank run (own trace + N-1 chunks of records arriving as "
                         "device copies + their expansion; triro.ray.sharded.EmulatedWorld) -- a bound, not a measurement")
    ap.add_argument("--arrival-priority", action="store_true", help="--emulate-world: expansion stream at high priority")
    ap.add_argument("--trace-priority", action="store_true",
                    help="N > 1 / --emulate-world: the step loop (the traces) runs on a HIGH-priority stream, so that the expansion on "
                         "the side stream only takes the wave slots the trace leaves free")
    ap.add_argument("--event-stride", type=int, default=0,
                    help="bracket every N-th timed step with a HIP event pair for the roofline's kernel time (0 = 5 ... 64 samples "
                         "over the timed region, an odd stride: 20 steps -> every 3rd, 1000 steps -> every 15th; measured: pairs around EVERY step "
                         "cost the wall clock 7.5 us of every 205)")
    ap.add_argument("--records", choices=["slot", "packed"], default="slot",
                    help="N > 1, closest-hit gather: 'slot' = 4-byte records, rank 0 holds the rays of the whole batch and "
                         "finishes the query from (ray, slot); 'packed' = 12-byte {slot, u, v} records, rank 0 needs no rays")
    ap.add_argument("--arrival", choices=["copy", "none"], default="copy",
                    help="--emulate-world: how the peers' records arrive: device copies on a copy stream (pessimistic: blit "
                         "kernels) or not at all (they are simply there: expansion cost only)")
    ap.add_argument("--exchange", choices=["native", "slot", "packed", "dense", "padded", "staged"], default=None,
                    help="N > 1: the rung of the exchange ladder to start from (default: slot, or packed with --records packed); the "
                         "preflight steps down from there (triro.ray.sharded.LADDER)")
    ap.add_argument("--no-preflight", action="store_true", help="N > 1: skip the checked small batch in front of the run")
    ap.add_argument("--stub", default=None, help="module:factory of a stand-in tracer (only with --backend gloo; tests)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline figure (protocol figure, roofline, verified, "
                         "parity, companions, CPU baseline); a plain run only times --steps steps")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32 / float64; a fixed seeded "
                         "sample of the rays when they would exceed 64 MB, with ray_index.npy)")
    return ap.parse_args(argv)


DUMP_BUDGET_BYTES = 64_000_000
DUMP_NAMES = ("hit", "front", "tri_idx", "loc", "uv")


def dump_outputs(path, out):
    """intersects_closest's five outputs as path/<name>.npy: bool -> float32, integers -> float64 (exact), floats keep
    their precision.  Above DUMP_BUDGET_BYTES a fixed sample of rays (seed 0, sorted) is written, with its indices."""
    import numpy as np
    import torch
    if out is None or out[0] is None:
        raise SystemExit("bench.py --dump-outputs: the timed path returned no outputs on this rank")
    os.makedirs(path, exist_ok=True)
    batch = tuple(out[0].shape)
    n = out[0].numel()
    flat = [x.reshape(n, *x.shape[len(batch):]) for x in out]
    dts = [np.float32 if x.dtype == torch.bool else np.float64 if not x.dtype.is_floating_point else
           (np.float64 if x.dtype == torch.float64 else np.float32) for x in flat]
    per_ray = sum(np.dtype(dt).itemsize * (x[0].numel() if n else 1) for x, dt in zip(flat, dts))
    idx = None
    if n * per_ray + 1024 > DUMP_BUDGET_BYTES:
        k = (DUMP_BUDGET_BYTES - 1024) // (per_ray + 8)   # (+ 8: the float64 index of each sampled ray; 1024: the .npy headers)
        idx = np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
        np.save(os.path.join(path, "ray_index.npy"), idx.astype(np.float64))
        sel = torch.from_numpy(idx).to(flat[0].device)
        flat = [x.index_select(0, sel) for x in flat]
    for name, x, dt in zip(DUMP_NAMES, flat, dts):
        a = x.cpu().numpy().astype(dt)
        np.save(os.path.join(path, f"{name}.npy"), a if idx is not None else a.reshape(*batch, *a.shape[1:]))


# ---- launcher --------------------------------------------------------------------------------
def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(args, argv) -> int:
    """Parent of an N-rank run.  Touches no GPU (device_count() does not initialise HIP on this
    image); the ranks are fresh child processes started by torch.distributed.run."""
    n = args.gpus
    if args.backend == "nccl":
        import torch
        have = torch.cuda.device_count()
        if have < n:
            print(f"bench.py: --gpus {n} needs {n} visible GPUs, this node shows {have}; "
                  f"refusing to report an {n}-GPU number from fewer devices", file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (RCCL across processes on this driver)
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, text=True, env=env)
    line = None
    for ln in proc.stdout:
        if ln.startswith('{"metric"'):
            line = ln.strip()
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if rc != 0:
        print(f"bench.py: the {n}-rank run failed (exit code {rc})", file=sys.stderr)
        return rc
    if line is None:
        print("bench.py: rank 0 printed no result line", file=sys.stderr)
        return 1
    print(line, flush=True)
    return 0


# ---- CPU baseline ----------------------------------------------------------------------------
def cpu_baseline(v, f, o, d, budget_s=20.0):
    """The oracle's BVH mode ("port": our CPU restatement, NOT Embree -- trimesh/pyembree are
    not installed in this image) on the host cores, same mesh, same rays, bounded time.  Only the C
    entry point is inside the clock (OracleIntersector.closest_timed: OpenMP, dynamic schedule over
    rays, outputs first touched by the workers); a 1-thread and an N-thread figure with N = the CPUs
    this process may really use (affinity mask cut by the cgroup quota -- a box that shows 128 cores
    to a container that is allowed a few would otherwise be timed oversubscribed)."""
    import numpy as np
    from oracle.oracle import OracleIntersector, num_threads, usable_cpus
    embree = None
    try:   # trimesh + Embree if the GPU box happens to have them
        import trimesh
        import embreex  # noqa: F401
        m = trimesh.Trimesh(vertices=v, faces=f, process=False)
        oo = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        dd = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        t0 = time.perf_counter()
        m.ray.intersects_location(oo, dd, multiple_hits=False)   # test/performance_test.py:75
        el = time.perf_counter() - t0
        embree = {"value": round(len(oo) / el / 1e6, 3), "unit": "Mrays/s", "cores": 1, "kind": "reference",
                  "sample": f"trimesh+embree mesh.ray.intersects_location(multiple_hits=False), {len(oo)} rays, 1 pass"}
    except Exception:
        embree = None
    R = OracleIntersector(v, f, mode=1)
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    ncpu = min(usable_cpus(), num_threads())
    R.closest_timed(o[:4096], d[:4096], ncpu)      # page in, start the thread team
    # one thread: the same rays (all of them when that fits a third of the budget, else leading rows)
    n1 = len(o)
    t_probe = R.closest_timed(o[:1 << 14], d[:1 << 14], 1)
    est = t_probe * len(o) / (1 << 14)
    if est > budget_s / 3:
        n1 = max(1 << 14, int(len(o) * (budget_s / 3) / est))
    t1 = R.closest_timed(o[:n1], d[:n1], 1)
    one = n1 / t1 / 1e6
    # N threads: passes back to back inside ONE closest_timed call (the thread team stays awake between them; in a
    # VM waking seven idle vCPUs per call costs more than tracing a million rays)
    t_warm = R.closest_timed(o, d, ncpu)
    t_warm = min(t_warm, R.closest_timed(o, d, ncpu))
    passes = int(max(1, min(40, (budget_s * 2 / 3 - 2 * t_warm) / max(t_warm, 1e-3))))
    el = R.closest_timed(o, d, ncpu, passes=passes)
    many = len(o) * passes / el / 1e6
    res = {"value": round(many, 3), "unit": "Mrays/s", "cores": ncpu, "kind": "port",
           "threads_1": {"value": round(one, 3), "rays": n1},
           "parallel_efficiency": round(many / one / ncpu, 3),
           "visible_cpus": os.cpu_count(),
           "sample": f"{len(o)}-ray sample of the workload x {passes} passes on {ncpu} threads (the CPUs this process may use; "
                     f"{os.cpu_count()} visible), {n1} rays on 1 thread; oracle median-split BVH + contract arithmetic, only the "
                     f"C entry point inside the clock (OpenMP, dynamic schedule over rays)"}
    if embree is not None:
        res = dict(embree, port=res)
    return res


# ---- the parity error bar (static: measured by scripts/watertight_bound.py, kept under profiles/) ---------------
def parity_error_bars():
    """The contract against an independent watertight reference (OptiX's built-in triangle test is closed and nothing of the
    reference runs here: parity is UNPINNED at the bit level).  Per BASELINE config at full size: the rays
    whose hit mask / triangle index / hit count differ from the published form of the Woop-Benthin-Wald test evaluated in
    float64 on the same (anchored) float32 rays, and the largest differences of what the API returns -- uv, loc -- and of
    the distance on the same triangle (profiles/r06_watertight_bound.jsonl, scripts/watertight_bound.py --full; the GPU
    outputs are the contract's bit for bit: tests/test_watertight.py, tests/test_gpu_configs.py)."""
    out = {"pinned_bit_exact_against_reference": False,
           "note": "bit-exact against the CPU oracle (every BASELINE config, full size, incl. loc / uv); the contract is watertight "
                   "since round 6 (float32 Moller-Trumbore where a proven error bound lets it decide, float64 edge functions "
                   "elsewhere, barycentrics from float64): against an independent float64 watertight test the differences below; "
                   "the reference's own arithmetic (OptiX) is closed and unbuildable here", "configs": {}}
    for name in ("r06_watertight_bound.jsonl", "r05_watertight_bound.jsonl"):
        p = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(p):
            continue
        try:
            for ln in open(p):
                ln = ln.strip()
                if not ln.startswith("{"):
                    continue
                j = json.loads(ln)
                n = max(int(j.get("rays", 0)), 1)
                key = j.get("config") or j.get("name")
                if not key or key in out["configs"]:
                    continue
                out["configs"][key] = {
                    "rays": int(j.get("rays", 0)),
                    "hit_mask_differs": j.get("only_contract", 0) + j.get("only_watertight", 0),
                    "tri_idx_differs": j.get("tri_diff_same_t", 0) + j.get("tri_diff_other", 0),
                    "count_differs": j.get("count_diff", 0),
                    "max_rel_t_diff_same_tri": j.get("max_rel_t_diff_same_tri"),
                    "max_rel_uv_diff": j.get("max_rel_uv_diff"), "max_abs_uv_diff": j.get("max_abs_uv_diff"),
                    "max_rel_loc_diff": j.get("max_rel_loc_diff"), "max_abs_loc_diff": j.get("max_abs_loc_diff")}
            out["source"] = "profiles/" + name
        except Exception as exc:      # noqa: BLE001
            out["error"] = str(exc)
        break
    return out


# ---- one rank --------------------------------------------------------------------------------
def rotate_y(x, deg):
    import numpy as np
    a = np.radians(deg)
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    out = x.copy()
    out[..., 0] = c * x[..., 0] + s * x[..., 2]
    out[..., 2] = -s * x[..., 0] + c * x[..., 2]
    return out


def stacked_rows(img, world_rows, a, z, roll=7):
    """rows [a, z) of the weak-scaling batch: `world` images stacked, image k = `img` rolled by k * roll rows
    (every rank's camera sees the same scene, shifted, so the shards differ).  img: [res, W, 3]."""
    import numpy as np
    res = img.shape[0]
    parts = []
    g = a
    while g < z:
        k, j = divmod(g, res)
        take = min(res - j, z - g)
        parts.append(np.roll(img, k * roll, axis=0)[j:j + take])
        g += take
    return np.concatenate(parts, axis=0) if parts else img[:0]


def build_workload(args, world, rank, dev, v, rad, share, workload, scaling, res, total_rays):
    """The rays of one benchmark configuration as THIS rank holds them: its shard of the job (`origins`, `dirs`), the
    bounds of everybody's shard, the shape of the gathered batch, and -- on request, for rank 0 -- the rays of the whole
    batch (`all_rays()`: what the caller of the reference's API holds, and what 4-byte records are finished from).
    workload c5i: scaling 'weak' = `world` batches of res x res rays stacked ([world * res, res], cut into row bands),
    'strong' = ONE res x res batch in `world` row bands; workload c5ii: ONE batch of total_rays hash rays."""
    import numpy as np
    import torch
    import workloads as W
    from triro.ray.sharded import shard_bounds, dst_bounds
    pinhole = args.rays == "pinhole" and workload == "c5i"
    strong_c5i = workload == "c5i" and scaling == "strong" and world > 1
    wl = {"workload": workload, "scaling": "strong" if (strong_c5i or workload == "c5ii") else "weak", "res": res,
          "strong_c5i": strong_c5i, "pinhole": pinhole, "o_np": None, "d_np": None, "bshape": None, "row_quantum": None}

    def split_batch(n_rays, quantum):
        if share is not None and share < 1.0 and world > 1:
            return dst_bounds(n_rays, world, 0, share, quantum)
        return [shard_bounds(n_rays, world, k) for k in range(world)]

    def hash_rays(a, z):
        lo, hi = v.min(0) * 1.5, v.max(0) * 1.5
        parts_o, parts_d = [], []
        for s in range(a, z, 1 << 23):                       # bounded temporaries
            po, pd = W.hash_rays_torch(min(1 << 23, z - s), 99, lo, hi, start=s, device=dev)
            parts_o.append(po)
            parts_d.append(pd)
        if not parts_o:
            return torch.zeros((0, 3), device=dev), torch.zeros((0, 3), device=dev)
        return (parts_o[0], parts_d[0]) if len(parts_o) == 1 else (torch.cat(parts_o), torch.cat(parts_d))

    if workload == "c5i":
        n_total = res * res * (1 if strong_c5i else world)
        bounds_all = split_batch(n_total, res if pinhole else 1)
        lo_ray, hi_ray = bounds_all[rank]
        if pinhole:
            o_img, d_img = W.pinhole_grid(res, res, distance=2.5 * rad)
            o_full = np.broadcast_to(o_img, d_img.shape)
            rows_ok = all(a % res == 0 and z % res == 0 for a, z in bounds_all)       # every rank decides alike
            if strong_c5i:
                wl["bshape"] = (res, res)
                if rows_ok and hi_ray > lo_ray:
                    o_np, d_np = o_full[lo_ray // res:hi_ray // res], d_img[lo_ray // res:hi_ray // res]
                else:
                    o_np, d_np = o_full.reshape(-1, 3)[lo_ray:hi_ray], d_img.reshape(-1, 3)[lo_ray:hi_ray]
            else:
                # weak: image k of the stack = the same camera, rolled by k x 7 rows, so that the shards differ
                wl["bshape"] = (world * res, res)
                if rows_ok:
                    d_np = stacked_rows(d_img, world, lo_ray // res, hi_ray // res)
                    o_np = stacked_rows(o_full, world, lo_ray // res, hi_ray // res, roll=0)
                else:
                    d_np = stacked_rows(d_img, world, 0, world * res).reshape(-1, 3)[lo_ray:hi_ray]
                    o_np = stacked_rows(o_full, world, 0, world * res, roll=0).reshape(-1, 3)[lo_ray:hi_ray]
            origins = torch.from_numpy(np.ascontiguousarray(o_np)).to(dev)
            dirs = torch.from_numpy(np.ascontiguousarray(d_np)).to(dev)
            wl["o_np"], wl["d_np"] = o_np, d_np
            if rows_ok:
                wl["row_quantum"] = res

            def all_rays():
                if strong_c5i:
                    ao, ad = o_full, d_img
                else:
                    ao = stacked_rows(o_full, world, 0, world * res, roll=0)
                    ad = stacked_rows(d_img, world, 0, world * res)
                t = (torch.from_numpy(np.ascontiguousarray(ao)).to(dev), torch.from_numpy(np.ascontiguousarray(ad)).to(dev))
                return t if rows_ok else (t[0].reshape(-1, 3), t[1].reshape(-1, 3))
        else:
            wl["bshape"] = (n_total,)
            origins, dirs = hash_rays(lo_ray, hi_ray)

            def all_rays():
                return hash_rays(0, n_total)
    else:
        n_total = total_rays
        bounds_all = split_batch(n_total, 1)
        lo_ray, hi_ray = bounds_all[rank]
        wl["bshape"] = (n_total,)
        origins, dirs = hash_rays(lo_ray, hi_ray)

        def all_rays():
            return hash_rays(0, n_total)
    wl.update(origins=origins, dirs=dirs, n=hi_ray - lo_ray, n_total=n_total, bounds_all=bounds_all, all_rays=all_rays)
    return wl


def run_rank(args):
    import numpy as np
    import torch
    import workloads as W
    from triro.ray.sharded import ShardedRayMeshIntersector, LADDER

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist_on = "RANK" in os.environ and "WORLD_SIZE" in os.environ   # launched by torch.distributed.run
    gloo = args.backend == "gloo"
    stub = bool(args.stub)
    if stub:
        if not gloo:
            raise SystemExit("--stub is only accepted with --backend gloo (a stand-in tracer is never measured)")
        dev = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
        # gloo without a stub: a functional run of the real tracer; the ranks may share GPUs
        local_dev = local_rank % torch.cuda.device_count() if gloo else local_rank
        torch.cuda.set_device(local_dev)
        dev = torch.device("cuda", local_dev)
    dist = None
    ctrl = None
    nccl_ok = True
    if dist_on:
        import datetime
        import torch.distributed as dist
        if gloo:
            dist.init_process_group("gloo")
        else:
            # (a collective that never completes ends the run after ten minutes instead of never; no device_id: the RCCL
            # communicator is created by the first collective -- the smoke test below --, where a failure can be caught)
            dist.init_process_group("nccl", timeout=datetime.timedelta(minutes=10))
        world = dist.get_world_size()          # the ranks the communicator actually has
        if world != args.gpus:
            print(f"bench.py: --gpus {args.gpus} but the launcher started {world} ranks; reporting n_gpus={world}",
                  file=sys.stderr)
        # a gloo CONTROL group beside the RCCL communicator: verdicts of the preflight travel on it (they must not
        # depend on the transport under test), and on the last rung of the exchange ladder the results themselves
        if not gloo and (world > 1 or args.force_gather):
            try:
                ctrl = dist.new_group(backend="gloo", timeout=datetime.timedelta(minutes=10))
            except Exception as exc:      # noqa: BLE001
                print(f"bench.py: no gloo control group ({exc}); the preflight's verdicts use the RCCL communicator", file=sys.stderr)
                ctrl = None
        # RCCL smoke test: one 4-byte all-reduce + a device synchronisation, verdict agreed on the control group.  If the
        # communicator cannot even do that on some rank, the whole run -- barriers, timing reduction, data -- moves to the
        # gloo group (exchange mode "staged"): a slow line instead of no line.
        if not gloo and ctrl is not None:
            ok_ = True
            try:
                t_ = torch.ones(1, dtype=torch.int32, device=dev)
                dist.all_reduce(t_)
                torch.cuda.synchronize()
                ok_ = int(t_.item()) == world
            except Exception as exc:      # noqa: BLE001
                ok_ = False
                print(f"bench.py: rank {rank}: RCCL smoke test failed: {type(exc).__name__}: {exc}", file=sys.stderr)
            v_ = torch.tensor([1 if ok_ else 0], dtype=torch.int32)
            dist.all_reduce(v_, op=dist.ReduceOp.MIN, group=ctrl)
            nccl_ok = bool(int(v_.item()) == 1)
            if not nccl_ok and rank == 0:
                print("bench.py: RCCL is unusable on this node: the run falls back to gloo (results staged through the host)", file=sys.stderr)
    elif args.gpus != 1:
        raise SystemExit("internal error: run_rank with --gpus > 1 outside a launcher")

    def sync():
        if not stub:
            torch.cuda.synchronize()

    if stub:
        import importlib
        modname, fname = args.stub.split(":")
        factory = getattr(importlib.import_module(modname), fname)
        hops = None
    else:
        import triro.backend.ops as hops
        from triro.ray.ray_optix import RayMeshIntersector
        for kv in args.opt:
            k, v_ = kv.split("=", 1)
            hops.set_option(k, int(v_))

    # ---- workload (synthetic, deterministic) -------------------------------------------------
    v, f = W.headline_mesh(args.subdiv)
    rad = float(np.linalg.norm(v, axis=1).max())
    # with --dst-share rank 0 (the destination of the gather, which also finishes everybody else's rays) takes a smaller shard
    share = resolve_share(args, world)
    wl = build_workload(args, world, rank, dev, v, rad, share, args.workload, args.scaling, args.res, args.total_rays)
    strong_c5i = wl["strong_c5i"]
    origins, dirs, n, n_total, bounds_all = wl["origins"], wl["dirs"], wl["n"], wl["n_total"], wl["bounds_all"]
    o_np, d_np = wl["o_np"], wl["d_np"]
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    sync()
    t0 = time.perf_counter()
    r = factory(v, f, dev) if stub else RayMeshIntersector(vertices=vt, faces=ft)
    sync()
    build_ms = (time.perf_counter() - t0) * 1e3
    info = r.bvh_info()

    gather_on = dist_on and (world > 1 or args.force_gather) and not args.no_gather
    S = ShardedRayMeshIntersector(r, force_collectives=args.force_gather, dst_share=share, ctrl_group=ctrl) if dist_on else None
    if S is not None and not nccl_ok:
        S.set_exchange_mode("staged")
    elif S is not None and args.exchange:
        S.set_exchange_mode(args.exchange)
    elif S is not None and args.records == "packed" and S.exchange_mode == "slot":
        S.set_exchange_mode("packed")
    elif (S is not None and world > 1 and not stub and not args.no_preflight and os.environ.get("TRIRO_NATIVE_STEP", "1") != "0"
          and S.native_available()):
        # Round 6: start on the top rung -- the whole step as ONE C call (60 us of host time against 150-390 for the
        # Python driver, which is host-bound on a 0.2-ms step: profiles/r06_emulate.jsonl).  Only behind the preflight:
        # it checks the rung's bits, and its watchdog aborts the rung's own communicator when nobody answers.
        S.set_exchange_mode("native")

    class Runner:
        """one workload through the exchange mode S is in: step() / drain() as the timed loop calls them"""

        def __init__(self, w, chunks):
            self.w, self.chunks, self.pending = w, chunks, []
            self.lead = w["origins"].dim() - 1
            self.packed_ok = gather_on and S._can_pack()       # the real tracer; stand-ins take the per-output exchange
            # 4-byte records: rank 0 (the caller of the reference's API: it hands in the whole batch) holds ALL rays and
            # finishes the peers' rays from (ray, slot); resident before the clock starts like every other input
            self.slot_rec = self.packed_ok and S.exchange_mode in ("slot", "native")
            self.all_rays = w["all_rays"]() if (self.slot_rec and rank == 0) else None

        def step(self):
            """one call; with the gather on, the pipeline is double-buffered: step k's exchange + expansion
            (RCCL stream, side stream) overlap step k+1's trace, and step() hands back step k-1's outputs"""
            w = self.w
            if not gather_on:
                return r.intersects_closest(w["origins"], w["dirs"])
            if not self.packed_ok:
                out = r.intersects_closest(w["origins"], w["dirs"])
                # chunks land in slices of rank 0's full-size outputs (c5ii / strong: ONE batch; weak: world x n rows)
                res_ = [S._gather_fixed(x.reshape(w["n"], *x.shape[self.lead:]), w["n_total"], 0, w["bounds_all"]) for x in out]
                if res_[0] is None:
                    return None
                b = w["bshape"]
                return [res_[0].view(b), res_[1].view(b), res_[2].view(b), res_[3].view(*b, 3), res_[4].view(*b, 2)]
            if self.slot_rec and S.exchange_mode == "native":       # the same step as ONE C call (include/triro_rccl.h)
                self.pending.append(S.closest_of_shard_native(w["origins"], w["dirs"], w["n_total"], batch_shape=w["bshape"], dst=0,
                                                              chunks=self.chunks or None, bounds=w["bounds_all"],
                                                              row_quantum=w["row_quantum"], all_rays=self.all_rays))
                return self.pending.pop(0).wait() if len(self.pending) > 1 else None
            self.pending.append(S.closest_of_shard_async(w["origins"], w["dirs"], w["n_total"], batch_shape=w["bshape"], dst=0,
                                                         chunks=self.chunks or None, bounds=w["bounds_all"],
                                                         row_quantum=w["row_quantum"], records="slot" if self.slot_rec else "packed",
                                                         all_rays=self.all_rays))
            return self.pending.pop(0).wait() if len(self.pending) > 1 else None

        def drain(self):
            out = None
            while self.pending:
                out = self.pending.pop(0).wait()
            return out

    def barrier():
        if dist_on:
            dist.barrier(group=None if nccl_ok else ctrl)
        sync()

    def event_pair():
        if stub:
            return None
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed_steps(count, fn):
        """`count` calls of fn, each bracketed by a pair of events recorded on the stream the
        kernels are launched on (torch's current stream); returns per-call GPU milliseconds."""
        ev = [event_pair() for _ in range(count)]
        for k in range(count):
            if ev[k]:
                ev[k][0].record()
            fn(k)
            if ev[k]:
                ev[k][1].record()
        sync()
        return [a.elapsed_time(b) for a, b in ev] if not stub else [0.0] * count

    def max_over_ranks(x):
        cpu_ = gloo or not nccl_ok
        t = torch.tensor([x], dtype=torch.float64, device="cpu" if cpu_ else dev)
        if dist_on:
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=None if nccl_ok else ctrl)
        return float(t.item())

    def timed_region(run, steps, warmup, min_warmup_ms, stride=None):
        """W untimed steps (and, when min_warmup_ms > 0, as many more as that much time takes), then EXACTLY `steps`
        timed steps between barrier + synchronize on both sides; the time is the MAX over the ranks.  With --full,
        sampled HIP event pairs on the launch stream give the per-step GPU time (the roofline's)."""
        import gc
        if stride is None:
            stride = max(1, int(args.event_stride)) if args.event_stride else max(1, steps // min(64, max(4, steps // 5)))
            if not args.event_stride and stride % 2 == 0:
                stride += 1          # (odd: every 4th launch measures its block costs, the one behind it carries their sort -- the samples must not
                                     # lock onto either; a 20-step run keeps 4 pairs: a pair costs the wall clock ~5 us, 7 of them were 1 % of such a run)
        # (a plain run has no event pairs: nothing but the steps between the clocks)
        ev = [event_pair() if args.full and k % stride == 0 else None for k in range(steps)]
        gc.collect()
        gc.disable()            # a step is ~0.3 ms: keep collector pauses out of the timed region
        t_w = time.perf_counter()
        w_done = 0
        out = None
        while w_done < warmup or (time.perf_counter() - t_w) * 1e3 < min_warmup_ms:
            o_k = run.step()
            out = o_k if o_k is not None else out
            w_done += 1
            if w_done % 8 == 0:
                sync()
        o_k = run.drain()
        out = o_k if o_k is not None else out
        barrier()
        t0_ = time.perf_counter()
        for k in range(steps):
            if ev[k]:
                ev[k][0].record()
            o_k = run.step()
            out = o_k if o_k is not None else out
            if ev[k]:
                ev[k][1].record()
        if run.pending:
            out = run.drain()                 # the last step's exchange is inside the timed region
        barrier()
        el = time.perf_counter() - t0_
        gc.enable()
        kms = [p_[0].elapsed_time(p_[1]) for p_ in ev if p_] if not stub else [el / steps * 1e3] * steps
        return {"elapsed": max_over_ranks(el), "kernel_ms": sorted(kms), "warmup_done": w_done, "out": out, "steps": steps}

    # bring the communicator up BEFORE the warm-up (the first collective builds the RCCL rings: hundreds
    # of milliseconds with an idle GPU); the barrier in front of the timed region is then a few tens of
    # microseconds and does not let the clocks drop
    barrier()
    barrier()

    # ---- preflight (VERDICT r04 "next" #1): the exchange this run is about to time, on a small batch, checked -------
    # One small batch of the same family (same sharding rule, same record form, two steps in flight) through the
    # exchange mode in force; rank 0 compares what it gathered with its own trace of the whole small batch.  A mismatch
    # or an exception on any rank moves every rank one rung down the ladder native -> slot -> packed -> dense -> padded -> staged
    # (triro.ray.sharded.preflight: the verdict is all-reduced on the gloo control group), and the run is timed in the
    # mode that passed: a first contact with N real GPUs that misbehaves costs bandwidth, not the bench line.
    exchange = None
    if gather_on and not args.no_preflight:
        small_res = max(64, min(args.res, 256) // 8 * 8)
        wl_s = build_workload(args, world, rank, dev, v, rad, share, args.workload, args.scaling, small_res,
                              min(args.total_rays, 1 << 18))
        expected_s = []

        def pf_run():
            rn = Runner(wl_s, args.chunks)
            got = None
            for _ in range(3):
                o_k = rn.step()
                got = o_k if o_k is not None else got
            o_k = rn.drain()
            return o_k if o_k is not None else got

        def pf_expected():
            if not expected_s:
                ao, ad = wl_s["all_rays"]()
                b = wl_s["bshape"]
                expected_s.append([x.reshape(*b, *x.shape[ao.dim() - 1:]) for x in r.intersects_closest(ao, ad)])
            return expected_s[0]
        try:
            exchange = S.preflight(dst=0, run=pf_run, expected=pf_expected)
        except Exception as exc:      # noqa: BLE001 -- no rung passed: say so, and time the run WITHOUT a gather rather than not at all
            exchange = {"exchange_mode_used": None, "requested": None, "attempts": getattr(S, "preflight_log", [{}])[-1].get("attempts", []),
                        "error": f"{type(exc).__name__}: {exc}"}
            gather_on = False
            print(f"bench.py: no exchange mode passed the preflight ({exc}); the run is timed WITHOUT the result gather", file=sys.stderr)
        del wl_s, expected_s
        if not stub:
            torch.cuda.empty_cache()
    run = Runner(wl, args.chunks)
    packed_ok, slot_rec = run.packed_ok, run.slot_rec

    sync()
    t_first = time.perf_counter()
    out = run.step()                  # very first call: lazy initialisation + no learned launch order yet
    if run.pending:
        out = run.drain()
    sync()
    first_call_ms = (time.perf_counter() - t_first) * 1e3
    # what the cold call returned: the steady-state launches of the timed region must reproduce it bit for bit (--full)
    first_out = [x.clone() for x in out] if args.full and out is not None and out[0] is not None else None
    # Everything that would leave the GPU idle between warm-up and the timed region (creating the
    # event objects, a garbage collection) happens BEFORE the warm-up: after a few milliseconds of
    # idleness the chip needs ~50 launches to come back to its steady clock, which is all a
    # 20-step run ever sees (measured: 0.275 instead of 0.256 ms per launch).
    # (the event pairs bracket every `stride`-th step: an event is a packet of its own in the queue, two per step cost
    # the wall clock -- from which `value` is computed -- a few microseconds of every 200; short runs keep every step)
    #
    # The protocol SURVEY.md 8(d) names -- W warm-ups, then K timed steps, nothing else -- first: on this batch shape
    # the library is still learning its launch order then (the first launches of a shape measure block costs and try
    # both node flavours), so this is what a caller gets on calls W+1 ... W+K of a new batch; `value` below is the
    # steady state after at least --min-warmup-ms of the same call.  Both are in the line (VERDICT r04 "next" #3).
    # (a plain run times the steady state only: the protocol figure is --full's)
    proto = None
    if args.full and args.min_warmup_ms > 0 and not stub:
        proto = timed_region(run, args.steps, args.warmup, 0.0)
    main_ = timed_region(run, args.steps, args.warmup if proto is None else 0, args.min_warmup_ms)
    elapsed, kernel_ms, out = main_["elapsed"], main_["kernel_ms"], main_["out"] if main_["out"] is not None else out
    w_done = main_["warmup_done"] + ((proto["warmup_done"] + proto["steps"]) if proto else 0)
    if args.dump_outputs and rank == 0:      # before anything else runs on this handle
        dump_outputs(args.dump_outputs, out)
    # what an event pair costs with nothing between its two records: the interval a pair reports holds that much more
    # than the kernel (rocprofv3's dispatch time does not), which is how kernel_avg_ms could exceed ms_per_step
    empty_pair_ms = 0.0
    if args.full and not stub:
        eps = timed_steps(200, lambda k: None)
        empty_pair_ms = float(np.median(eps))
    if os.environ.get("TRIRO_BENCH_TRACE") and rank == 0:   # per-step durations, launch order (--full: event pairs)
        print("per-step ms:", " ".join(f"{x:.3f}" for x in kernel_ms), file=sys.stderr)
    kernel_raw_ms = float(np.mean(kernel_ms)) if kernel_ms else None
    kernel_avg_ms = max(kernel_raw_ms - empty_pair_ms, 1e-6) if kernel_ms else None

    # the last timed step against the cold first call (different launch order, split set, tiles and
    # node flavour; same rays): any difference is a bug in a "speed only" mechanism
    verified = None
    if first_out is not None and out is not None and out[0] is not None:
        verified = all(torch.equal(a, b) for a, b in zip(out, first_out))

    # ---- N > 1: the other scaling of the same metric, in the same line (VERDICT r04 "next" #1b) -------------------
    companions_n = {}
    if args.full and gather_on and world > 1 and not args.no_companions:
        def companion(name, workload, scaling, chunks, steps):
            try:
                w2 = build_workload(args, world, rank, dev, v, rad, resolve_share(args, world), workload, scaling, args.res, args.total_rays)
                rn = Runner(w2, chunks)
                o1 = rn.step()
                o1 = rn.drain() if rn.pending else o1
                first2 = [x.clone() for x in o1] if o1 is not None and o1[0] is not None else None
                m2 = timed_region(rn, steps, max(args.warmup, 10), args.min_warmup_ms)
                ok2 = None
                if first2 is not None and m2["out"] is not None and m2["out"][0] is not None:
                    ok2 = all(torch.equal(a, b) for a, b in zip(m2["out"], first2))
                companions_n[name] = {"value": round(w2["n_total"] * steps / m2["elapsed"] / 1e6, 2), "unit": "Mrays/s",
                                      "ms_per_step": round(m2["elapsed"] / steps * 1e3, 4), "steps": steps,
                                      "rays_total": w2["n_total"], "shard_rays": [z_ - a_ for a_, z_ in w2["bounds_all"]],
                                      "chunks": chunks or "auto", "verified": ok2}
                del w2, rn
            except Exception as exc:      # noqa: BLE001 -- a companion must never cost the bench line
                companions_n[name] = {"error": f"{type(exc).__name__}: {exc}"}
        if args.workload == "c5i" and not strong_c5i:
            companion("strong_1024" if args.res == 1024 else f"strong_{args.res}", "c5i", "strong", args.chunks, min(args.steps, 200))
        elif args.workload == "c5i":
            companion("weak", "c5i", "weak", args.chunks, min(args.steps, 200))
        else:
            if args.chunks != 0:      # (chunks 0 IS the library's rule: nothing to put beside it)
                companion("default_chunks", "c5ii", "strong", 0, min(args.steps, 10))
    run.all_rays = None
    if rank == 0:
        value = n_total * args.steps / elapsed / 1e6
        # the node array the timed launches walked: the exact 64-byte nodes or the 32-byte grid nodes
        # (the streaming launch always, the direct closest launch when the library measured them
        # faster: tr_bvh_last_launch) -- "one read of the BVH" counts the arrays that kernel can touch
        grid_nodes = False
        if not stub:
            if args.workload == "c5ii":
                grid_nodes = True
            else:
                try:
                    grid_nodes = bool(r.as_wrapper.last_launch()["grid_nodes"])
                except Exception:
                    grid_nodes = False
        node_bytes_used = info["num_nodes"] * 32 if grid_nodes else info["node_bytes"]
        bvh_bytes = node_bytes_used + info["tri_bytes"]
        algo_bytes = n * BYTES_PER_RAY_CLOSEST + bvh_bytes          # per launch (= per rank and step)
        traffic, traffic_src = None, None
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        default_c5i = args.workload == "c5i" and args.res == 1024 and args.rays == "pinhole" and not strong_c5i
        default_c5ii = args.workload == "c5ii" and args.total_rays == C5II_RAYS
        if args.full and (default_c5i or default_c5ii) and os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if default_c5i:
                    traffic = tj.get("closest_hbm_bytes_per_launch")
                else:       # per launch of one rank: scaled from the profiled 12.5 M-ray shard to this rank's rays
                    per_ray = tj.get("c5ii_hbm_bytes_per_ray")
                    traffic = int(per_ray * n) if per_ray else None
                traffic_src = f"profiles/traffic.json (static: rocprofv3 PMC passes of {tj.get('round', 'an earlier round')}, not measured in this run)"
            except Exception:
                traffic = None
        hit0 = out[0] if out is not None and out[0] is not None else None
        gather_txt = ""
        if gather_on:
            gather_txt = ", results gathered to rank 0 inside the timed region"
            if args.force_gather and world == 1:
                gather_txt += " [--force-gather: the exchange is a self-gather in a one-rank communicator]"
            via = "gloo, host-staged" if (gloo or (S is not None and S.exchange_mode == "staged")) else "RCCL"
            if packed_ok:
                gather_txt += (f" (4 B/ray slot records over {via}, finished on rank 0 from its copy of the rays, " if slot_rec else
                               f" (12 B/ray packed records over {via}, expanded on rank 0, ") + "exchange of step k overlaps trace of step k+1)"
                if slot_rec and S.exchange_mode == "native":
                    gather_txt += " [the step is ONE C call: tr_sharded_closest_step, libtriro_rccl.so]"
            else:
                gather_txt += f" (26 B/ray dense outputs over {via}, exchange mode '{S.exchange_mode}')"
        metric = "Mrays/s closest-hit, 1M-tri mesh, 1024^2 ray batch"
        kernel_name = "k_query_direct<CLOSEST>"
        if strong_c5i:
            wl_txt = (f"C5(i): icosphere({args.subdiv})+displacement seed 0, {len(f)} tris; ONE {args.res}x{args.res} "
                  f"{args.rays} batch cut into {world} row bands; intersects_closest (stream_compaction=False)")
            par = f"ray-sharded x{world}, BVH replicated" + gather_txt
            scaling = "strong"
        elif args.workload == "c5i":
            wl_txt = (f"C5(i): icosphere({args.subdiv})+displacement seed 0, {len(f)} tris; {args.res}x{args.res} "
                  f"{args.rays} rays per GPU; intersects_closest (stream_compaction=False)")
            par = f"ray-sharded x{world}, BVH replicated" + gather_txt
            if world > 1 and share is not None:
                par += (f"; the {world} x {args.res}^2 rays of a step are cut into row bands, rank 0's narrower (dst_share {share}): "
                        f"total work per step = {world} x the 1-GPU batch")
            scaling = "weak"
        else:
            metric = "Mrays/s closest-hit, 1M-tri mesh, 100M-ray batch (BASELINE.json config 5; not the 1024^2 headline batch)"
            kernel_name = "k_query_stream<CLOSEST>"
            wl_txt = (f"C5(ii): icosphere({args.subdiv})+displacement seed 0, {len(f)} tris; ONE batch of {n_total} hash rays "
                  f"(seed 99) in {world} contiguous shard(s); intersects_closest (stream_compaction=False)")
            par = f"ray-sharded x{world}, BVH replicated" + gather_txt
            scaling = "strong"
        res = {
            "metric": metric,
            "value": round(value, 2), "unit": "Mrays/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "f32",
            "data": "stub tracer: launcher self-test, NOT a measurement" if stub else
                    ("synthetic; FUNCTIONAL RUN over gloo (ranks share GPUs, results staged through the host): NOT a measurement"
                     if gloo else "synthetic"),
            "verified": verified,
            "config": {"workload": wl_txt, "rays_per_gpu": n, "rays_total": n_total, "triangles": int(len(f)),
                       "parallelism": par, "dst_share": share if world > 1 else None,
                       "shard_rays": [z_ - a_ for a_, z_ in bounds_all] if world > 1 else None, "warmup_steps_done": w_done,
                       "warmup_note": ("`value` = the steady state: `warmup_steps_done` launches of this batch shape precede its timed region "
                                       f"(the requested {args.warmup}, the {args.steps} timed steps of `value_warmup_requested`, and "
                                       f"--min-warmup-ms {args.min_warmup_ms:g} of further launches); `value_warmup_requested` = exactly "
                                       f"--warmup {args.warmup} launches, then {args.steps} timed steps (SURVEY.md 8d's protocol)") if proto else None,
                       "exchange_mode_used": (exchange or {}).get("exchange_mode_used") if gather_on or exchange else None,
                       "rccl_ok": (nccl_ok if (dist_on and not gloo) else None),
                       "exchange": exchange,
                       "bvh_depth": info["depth"], "bvh_bytes": int(bvh_bytes), "bvh_build_ms": round(build_ms, 2),
                       "hit_fraction": round(float(hit0.float().mean().item()), 4) if hit0 is not None else None},
        }
        if args.full:
            res["value_warmup_requested"] = round(n_total * proto["steps"] / proto["elapsed"] / 1e6, 2) if proto else None
            res["ms_per_step_warmup_requested"] = round(proto["elapsed"] / proto["steps"] * 1e3, 4) if proto else None
            achieved = algo_bytes / (kernel_avg_ms * 1e-3) / 1e9
            algo_bytes_exact = n * BYTES_PER_RAY_CLOSEST + info["node_bytes"] + info["tri_bytes"]
            compulsory = n * BYTES_PER_RAY_CLOSEST / (kernel_avg_ms * 1e-3) / 1e9
            res["roofline"] = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                               "frac": round(achieved / HBM_PEAK_GBPS, 5), "traffic": traffic, "traffic_source": traffic_src,
                               "kernel": kernel_name, "kernel_avg_ms": round(kernel_avg_ms, 4),
                               "kernel_event_interval_ms": round(kernel_raw_ms, 4), "empty_event_pair_ms": round(empty_pair_ms, 4),
                               "kernel_min_ms": round(max(kernel_ms[0] - empty_pair_ms, 0.0), 4),
                               "kernel_median_ms": round(max(kernel_ms[len(kernel_ms) // 2] - empty_pair_ms, 0.0), 4), "kernel_samples": len(kernel_ms), "first_call_ms": round(first_call_ms, 4),
                               "algorithmic_bytes": int(algo_bytes),
                               "node_flavour": "32-byte grid nodes" if grid_nodes else "exact 64-byte nodes",
                               "frac_on_exact_node_bytes": round(algo_bytes_exact / (kernel_avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 5),
                               "compulsory_frac": round(compulsory / HBM_PEAK_GBPS, 5),
                               "note": "achieved = (50 B/ray compulsory I/O + one read of the node and triangle arrays the launch walks) per launch / "
                                       "kernel_avg_ms = the mean interval of kernel_samples HIP event pairs spread over the timed region "
                                       "(kernel_event_interval_ms) minus what a pair reports with NOTHING between its records "
                                       "(empty_event_pair_ms, the median of 200 measured in this run): the rocprofv3 dispatch time of "
                                       "the same command is in profiles/r06c_summary.md; compulsory_frac counts the 50 B/ray only; the path is "
                                       "cache-latency / instruction-issue bound, not HBM-bandwidth bound (DESIGN.md 5); "
                                       "frac_on_exact_node_bytes = the same time against round 1's numerator (64-byte nodes), "
                                       "for comparison across rounds only"}
            if gather_on:
                res["roofline"]["note"] += ("; kernel_avg_ms here is the caller-stream time of a step (trace; the exchange and the "
                                            "expansion run on RCCL's and a side stream)" if packed_ok else
                                            "; kernel_avg_ms here includes the result gather")
        for name_, comp_ in companions_n.items():
            res[name_] = comp_
        if companions_n:
            res["scaling_note"] = ("`value` is the " + scaling + "-scaling figure of this run; "
                                   + ", ".join(companions_n) + " = the same ranks, exchange mode and metric on the other split of the "
                                   "work (strong_<res>: ONE res^2 batch cut into N row bands -- the metric's literal batch; weak: N such "
                                   "batches per step; default_chunks: the chunking ONE library call uses instead of bench.py's one chunk "
                                   "per shard with two steps in flight)")
        if args.full:
            res["parity"] = parity_error_bars()
        single = world == 1 and not stub
        if args.full and single and not args.no_companions and args.workload == "c5i":
            # honest companions of the steady-state figure: the same launch
            # without a learned block order, and with an order that is always one frame stale
            rl = res["roofline"]
            hops.set_option("adaptive", 0)
            for _ in range(5):
                r.intersects_closest(origins, dirs)
            cold = timed_steps(100, lambda k: r.intersects_closest(origins, dirs))
            hops.set_option("adaptive", 1)
            rl["cold_kernel_ms"] = round(float(np.mean(cold)), 4)
            # what a one-shot call really gets: the FIRST launch of this batch shape on fresh handles (no
            # order, exact nodes, BVH arena not yet in any cache); a small query first, so that the
            # handle's scheduling buffers exist and only GPU work lies between the events
            small_o, small_d = origins[:64].contiguous(), dirs[:64].contiguous()
            firsts = []
            for _ in range(8):
                rr = RayMeshIntersector(vertices=vt, faces=ft)
                rr.intersects_closest(small_o, small_d)
                sync()
                e0, e1 = event_pair()
                e0.record()
                rr.intersects_closest(origins, dirs)
                e1.record()
                sync()
                firsts.append(e0.elapsed_time(e1))
                del rr
            rl["first_launch_kernel_ms"] = round(float(np.median(firsts)), 4)
            rl["first_launch_note"] = ("median over 8 fresh handles of the first full-size launch (query kernel on a cold "
                                       "arena + k_sched_sort); cold_kernel_ms = steady launches with adaptive=0 (no order, rows). "
                                       "A sampling pre-pass for first launches was built and measured: no gain "
                                       "(profiles/r03_prepass_first_launch.jsonl)")
            if args.rays == "pinhole":
                frames = []
                for k in range(8):      # camera orbiting by 0.25 degrees per frame
                    frames.append((torch.from_numpy(np.ascontiguousarray(rotate_y(np.ascontiguousarray(o_np), 0.25 * k))).to(dev),
                                   torch.from_numpy(rotate_y(d_np, 0.25 * k)).to(dev)))
                seq = list(range(8)) + list(range(6, 0, -1))      # ping-pong: every step moves by one frame
                for k in range(2 * len(seq)):
                    r.intersects_closest(*frames[seq[k % len(seq)]])
                mov = timed_steps(140, lambda k: r.intersects_closest(*frames[seq[k % len(seq)]]))
                rl["moving_camera_kernel_ms"] = round(float(np.mean(mov)), 4)
                rl["moving_camera_note"] = "camera orbits 0.25 deg per step: the learned launch order is one frame stale"
                del frames
            # the reference's own published benchmark shape (test/performance_test.py:10-20, 39-44, 54-57:
            # 640 x 360 pinhole rays, f = 444 px, stride-0 origin, 83.62 us per Python call on an RTX 3090
            # with the camera inside a bedroom model that is not obtainable here): on the headline mesh
            # (camera outside) and on workloads.interior_room() (909 088 tris, camera inside)
            rs = {}
            eye = np.array([0.0, 0.0, 2.5 * rad])
            for name, rr, e, t in (("headline", r, eye, np.zeros(3)), ("interior", None, W.INTERIOR_EYE, W.INTERIOR_TARGET)):
                if rr is None:
                    vi, fi = W.interior_room()
                    rr = RayMeshIntersector(vertices=torch.from_numpy(vi).to(dev), faces=torch.from_numpy(fi).to(dev))
                _, d_rs = W.ref_shape_rays(e, t)
                o_rs = torch.from_numpy(np.asarray(e, np.float32)).to(dev).expand(360, 640, 3)      # stride 0, as in the reference
                d_rs = torch.from_numpy(d_rs).to(dev)
                for _ in range(40):
                    rr.intersects_closest(o_rs, d_rs)
                kms = timed_steps(200, lambda k: rr.intersects_closest(o_rs, d_rs))
                sync()
                t1 = time.perf_counter()
                for _ in range(500):
                    out_rs = rr.intersects_closest(o_rs, d_rs)
                sync()
                call_ms = (time.perf_counter() - t1) / 500 * 1e3
                t1 = time.perf_counter()
                for _ in range(200):
                    out_rs = rr.intersects_closest(o_rs, d_rs)
                    sync()               # the reference's loop synchronises in every call (cudaFree, ray.cpp:287)
                sync_ms = (time.perf_counter() - t1) / 200 * 1e3
                # the same call captured in a HIP graph (torch.cuda.graph on a side stream that has been queried
                # before: the library allocates nothing and never synchronises in a warmed-up query) and replayed
                # with a synchronisation per replay: what is left of the host side of a small synchronous call
                graph_ms = None
                try:
                    gs = torch.cuda.Stream(dev)
                    gs.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(gs):
                        for _ in range(12):
                            rr.intersects_closest(o_rs, d_rs)
                    torch.cuda.current_stream(dev).wait_stream(gs)
                    sync()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=gs):
                        out_g = rr.intersects_closest(o_rs, d_rs)
                    for _ in range(20):
                        graph.replay()
                    sync()
                    t1 = time.perf_counter()
                    for _ in range(200):
                        graph.replay()
                        sync()
                    graph_ms = (time.perf_counter() - t1) / 200 * 1e3
                    if not all(torch.equal(a, b) for a, b in zip(out_g, out_rs)):
                        graph_ms = None
                    del graph, out_g
                except Exception as exc:      # a companion must never cost the bench line
                    print(f"bench.py: graph replay companion skipped ({exc})", file=sys.stderr)
                rs[name] = {"kernel_ms": round(float(np.mean(kms)), 4), "call_ms": round(call_ms, 4),
                            "call_sync_ms": round(sync_ms, 4),
                            "graph_replay_sync_ms": None if graph_ms is None else round(graph_ms, 4),
                            "hit_fraction": round(float(out_rs[0].float().mean().item()), 4),
                            "triangles": int(rr.bvh_info()["num_tris"])}
            res["ref_shape"] = {"rays": 640 * 360, "scenes": rs,
                                "ref_shape_kernel_ms": rs["interior"]["kernel_ms"], "ref_shape_call_ms": rs["interior"]["call_ms"],
                                "note": "640x360 pinhole, f=444 px, stride-0 origin (the reference's published call: 83.62 us wall "
                                        "on an RTX 3090, its own bedroom scene); kernel_ms = HIP events around the call, call_ms = "
                                        "wall per Python call in a loop of 500 (asynchronous launches), call_sync_ms = with a device "
                                        "synchronisation in every call as the reference's loop has, graph_replay_sync_ms = the call captured in a HIP "
                                        "graph and replayed, one synchronisation per replay"}
            # Two batches in flight: the same launches dealt round-robin to two streams, each with its own outputs
            # (and its own learned launch order: the order is kept per (handle, stream)).  The second launch fills
            # the ramp-down of the first -- a launch ends with a few long waves.  NOT the headline (`value` is one
            # stream, one launch at a time, as the reference's loop runs): what a caller that pipelines batches gets.
            side = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
            for s_ in side:
                s_.wait_stream(torch.cuda.current_stream(dev))
            outs2 = [None, None]
            for k in range(80):
                with torch.cuda.stream(side[k & 1]):
                    outs2[k & 1] = r.intersects_closest(origins, dirs)
            sync()
            t1 = time.perf_counter()
            for k in range(600):
                with torch.cuda.stream(side[k & 1]):
                    outs2[k & 1] = r.intersects_closest(origins, dirs)
            sync()
            pip_ms = (time.perf_counter() - t1) / 600 * 1e3
            first_out = r.intersects_closest(origins, dirs)
            sync()
            res["pipelined"] = {"streams": 2, "ms_per_step": round(pip_ms, 4), "mrays_per_s": round(n / pip_ms / 1e3, 1),
                                "results_identical": bool(all(torch.equal(a, b) for o2 in outs2 for a, b in zip(o2, first_out))),
                                "note": "600 launches of the same batch dealt round-robin to two streams (own outputs per stream): "
                                        "the next launch fills the ramp-down of the previous one; informational, not `value`"}
            del outs2, first_out
            # what the traversal of one launch touches (instrumented kernel): informational -- most of it is served by
            # L1 / L2, so it is NOT compared with any bandwidth ceiling (round 3's "gather_ceiling" did, and said nothing)
            st = hops.trace_stats_closest(r.as_wrapper, origins, dirs)
            node_b = 32 if grid_nodes else 64
            res["traversal"] = {"node_visits_per_ray": round(st["node_visits"] / st["rays"], 2),
                                "tri_tests_per_ray": round(st["tri_tests"] / st["rays"], 2),
                                "node_record_bytes": node_b,
                                "bytes_requested_per_launch": int(st["node_visits"] * node_b + st["tri_tests"] * 48),
                                "note": "node visits x the record size of the node flavour the timed launches walked + triangle "
                                        "tests x 48 B; requests, mostly cache hits -- compare with roofline.traffic (HBM bytes)"}
        if args.stats and single:
            st = hops.trace_stats_closest(r.as_wrapper, origins, dirs)
            res["trace_stats"] = {k: (v_ / st["rays"] if k != "rays" else v_) for k, v_ in st.items()}
        if args.full and single and not args.no_cpu_baseline:
            if o_np is not None:
                res["cpu_baseline"] = cpu_baseline(v, f, o_np, d_np)
            else:
                m = min(n, 1 << 20)
                res["cpu_baseline"] = cpu_baseline(v, f, origins[:m].cpu().numpy(), dirs[:m].cpu().numpy())
        print(json.dumps(res), flush=True)
    if verified is False:
        print("bench.py: the last timed step's outputs differ from the first call's -- a scheduling hint changed results",
              file=sys.stderr)
    if dist_on:
        dist.barrier(group=None if nccl_ok else ctrl)
        dist.destroy_process_group()
    return 3 if verified is False else 0


# ---- one-GPU emulation of the destination rank of an N-rank run --------------------------------
def run_emulation(args):
    """bench.py --emulate-world N [--workload c5i|c5ii] [--scaling weak|strong] [--dst-share s|auto]

    What the destination rank (rank 0) of an N-GPU run does per step, on ONE GPU: it traces its own shard
    with the real tracer (dense, straight into its rows of the outputs), the other ranks' 12-byte records --
    traced here beforehand, outside the clock -- arrive as device copies on a copy stream, and their expansion
    runs on the side stream: triro.ray.sharded.EmulatedWorld drives the very pipeline code of a real run
    (closest_of_shard_async), only the transport is replaced.  The peers only trace, so rank 0 is the bound;
    the line reports its step time next to the plain single-GPU step of the same workload and the scaling
    that bound implies.  NOT a multi-GPU measurement (labelled in every field that could be mistaken for one)."""
    import numpy as np
    import torch
    import workloads as W
    import triro.backend.ops as hops
    from triro.ray.ray_optix import RayMeshIntersector
    from triro.ray.sharded import EmulatedWorld, shard_bounds, dst_bounds

    if not torch.cuda.is_available():
        raise SystemExit("bench.py --emulate-world needs a GPU")
    N = args.emulate_world
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for kv in args.opt:
        k, v_ = kv.split("=", 1)
        hops.set_option(k, int(v_))
    v, f = W.headline_mesh(args.subdiv)
    rad = float(np.linalg.norm(v, axis=1).max())
    r = RayMeshIntersector(vertices=torch.from_numpy(v).to(dev), faces=torch.from_numpy(f).to(dev))
    share = resolve_share(args, N)
    res_ = args.res
    lo_box, hi_box = v.min(0) * 1.5, v.max(0) * 1.5
    weak = args.workload == "c5i" and args.scaling == "weak"
    pinhole = args.workload == "c5i" and args.rays == "pinhole"

    def hash_rays(a, z):
        parts_o, parts_d = [], []
        for s_ in range(a, z, 1 << 23):
            po, pd = W.hash_rays_torch(min(1 << 23, z - s_), 99, lo_box, hi_box, start=s_, device=dev)
            parts_o.append(po)
            parts_d.append(pd)
        if not parts_o:
            return torch.zeros((0, 3), device=dev), torch.zeros((0, 3), device=dev)
        return torch.cat(parts_o), torch.cat(parts_d)

    # the batch: rays_of(k) = rank k's shard as the tensors that rank would hold
    if weak:
        n = res_ * res_
        n_total = N * n
        if share is not None and share < 1.0:
            bounds = dst_bounds(n_total, N, 0, share, res_ if pinhole else 1)
        else:
            bounds = [(k * n, (k + 1) * n) for k in range(N)]
        bshape = (N * res_, res_) if pinhole else (n_total,)
        if pinhole:
            o_np, d_np = W.pinhole_grid(res_, res_, distance=2.5 * rad)
            o_img = np.broadcast_to(o_np, (res_, res_, 3))

            def rays_of(k):
                a, z = bounds[k]
                return (torch.from_numpy(np.ascontiguousarray(stacked_rows(o_img, N, a // res_, z // res_, roll=0))).to(dev),
                        torch.from_numpy(np.ascontiguousarray(stacked_rows(d_np, N, a // res_, z // res_))).to(dev))
            plain_rays = (torch.from_numpy(np.ascontiguousarray(o_img)).to(dev), torch.from_numpy(np.ascontiguousarray(d_np)).to(dev))
        else:
            def rays_of(k):
                return hash_rays(*bounds[k])
            plain_rays = hash_rays(0, n)
        plain_n = n
    else:
        n_total = res_ * res_ if args.workload == "c5i" else args.total_rays
        q = res_ if pinhole else 1
        if share is not None and share < 1.0:
            bounds = dst_bounds(n_total, N, 0, share, q)
        else:
            bounds = [shard_bounds(n_total, N, k) for k in range(N)]
        rows_ok = pinhole and all(a % res_ == 0 and z % res_ == 0 for a, z in bounds)
        bshape = (res_, res_) if pinhole else (n_total,)
        if pinhole:
            o_np, d_np = W.pinhole_grid(res_, res_, distance=2.5 * rad)
            o_full = torch.from_numpy(np.ascontiguousarray(o_np)).to(dev)
            d_full = torch.from_numpy(d_np).to(dev)

            def rays_of(k):
                a, z = bounds[k]
                if rows_ok and z > a:
                    return o_full[a // res_:z // res_], d_full[a // res_:z // res_]
                return o_full.reshape(-1, 3)[a:z], d_full.reshape(-1, 3)[a:z]
            plain_rays = (o_full, d_full)
        else:
            full = hash_rays(0, n_total)

            def rays_of(k):
                a, z = bounds[k]
                return full[0][a:z], full[1][a:z]
            plain_rays = full
        plain_n = n_total
    row_quantum = res_ if pinhole and all(a % res_ == 0 and z % res_ == 0 for a, z in bounds) else None

    def sync():
        torch.cuda.synchronize()

    # ---- the peers' records and the expected dense results, outside the clock ----------------------
    slot_rec = args.records == "slot"            # 4-byte records: rank 0 holds the rays of the whole batch
    peer_records = torch.empty((n_total,) if slot_rec else (n_total, 3), dtype=torch.int32, device=dev)
    slots = os.environ.get("TRIRO_PACKED_SLOTS", "1") != "0"      # the record form ShardedRayMeshIntersector will expand

    def trace_records(ok_, dk_, out_):
        if slot_rec:
            r.intersects_closest_slots(ok_, dk_, out=out_)
        else:
            r.intersects_closest_packed(ok_, dk_, out=out_, slots=slots)
    all_rays = None
    if slot_rec:
        if weak and pinhole:
            all_rays = (torch.from_numpy(np.ascontiguousarray(stacked_rows(o_img, N, 0, N * res_, roll=0))).to(dev),
                        torch.from_numpy(np.ascontiguousarray(stacked_rows(d_np, N, 0, N * res_))).to(dev))
        elif weak:
            all_rays = hash_rays(0, n_total)
        else:
            all_rays = plain_rays
        if row_quantum is None:
            all_rays = (all_rays[0].reshape(-1, 3), all_rays[1].reshape(-1, 3))
    expected = []
    peer_ms = 0.0
    for k in range(N):
        ok_, dk_ = rays_of(k)
        a, z = bounds[k]
        if z == a:
            expected.append(None)
            continue
        if k > 0:
            for _ in range(3):
                trace_records(ok_, dk_, peer_records[a:z])
            if k == 1:      # what a peer's step costs (its trace into records; it sends them asynchronously)
                reps = 20 if z - a < (1 << 22) else 5
                for _ in range(reps if z - a < (1 << 22) else 2):
                    trace_records(ok_, dk_, peer_records[a:z])
                sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    trace_records(ok_, dk_, peer_records[a:z])
                sync()
                peer_ms = (time.perf_counter() - t0) / reps * 1e3
        expected.append([x.reshape(z - a, *x.shape[ok_.dim() - 1:]).clone() for x in r.intersects_closest(ok_, dk_)])
    sync()
    E = EmulatedWorld(r, N, peer_records, dst_share=share, arrival_priority=args.arrival_priority, arrival=args.arrival)
    o0, d0 = rays_of(0)
    steps = args.steps
    warm = max(args.warmup, 20)
    if plain_n >= (1 << 24):
        steps, warm = min(steps, 20), min(warm, 6)

    # ---- plain single-GPU step of the same workload -------------------------------------------------
    for _ in range(warm):
        r.intersects_closest(*plain_rays)
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.intersects_closest(*plain_rays)
    sync()
    plain_ms = (time.perf_counter() - t0) / steps * 1e3

    # ---- rank 0's step in the pretended world --------------------------------------------------------
    pending = []
    import contextlib
    hp = torch.cuda.Stream(device=dev, priority=-1) if args.trace_priority else None
    if hp is not None:
        hp.wait_stream(torch.cuda.current_stream(dev))

    def trace_ctx():
        return torch.cuda.stream(hp) if hp is not None else contextlib.nullcontext()

    native = args.exchange == "native" and args.records == "slot" and args.arrival == "none" and all_rays is not None

    def step():
        if native:          # rank 0's step as ONE C call (include/triro_rccl.h); the peers' records are already there
            pending.append(E.closest_of_shard_native(o0, d0, n_total, batch_shape=bshape, dst=0, chunks=args.chunks or None,
                                                     bounds=bounds, row_quantum=row_quantum, all_rays=all_rays,
                                                     flags=hops.STEP_NO_EXCHANGE, records=E.peer_records, world=N, rank=0))
        else:
            pending.append(E.closest_of_shard_async(o0, d0, n_total, batch_shape=bshape, dst=0, chunks=args.chunks or None,
                                                    bounds=bounds, row_quantum=row_quantum, records=args.records, all_rays=all_rays))
        return pending.pop(0).wait() if len(pending) > 1 else None

    def drain():
        out_ = None
        while pending:
            out_ = pending.pop(0).wait()
        return out_
    out = None

    def device_mallocs():
        st = torch.cuda.memory_stats(dev)
        return int(st.get("num_device_alloc", 0)), int(st.get("num_device_free", 0))
    with trace_ctx():
        # The warm-up keeps the previous step's outputs alive exactly as the timed loop does (round 6).  Until then it
        # dropped them at once, the timed loop -- two steps in flight + the result the caller still holds -- needed a THIRD
        # 26-B-per-ray output pool (2.6 GB at 100 M rays), and that one hipMalloc sat inside the clock: 1 ms on pristine
        # device memory, 50-60 ms when the driver first has to scrub pages earlier processes used -- round 5's "bistable"
        # rank-0 step (1.74 / 7.5 ms for 10 timed steps: profiles/r06_emulate_bistable.txt has the kernel trace with the gap).
        for _ in range(warm):
            o_k = step()
            out = o_k if o_k is not None else out
        out = drain() or out
        sync()
        m0 = device_mallocs()
        t0 = time.perf_counter()
        for _ in range(steps):
            o_k = step()
            out = o_k if o_k is not None else out
        out = drain() or out
        sync()
        rank0_ms = (time.perf_counter() - t0) / steps * 1e3
        m1 = device_mallocs()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out)
    # the same without the peers (own shard only, dense): what the arrivals + expansions add
    for _ in range(warm):
        r.intersects_closest(o0, d0)
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.intersects_closest(o0, d0)
    sync()
    own_ms = (time.perf_counter() - t0) / steps * 1e3 if bounds[0][1] > bounds[0][0] else 0.0
    # expansion alone (all peers' rows, nothing else running)
    flat = [x.reshape(n_total, *x.shape[len(bshape):]) for x in out]
    pa, pz = bounds[1][0], bounds[-1][1]
    rl = {"row_length": row_quantum} if (slots and row_quantum) else {}

    def expand_all():
        if slot_rec:
            if row_quantum:
                ro, rd = all_rays[0][pa // row_quantum:pz // row_quantum], all_rays[1][pa // row_quantum:pz // row_quantum]
            else:
                ro, rd = all_rays[0][pa:pz], all_rays[1][pa:pz]
            r.closest_from_slots(ro, rd, peer_records[pa:pz], outs=tuple(x[pa:pz] for x in flat), row_length=row_quantum or 0)
        else:
            r.closest_expand(peer_records[pa:pz], outs=tuple(x[pa:pz] for x in flat), slots=slots, **rl)
    for _ in range(5):
        expand_all()
    sync()
    t0 = time.perf_counter()
    for _ in range(20):
        expand_all()
    sync()
    expand_ms = (time.perf_counter() - t0) / 20 * 1e3
    # ---- verification: every row against a dense trace of that rank's rays ---------------------------
    verified = True
    out = E.closest_of_shard_async(o0, d0, n_total, batch_shape=bshape, dst=0, chunks=args.chunks or None,
                                   bounds=bounds, row_quantum=row_quantum, records=args.records, all_rays=all_rays).wait()
    sync()
    flat = [x.reshape(n_total, *x.shape[len(bshape):]) for x in out]
    for k in range(N):
        a, z = bounds[k]
        if expected[k] is None:
            continue
        verified = verified and all(torch.equal(g[a:z], e) for g, e in zip(flat, expected[k]))
    bound_ms = max(rank0_ms, peer_ms)
    if weak:
        implied = N * plain_ms / bound_ms
        value = n_total / bound_ms / 1e3
    else:
        implied = plain_ms / bound_ms
        value = n_total / bound_ms / 1e3
    res = {
        "metric": f"EMULATED on one GPU: Mrays/s closest-hit implied by the destination rank's step of a {N}-rank run "
                  f"(NOT a multi-GPU measurement)",
        "value": round(value, 2), "unit": "Mrays/s", "n_gpus": 1, "emulated_world": N, "steps": steps, "warmup": warm,
        "ms_per_step": round(bound_ms, 4), "higher_is_better": True, "scaling": "weak" if weak else "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic; peers' records pre-traced, arrival emulated by device copies",
        "verified": bool(verified),
        "config": {"workload": f"{args.workload} {'weak' if weak else 'strong'}: {n_total} rays in {N} shards "
                               f"({args.rays if args.workload == 'c5i' else 'hash'} rays), headline mesh {len(f)} tris",
                   "rays_total": n_total, "rays_rank0": bounds[0][1] - bounds[0][0], "rays_peer": bounds[1][1] - bounds[1][0],
                   "dst_share": share, "chunks": args.chunks or "auto", "arrival_priority": bool(args.arrival_priority),
                   "arrival": args.arrival, "step_driver": "native (tr_sharded_closest_step)" if native else "python", "trace_priority": bool(args.trace_priority), "opts": list(args.opt), "record_form": "slot only, 4 B" if slot_rec else ("slot, u, v: 12 B" if slots else "face, u, v: 12 B")},
        "emulation": {"plain_1gpu_ms_per_step": round(plain_ms, 4), "plain_1gpu_rays": plain_n,
                      "rank0_ms_per_step": round(rank0_ms, 4), "rank0_own_trace_only_ms": round(own_ms, 4),
                      "peer_trace_ms_per_step": round(peer_ms, 4), "expansion_alone_ms": round(expand_ms, 4),
                      "expansion_rays": pz - pa,
                      "expansion_GBps": round((pz - pa) * (54 if slot_rec else 38) / (expand_ms * 1e-3) / 1e9, 1) if expand_ms > 0 else None,
                      "implied_scaling_vs_1gpu": round(implied, 3),
                      "device_mallocs_in_timed_region": m1[0] - m0[0], "device_frees_in_timed_region": m1[1] - m0[1],
                      "note": "implied = N x plain / max(rank0, peer) for weak scaling, plain / max(rank0, peer) for strong; "
                              "arrival = device-to-device copies (read + write; an xGMI receive only writes); link time is not "
                              "modelled (12-byte records: 12.6 MB per peer and 1 M rays = 0.2 ms on one 76.8 GB/s link direction at 80 %; "
                              "4-byte records: 0.07 ms); expansion_GBps counts 38 B/ray (12-byte records) or 54 B/ray (4-byte records + the ray)"},
    }
    print(json.dumps(res), flush=True)
    return 0 if verified else 3


def main(argv=None):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (RCCL across processes on this driver), before anything touches HIP
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    under_launcher = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if args.emulate_world > 1:
        if under_launcher or args.gpus != 1:
            raise SystemExit("--emulate-world runs in ONE process on one GPU")
        return run_emulation(args)
    if args.gpus > 1 and not under_launcher:
        return launch_ranks(args, argv)
    return run_rank(args)


if __name__ == "__main__":
    sys.exit(main())
