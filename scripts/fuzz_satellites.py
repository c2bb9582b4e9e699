#!/usr/bin/env python3
"""Randomised GPU-vs-brute-force parity sweep of the fourteen satellite query libraries (run on the GPU box): the long-run form
of tests/test_gpu_satellite_sweep.py, with the same generator and the same family table (tests/satellite_sweep.py).  Per
iteration a fresh handle, every native entry of the family at the drawn knobs, bit for bit against the host brute force, and
in every second iteration a refit and the same again.  A mismatch prints MISMATCH with the line that reproduces the case and
the sweep goes on; an exception from a native call ends the run at once -- nothing more is started on a device that has raised.
usage: python scripts/fuzz_satellites.py [--iters 60] [--seed 1] [--family all | a family | several, comma-separated]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "host_sim")]
import torch
import poison
import satellite_sweep as S
import triro.backend.ops as hops

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=60); ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--family", default="all", help="one or several (comma-separated) of the fourteen: " + ", ".join(S.FAMILIES) + " (default: all of them)")
a = ap.parse_args()
families = S.FAMILIES if a.family == "all" else tuple(a.family.split(","))
assert all(f in S.FAMILIES for f in families), families
dev = torch.device("cuda:0")
poison.install()                                          # outputs are born poisoned, as in the suite


def checked(name, original):
    def call(*args, **kwargs):
        res = original(*args, **kwargs)
        torch.cuda.synchronize()
        poison.assert_written(*(res if isinstance(res, tuple) else (res,)), what=name)
        return res
    return call


for name in S.natives():
    setattr(hops, name, checked(name, getattr(hops, name)))
bad = 0
for family in families:
    t0, wrong = time.time(), 0
    for it in range(a.iters):
        case = S.draw(family, a.seed, it)
        try:
            S.run_device(case, dev)
        except AssertionError as e:                       # a comparison (or a written-check) failed: the finding; the device is fine
            wrong += 1
            print("MISMATCH", case.line, "::", str(e)[:400], flush=True)
        except BaseException:                             # a native call raised: stop here
            print("EXCEPTION in", case.line, flush=True)
            raise
        else:
            if it % 10 == 0:
                print("ok ", case.line, flush=True)
    bad += wrong
    print(f"family {family}: {a.iters} iterations, {wrong} mismatches, {time.time() - t0:.1f} s", flush=True)
print("done:", len(families), "families x", a.iters, "iterations,", bad, "mismatches")
sys.exit(1 if bad else 0)
