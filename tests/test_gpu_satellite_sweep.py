"""The randomised parity sweep of the fourteen satellite query libraries on the GPU (tests/satellite_sweep.py: the generator
and the family table; tests/test_satellite_sweep_cpu.py: the same cases on the host).

One test per family runs the suite's fixed seed: per iteration a fresh RayMeshIntersector or RaySceneIntersector on a random
mesh (or scene) of the iteration's kind, every native entry of the family once at the drawn knobs against the host brute
force, bit for bit with the family's own comparator, and in every second iteration a refit and the same again.  Outputs
are born poisoned and every native call is followed by poison.assert_written.  The first mismatch ends the test with the
case's description line, which reproduces it (satellite_sweep.draw); an error of a native call is not caught."""
import pytest
import torch

import poison
import satellite_sweep as S
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

CALLS = {}


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every native call of every family: counted, and all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    names = S.natives()
    originals = {name: getattr(hops, name) for name in names}

    def wrap(name):
        original = originals[name]

        def call(*args, **kwargs):
            res = original(*args, **kwargs)
            CALLS[name] = CALLS.get(name, 0) + 1
            torch.cuda.synchronize()
            poison.assert_written(*(res if isinstance(res, tuple) else (res,)), what=name)
            return res
        return call
    for name in names:
        setattr(hops, name, wrap(name))
    try:
        yield
    finally:
        for name, original in originals.items():
            setattr(hops, name, original)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_kernels_match_the_brute_force_on_random_meshes_batches_and_knobs(device, family):
    before = sum(CALLS.values())
    for iteration in range(S.SUITE_ITERATIONS[family]):
        S.run_device(S.draw(family, S.SUITE_SEED, iteration), device)
    # (scene_nearest calls tr_scene_closest_point itself, and scene_tris tr_scene_tris_any, _count and _fill, between guard rows,
    # and check every row inside: no binding to wrap)
    assert family in ("scene_nearest", "scene_tris") or sum(CALLS.values()) > before, "no native entry went through the written-check"
