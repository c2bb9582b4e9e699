"""Scripted sequences of meshes, batches and options on ONE handle (tests/handle_scripts.py holds the table, the expected
values and the interpreter; tests/test_handle_scripts_cpu.py checks the table).

Every launch of every script is compared with the oracle bit for bit (closest_point with the host brute force) and checked
for output elements that were never written; every script asserts through tr_bvh_last_launch that it reached the state it
is about: a learned order, split blocks, a carried sort, addressing 2, launch shape 4.  The launch count and the wall time
of each script are printed, not asserted (DESIGN.md has the figures of an MI355X).

Expectations corrected against the first reading of csrc/launch_policy.inc (sched_first_launches, sched_measure): under tile = 2, split = 2 the plain and the
wanted launch shape differ, the second launch of a batch shape starts `launches` again, and so the FIFTH launch of a shape
defers its sort and the sixth carries it (script 1 runs 5 and 6 launches before its transitions, not 4 and 5); with default
options the two shapes are one and the fourth launch defers (scripts 2, 6 and 7).  A refit, unlike update_raw, leaves
`launches` alone: the first launch after it carries the waiting sort.  And the soup has 24 000 triangles, not 20 000:
only then is it larger than the sphere (20 480), so that the updates of scripts 4 and 5 grow the arena and the wide buffers."""
import time

import pytest

import handle_scripts as S
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(S.SCRIPTS))
def test_script(device, tmp_path, name):
    import torch
    script = S.SCRIPTS[name]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    launches = S.run_script(script, device, tmp_path, label=name)
    torch.cuda.synchronize()
    print(f"{name}: {len(script)} steps, {launches} launches compared, {time.perf_counter() - t0:.2f} s (oracle included on first use)")
    assert launches == S.count_launches(script)
