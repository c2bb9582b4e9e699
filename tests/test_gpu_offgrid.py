"""The native box, triangle and plane queries (libtriro_boxes.so, libtriro_tris.so, libtriro_planes.so) against EXACT arithmetic
on ordinary float32 inputs -- full mantissas, nothing on a lattice: the families and near-touching queries of
tests/offgrid_cases.py, the same as tests/test_offgrid_cpu.py runs through the host brute forces.

Every other GPU test of these queries compares the kernels with tests/host_sim/*_sim.brute, the same header compiled with g++,
or with the integer references on snapped inputs, where float64 rounds nothing.  Here the kernels' own results -- any, count
and list, for planes both predicates and the segments -- are compared DIRECTLY with the exact tables and the exact rational
crossing points (offgrid_cases.check_sets / check_planes: what may be left out is decided there, in exact arithmetic), so the
culling of the walks is held to geometry as well, not only the leaf predicate; and bit for bit with the host brute force, the
`denormal` family included.  Each family runs at stack_entries / frontier_entries 0 (the whole capacity) and 1 (the overflow
paths).  The exact tables are computed once per process (offgrid_cases caches them)."""
import numpy as np
import pytest
import torch

import boxes_cases as BC
import offgrid_cases as OC
import planes_cases as PC
import poison
import tris_cases as TC
from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

NATIVES = ("boxes_native", "boxes_fill_native", "tris_native", "tris_fill_native", "planes_native", "planes_fill_native")
ENTRIES = (0, 1)


def T(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)


def make(name, device):
    from triro.ray.ray_optix import RayMeshIntersector
    v, f = OC.family(name)
    return RayMeshIntersector(vertices=T(v, device), faces=T(f, device))


@pytest.fixture(autouse=True)
def checked_native(poisoned_outputs):
    """every native call: all outputs checked for unwritten elements"""
    import triro.backend.ops as hops
    originals = {name: getattr(hops, name) for name in NATIVES}

    def wrap(name):
        original = originals[name]

        def call(*args, **kwargs):
            res = original(*args, **kwargs)
            torch.cuda.synchronize()
            poison.assert_written(*(res if isinstance(res, tuple) else (res,)), what=name)
            return res
        return call
    for name in NATIVES:
        setattr(hops, name, wrap(name))
    try:
        yield
    finally:
        for name, original in originals.items():
            setattr(hops, name, original)


def host(x):
    return None if x is None else x.cpu().numpy()


def native_tris(r, tri, device, stack_entries):
    import tris_sim
    import triro.backend.ops as hops
    tt = T(tris_sim.triangles(tri).reshape(-1, 3, 3), device)
    any_ = hops.tris_native(r.as_wrapper, tt, "any", stack_entries)
    count = hops.tris_native(r.as_wrapper, tt, "count", stack_entries)
    offsets, face = hops.faces_meeting_triangles_native(r.as_wrapper, tt, stack_entries)
    torch.cuda.synchronize()
    poison.assert_written(offsets, what="faces_meeting_triangles_native offsets")
    return tris_sim.Result(host(any_), host(count), host(offsets), host(face))


def native_boxes(r, lo, hi, device, stack_entries):
    import boxes_sim
    import triro.backend.ops as hops
    lo, hi = boxes_sim.boxes(lo, hi)
    lt, ht = T(lo, device), T(hi, device)
    any_ = hops.boxes_native(r.as_wrapper, lt, ht, "any", stack_entries)
    count = hops.boxes_native(r.as_wrapper, lt, ht, "count", stack_entries)
    offsets, face, inside = hops.faces_in_boxes_native(r.as_wrapper, lt, ht, True, stack_entries)
    torch.cuda.synchronize()
    poison.assert_written(offsets, what="faces_in_boxes_native offsets")
    return boxes_sim.Result(host(any_), host(count), host(offsets), host(face), host(inside))


def native_planes(r, origins, normals, device, cut, frontier_entries):
    import planes_sim
    import triro.backend.ops as hops
    o, nr = planes_sim.planes(origins, normals)
    ot, nt = T(o, device), T(nr, device)
    any_ = hops.planes_native(r.as_wrapper, ot, nt, "any", cut, frontier_entries)
    count = hops.planes_native(r.as_wrapper, ot, nt, "count", cut, frontier_entries)
    offsets, face, seg = hops.faces_on_planes_native(r.as_wrapper, ot, nt, cut, cut, frontier_entries)
    torch.cuda.synchronize()
    poison.assert_written(offsets, what="faces_on_planes_native offsets")
    return planes_sim.Result(host(any_), host(count), host(offsets), host(face), host(seg))


@pytest.mark.parametrize("name", OC.FAMILIES)
def test_triangles_equal_exact_geometry_and_the_host_bits(device, name):
    import tris_sim
    v, f = OC.family(name)
    tri = OC.tri_queries(name).data
    r = make(name, device)
    brute = tris_sim.brute(v, f, tri)
    for entries in ENTRIES:
        what = f"{name}, triangles, stack_entries {entries}"
        got = native_tris(r, tri, device, entries)
        TC.check_identities(got, what)
        left = OC.check_sets(name, "triangles", TC.listed(got, len(tri), len(f)), got)
        TC.assert_same(got, brute, what)
        print(f"{what}: {left} exact ties left out")


@pytest.mark.parametrize("name", OC.FAMILIES)
def test_boxes_equal_exact_geometry_and_the_host_bits(device, name):
    import boxes_sim
    v, f = OC.family(name)
    lo, hi = OC.box_queries(name).data
    r = make(name, device)
    brute = boxes_sim.brute(v, f, lo, hi)
    for entries in ENTRIES:
        what = f"{name}, boxes, stack_entries {entries}"
        got = native_boxes(r, lo, hi, device, entries)
        BC.check_identities(got, what)
        left = OC.check_sets(name, "boxes", BC.listed(got, len(lo), len(f)), got)
        BC.assert_same(got, brute, what)
        print(f"{what}: {left} exact ties left out")


@pytest.mark.parametrize("name", OC.FAMILIES)
def test_planes_equal_exact_signs_crossing_points_and_the_host_bits(device, name):
    import planes_sim
    v, f = OC.family(name)
    o, nr = OC.plane_queries(name).data
    r = make(name, device)
    brute = {cut: planes_sim.brute(v, f, o, nr, cut=cut) for cut in (False, True)}
    for entries in ENTRIES:
        what = f"{name}, planes, frontier_entries {entries}"
        got = {cut: native_planes(r, o, nr, device, cut, entries) for cut in (False, True)}
        for cut in (False, True):
            PC.check_identities(got[cut], what)
        left, ill, rows, worst = OC.check_planes(name, got[False], got[True], PC.listed)
        for cut in (False, True):
            PC.assert_same(got[cut], brute[cut], f"{what}, cut={cut}")
        print(f"{what}: {left} pairs below the bound, {ill} rows on ill-conditioned edges, {rows} rows compared, the largest "
              f"crossing error {worst:.8f} float32 steps")
