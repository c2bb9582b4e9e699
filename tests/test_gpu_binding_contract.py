"""The Python binding between the user and the native entries (triro/backend/ops.py, triro/ray/ray_optix.py,
triro/ray/scene.py): what it rejects, what shapes and dtypes it returns, what it converts.

Nothing here is about kernels: the mesh is one tetrahedron, the scene two placed copies of it, the batches hold 0, 1, 3 or 4
queries -- the only sizes at which argument checks, output allocation and reshapes can go wrong.  Four properties:

  * a rejection table: one row per rule of the three files, (call, exception type, the argument's name plus the key word of the
    message);
  * batch shapes in, batch shapes out: every public query on inputs of batch shape (), (3,), (2, 2) and (0,);
  * a list and a float64 numpy array give what the float32 GPU tensor gives, wherever array-likes are accepted;
  * strided float32 rays reach the range and the scene queries as they are and give the result of their contiguous copy."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from poison import poisoned_outputs  # noqa: F401  (autouse: the seam is swapped in every test below)

pytestmark = pytest.mark.gpu

VERTICES = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
FACES = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
PLACEMENTS = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], [[1, 0, 0, 3], [0, 1, 0, 0], [0, 0, 1, 0]]], np.float32)
BATCHES = ((), (3,), (2, 2), (0,))
b_, i32, i64, f32 = torch.bool, torch.int32, torch.int64, torch.float32


def inputs(dev, bs):
    """the arguments of every family for the batch shape bs, float32 on dev: every coordinate is a small dyadic number, so a
    float64 copy and a list hold the same values"""
    n = int(np.prod(bs, dtype=np.int64))
    k = torch.arange(n, dtype=f32, device=dev).reshape(bs) / 64
    z = torch.zeros_like(k)
    x = SimpleNamespace(bs=tuple(bs), n=n)
    x.o = torch.stack((k + 0.125, z + 0.125, z - 2), -1)            # rays up the z axis through the tetrahedron
    x.d = torch.stack((z, z, z + 1), -1)
    x.p1 = x.o + torch.tensor([0, 0, 4], dtype=f32, device=dev)     # the far ends of the same rays as segments
    x.p = torch.stack((k + 0.125, z + 0.125, z + 0.125), -1)        # points inside it
    x.lo, x.hi = x.p - 0.25, x.p + 0.25
    x.nrm = x.d
    corners = [torch.tensor(c, dtype=f32, device=dev) for c in ((-1, 0, 0), (1, 0, 0), (0, 1, 0))]
    x.tri = torch.stack([x.p + c for c in corners], -2)
    x.tmin, x.tmax = z + 0.5, z + 8
    x.r = z + 0.5
    return x


@pytest.fixture(scope="module")
def c(device):
    """the tetrahedron, the scene, an unbuilt handle and the inputs of each batch shape"""
    from triro.ray import RaySceneIntersector
    from triro.ray.ray_optix import OptixAccelStructureWrapper, RayMeshIntersector
    c = SimpleNamespace(dev=device)
    c.r = RayMeshIntersector(vertices=torch.from_numpy(VERTICES).to(device), faces=torch.from_numpy(FACES).to(device))
    c.s = RaySceneIntersector([c.r], [0, 0], PLACEMENTS)
    c.aw, c.sh, c.di = c.r.as_wrapper, c.s._handle, c.s.device.index
    c.unbuilt = OptixAccelStructureWrapper()
    c.x = {bs: inputs(device, bs) for bs in BATCHES}
    x = c.x[(3,)]
    c.direction = torch.tensor([0.0, 0.0, 1.0], device=device)
    c.count, c.offsets = torch.zeros(3, dtype=i32, device=device), torch.zeros(3, dtype=i64, device=device)
    c.slots = torch.full((3,), -1, dtype=i32, device=device)
    c.packed = torch.full((3, 3), -1, dtype=i32, device=device)
    c.outs = lambda: (torch.zeros(3, dtype=b_, device=device), torch.zeros(3, dtype=b_, device=device), torch.zeros(3, dtype=i32, device=device),
                      torch.zeros((3, 3), dtype=f32, device=device), torch.zeros((3, 2), dtype=f32, device=device))
    # the eight fills: (function, the arguments before (count, offsets, total))
    c.fills = {"within": ("within_fill_native", (c.aw, x.p, 0.5)), "boxes": ("boxes_fill_native", (c.aw, x.lo, x.hi)),
               "tris": ("tris_fill_native", (c.aw, x.tri)), "planes": ("planes_fill_native", (c.aw, x.p, x.nrm)),
               "cross": ("cross_fill_native", (c.aw, x.o, x.d, None, None)),
               "scene_cross": ("scene_cross_fill_native", (c.sh, c.di, x.o, x.d, None, None)),
               "scene_points": ("scene_points_fill_native", (c.sh, c.di, x.p, c.direction)),
               "scene_tris": ("scene_tris_fill_native", (c.sh, c.di, x.tri))}
    # the four functions that take `outs`: outs -> the call
    c.with_outs = {"intersects_closest": lambda outs: hops().intersects_closest(c.aw, x.o, x.d, outs=outs),
                   "closest_from_slots": lambda outs: hops().closest_from_slots(c.aw, x.o, x.d, c.slots, outs=outs),
                   "closest_expand_slots": lambda outs: hops().closest_expand_slots(c.aw, c.packed, outs=outs),
                   "closest_expand": lambda outs: hops().closest_expand(c.packed, c.r.mesh_vertices, c.r.mesh_faces, outs=outs)}
    return c


def hops():
    import triro.backend.ops as ops
    return ops


# ---- 1: the rejection table -----------------------------------------------------------------------------------------------
def X(c):
    return c.x[(3,)]


V, R = ValueError, RuntimeError
# (call, exception type, the argument's name and the key word of the message as a regular expression)
REJECTED = [
    # check_rays: what every ray query of ops.py runs first
    (lambda c: c.r.intersects_any(X(c).o.cpu().numpy(), X(c).d), V, "origins must be a torch.Tensor"),
    (lambda c: c.r.intersects_any(X(c).o.cpu(), X(c).d), V, "origins must reside on a GPU"),
    (lambda c: c.r.intersects_first(X(c).o, X(c).d.cpu()), V, "directions must reside on a GPU"),
    (lambda c: c.r.intersects_count(X(c).o.double(), X(c).d.double()), V, "origins must be float32"),
    (lambda c: c.r.intersects_closest(X(c).o, X(c).d.half()), V, "directions must be float32"),
    (lambda c: c.r.intersects_location(X(c).o[:, :2], X(c).d[:, :2]), V, r"origins must have shape \[\*b, 3\]"),
    (lambda c: c.r.intersects_any(X(c).o.reshape(1, 1, 1, 3, 3), X(c).d.reshape(1, 1, 1, 3, 3)), V, "origins must have shape"),
    (lambda c: c.r.intersects_any(X(c).o, X(c).d[:2]), V, "origins .* and directions .* differ in shape"),
    (lambda c: c.r.intersects_closest_packed(X(c).o.cpu(), X(c).d), V, "origins must reside"),
    (lambda c: c.r.intersects_closest_slots(X(c).o, X(c).d.double()), V, "directions must be float32"),
    (lambda c: hops().trace_stats(c.aw, X(c).o.cpu(), X(c).d), V, "origins must reside"),
    (lambda c: hops().trace_stats_closest(c.aw, X(c).o, X(c).d.cpu()), V, "directions must reside"),
    (lambda c: hops().range_any_native(c.aw, X(c).o.cpu(), X(c).d), V, "origins must reside"),
    (lambda c: hops().range_closest_native(c.aw, X(c).o.double(), X(c).d), V, "origins must be float32"),
    (lambda c: hops().cross_count_native(c.aw, X(c).o, X(c).d[:2]), V, "differ in shape"),
    (lambda c: hops().scene_any_native(c.sh, c.di, X(c).o.cpu(), X(c).d), V, "origins must reside"),
    (lambda c: hops().scene_closest_native(c.sh, c.di, X(c).o, X(c).d.double()), V, "directions must be float32"),
    (lambda c: hops().scene_cross_count_native(c.sh, c.di, X(c).o[:, :2], X(c).d[:, :2]), V, "origins must have shape"),
    # an unbuilt handle
    (lambda c: hops().intersects_any(c.unbuilt, X(c).o, X(c).d), R, "has not been built"),
    (lambda c: hops().intersects_location(c.unbuilt, X(c).o, X(c).d), R, "has not been built"),
    (lambda c: hops().range_any_native(c.unbuilt, X(c).o, X(c).d), R, "has not been built"),
    (lambda c: hops().cross_count_native(c.unbuilt, X(c).o, X(c).d), R, "has not been built"),
    (lambda c: hops().closest_point_native(c.unbuilt, X(c).p), R, "has not been built"),
    (lambda c: hops().contains_points_native(c.unbuilt, X(c).p, c.direction, None, None), R, "has not been built"),
    (lambda c: hops().within_native(c.unbuilt, X(c).p, 0.5), R, "has not been built"),
    (lambda c: hops().boxes_native(c.unbuilt, X(c).lo, X(c).hi), R, "has not been built"),
    (lambda c: hops().tris_native(c.unbuilt, X(c).tri), R, "has not been built"),
    (lambda c: hops().planes_native(c.unbuilt, X(c).p, X(c).nrm), R, "has not been built"),
    (lambda c: hops().closest_expand_slots(c.unbuilt, c.packed), R, "has not been built"),
    (lambda c: hops().scene_commit(c.sh, [0], [0], PLACEMENTS[:1], c.di), R, "member 0.*has not been built"),
    # the single outputs, the slots and the packed records
    (lambda c: c.r.intersects_closest_packed(X(c).o, X(c).d, out=c.packed[:2]), V, r"out must be a contiguous int32 \[n, 3\]"),
    (lambda c: c.r.intersects_closest_packed(X(c).o, X(c).d, out=c.packed.float()), V, r"out must be a contiguous int32 \[n, 3\]"),
    (lambda c: c.r.intersects_closest_slots(X(c).o, X(c).d, out=c.slots[:2]), V, r"out must be a contiguous int32 \[n\]"),
    (lambda c: c.r.intersects_closest_slots(X(c).o, X(c).d, out=c.packed[:, 0]), V, r"out must be a contiguous int32 \[n\]"),
    (lambda c: c.r.closest_from_slots(X(c).o, X(c).d, c.slots[:2]), V, r"slots must be a contiguous int32 \[n\]"),
    (lambda c: c.r.closest_from_slots(X(c).o, X(c).d, c.slots.long()), V, "slots must be a contiguous int32"),
    (lambda c: c.r.closest_expand(c.packed[:, :2], slots=True), V, r"packed must be a contiguous int32 \[n, 3\]"),
    (lambda c: c.r.closest_expand(c.packed.cpu(), slots=True), V, "packed must be .* on the GPU"),
    (lambda c: c.r.closest_expand(c.packed.reshape(-1)), V, r"packed must be a contiguous int32 \[n, 3\]"),
    (lambda c: c.r.closest_expand(c.packed.t()), V, "packed must be a contiguous"),
    (lambda c: hops().closest_expand(c.packed, c.r.mesh_vertices.double(), c.r.mesh_faces), V, "vertices must be contiguous float32"),
    (lambda c: hops().closest_expand(c.packed, c.r.mesh_vertices, c.r.mesh_faces.long()), V, "faces contiguous int32"),
    (lambda c: hops().closest_expand(c.packed, c.r.mesh_vertices.cpu(), c.r.mesh_faces.cpu()), V, "packed, vertices and faces must live on the same GPU"),
    (lambda c: c.r.closest_expand(c.packed, batch_shape=(2, 2)), V, "batch_shape .* does not hold 3 rays"),
    (lambda c: c.r.closest_expand(c.packed, batch_shape=(4,), slots=True), V, "batch_shape .* does not hold 3 rays"),
    # ray indices are int32
    (lambda c: hops().intersects_location(c.aw, X(c).o, X(c).d, ray_base=(1 << 31) - 3), V, "int32 ray_idx"),
    (lambda c: hops().compact_closest(torch.zeros(3, dtype=b_, device=c.dev), None, None, None, None, ray_base=1 << 31), V, "int32 ray_idx"),
    # points
    (lambda c: hops().closest_point_native(c.aw, X(c).p.cpu()), V, "points must be a float32 GPU tensor"),
    (lambda c: hops().closest_point_native(c.aw, X(c).p.double()), V, "points must be a float32 GPU tensor"),
    (lambda c: hops().contains_points_native(c.aw, X(c).p.reshape(-1), c.direction, None, None), V, r"points must be .* \[n, 3\]"),
    (lambda c: hops().within_native(c.aw, X(c).p[:, :2], 0.5), V, r"points must be .* \[n, 3\]"),
    (lambda c: hops().within_closest_native(c.aw, X(c).p.cpu().numpy(), 0.5), V, "points must be a float32 GPU tensor"),
    (lambda c: hops().scene_points_any_native(c.sh, c.di, X(c).p.cpu(), c.direction), V, "points must be a float32 GPU tensor"),
    (lambda c: hops().scene_points_list_native(c.sh, c.di, X(c).p.double(), c.direction), V, "points must be a float32 GPU tensor"),
    (lambda c: hops().scene_closest_point_native(c.sh, c.di, X(c).p[:, :2]), V, r"points must be .* \[n, 3\]"),
    # contains_points_native: the direction and the box
    (lambda c: hops().contains_points_native(c.aw, X(c).p, c.direction, c.direction, None), V, "box_lo and box_hi must both be given"),
    (lambda c: hops().contains_points_native(c.aw, X(c).p, c.direction, None, c.direction), V, "box_lo and box_hi must both be given"),
    (lambda c: hops().contains_points_native(c.aw, X(c).p, c.direction[:2], None, None), V, "direction, box_lo and box_hi must be tensors of 3"),
    (lambda c: hops().contains_points_native(c.aw, X(c).p, c.direction, [0, 0, 0], c.direction), V, "direction, box_lo and box_hi must be tensors of 3"),
    (lambda c: hops().scene_points_any_native(c.sh, c.di, X(c).p, c.direction[:2]), V, "direction must be a float32 tensor of three"),
    (lambda c: hops().scene_points_count_native(c.sh, c.di, X(c).p, c.direction.double()), V, "direction must be a float32 tensor of three"),
    (lambda c: hops().scene_points_fill_native(c.sh, c.di, X(c).p, c.direction.cpu(), c.count, c.offsets, 0), V, "direction must be a float32 tensor of three"),
    # bounds and radii of the native entries: dense float32 [n] on the device
    (lambda c: hops().range_any_native(c.aw, X(c).o, X(c).d, tmin=X(c).tmin[:2]), V, "tmin must be None or a contiguous float32"),
    (lambda c: hops().range_closest_native(c.aw, X(c).o, X(c).d, tmax=X(c).tmax.double()), V, "tmax must be None or a contiguous float32"),
    (lambda c: hops().cross_count_native(c.aw, X(c).o, X(c).d, tmin=0.5), V, "tmin must be None or a contiguous float32"),
    (lambda c: hops().scene_any_native(c.sh, c.di, X(c).o, X(c).d, tmax=X(c).tmax.cpu()), V, "tmax must be None or a contiguous float32"),
    (lambda c: hops().scene_cross_count_native(c.sh, c.di, X(c).o, X(c).d, tmin=X(c).tmin.repeat(2)[::2]), V, "tmin must be None or a contiguous"),
    (lambda c: hops().within_native(c.aw, X(c).p, X(c).r[:2]), V, "radius must be a number or a contiguous float32"),
    (lambda c: hops().within_closest_native(c.aw, X(c).p, X(c).r.double()), V, "radius must be a number or a contiguous float32"),
    (lambda c: hops().faces_within_native(c.aw, X(c).p, X(c).r.cpu()), V, "radius must be a number or a contiguous float32"),
    (lambda c: hops().scene_closest_point_native(c.sh, c.di, X(c).p, X(c).r[:2]), V, "max_distance must be a number or a contiguous float32"),
    (lambda c: hops().scene_closest_point_native(c.sh, c.di, X(c).p, X(c).r.cpu()), V, "max_distance must be a number or a contiguous float32"),
    # pairs and triangles of the native entries
    (lambda c: hops().boxes_native(c.aw, X(c).lo.cpu(), X(c).hi), V, "lo must be a float32 GPU tensor"),
    (lambda c: hops().boxes_native(c.aw, X(c).lo, X(c).hi.double()), V, "hi must be a float32 GPU tensor"),
    (lambda c: hops().faces_in_boxes_native(c.aw, X(c).lo, X(c).hi[:2]), V, "lo .* and hi .* must have one shape and one device"),
    (lambda c: hops().planes_native(c.aw, X(c).p[:, :2], X(c).nrm), V, r"origins must be a float32 GPU tensor of shape \[n, 3\]"),
    (lambda c: hops().planes_native(c.aw, X(c).p, X(c).nrm.cpu().numpy()), V, "normals must be a float32 GPU tensor"),
    (lambda c: hops().faces_on_planes_native(c.aw, X(c).p, X(c).nrm[:2]), V, "origins .* and normals .* must have one shape"),
    (lambda c: hops().tris_native(c.aw, X(c).tri.cpu()), V, "triangles must be a float32 GPU tensor"),
    (lambda c: hops().tris_native(c.aw, X(c).tri.reshape(-1, 3)), V, r"triangles must be .* \[n, 3, 3\]"),
    (lambda c: hops().faces_meeting_triangles_native(c.aw, X(c).tri.double()), V, "triangles must be a float32 GPU tensor"),
    # the query strings and the options that need one another
    (lambda c: hops().within_native(c.aw, X(c).p, 0.5, "list"), V, "query must be 'any' or 'count'"),
    (lambda c: hops().boxes_native(c.aw, X(c).lo, X(c).hi, "first"), V, "query must be 'any' or 'count'"),
    (lambda c: hops().tris_native(c.aw, X(c).tri, None), V, "query must be 'any' or 'count'"),
    (lambda c: hops().planes_native(c.aw, X(c).p, X(c).nrm, "cut"), V, "query must be 'any' or 'count'"),
    (lambda c: hops().trace_stats(c.aw, X(c).o, X(c).d, "nearest"), KeyError, "nearest"),
    (lambda c: hops().planes_fill_native(c.aw, X(c).p, X(c).nrm, c.count, c.offsets, 0, cut=False, want_segments=True), V, "want_segments needs cut"),
    (lambda c: hops().faces_on_planes_native(c.aw, X(c).p, X(c).nrm, cut=False, want_segments=True), V, "want_segments needs cut"),
    # RayMeshIntersector: the mesh
    (lambda c: type(c.r)(), V, "Either 'mesh' or 'vertices' and 'faces'"),
    (lambda c: type(c.r)(vertices=VERTICES[:, :2], faces=FACES, device=c.dev), V, r"vertices must have shape \[n, 3\]"),
    (lambda c: type(c.r)(vertices=VERTICES, faces=FACES[:, :2], device=c.dev), V, r"faces must have shape \[f, 3\]"),
    # RayMeshIntersector: points, pairs, triangles, rays and segments as the caller names them
    (lambda c: c.r.closest_point(X(c).p.cpu()), V, "points must reside on a GPU"),
    (lambda c: c.r.within_any(X(c).p[:, :2], 0.5), V, r"points must have shape \[\*b, 3\]"),
    (lambda c: c.r.within_count(torch.tensor(1.0, device=c.dev), 0.5), V, r"points must have shape \[\*b, 3\]"),
    (lambda c: c.r.faces_within(X(c).p.cpu(), 0.5), V, "points must reside on a GPU"),
    (lambda c: c.r.signed_distance(X(c).p.cpu()), V, "points must reside on a GPU"),
    (lambda c: c.r.signed_distance(X(c).p[:, :2]), V, r"points must have shape \[\*b, 3\]"),
    (lambda c: c.r.within_any(X(c).p, X(c).r[:2]), V, "radius of shape .* does not broadcast"),
    (lambda c: c.r.faces_within(X(c).p, [0.5, 0.5]), V, "radius of shape .* does not broadcast"),
    (lambda c: c.r.closest_point(X(c).p, max_distance=X(c).r[:2]), V, "max_distance of shape .* does not broadcast"),
    (lambda c: c.r.boxes_any(X(c).lo.cpu(), X(c).hi), V, "lo must reside on a GPU"),
    (lambda c: c.r.boxes_count(X(c).lo, X(c).hi.cpu()), V, "hi must reside on a GPU"),
    (lambda c: c.r.faces_in_boxes(X(c).lo[:, :2], X(c).hi), V, r"lo must have shape \[\*b, 3\]"),
    (lambda c: c.r.boxes_any(X(c).lo, X(c).hi.reshape(-1)), V, r"hi must have shape \[\*b, 3\]"),
    (lambda c: c.r.boxes_count(X(c).lo, X(c).hi[:2]), V, "lo of shape .* and hi of shape .* do not broadcast"),
    (lambda c: c.r.planes_any(X(c).p.cpu(), X(c).nrm), V, "origins must reside on a GPU"),
    (lambda c: c.r.planes_count(X(c).p, X(c).nrm[:, :2]), V, r"normals must have shape \[\*b, 3\]"),
    (lambda c: c.r.faces_on_planes(X(c).p, X(c).nrm[:2]), V, "origins of shape .* and normals of shape .* do not broadcast"),
    (lambda c: c.r.section_segments(X(c).p, X(c).nrm.cpu()), V, "normals must reside on a GPU"),
    (lambda c: c.r.section_multiplane([0, 0], [0, 0, 1], [0.25]), V, r"origin and normal must have shape \[3\]"),
    (lambda c: c.r.section_multiplane([0, 0, 0], [0, 0, 1], [[0.25]]), V, r"heights \[m\]"),
    (lambda c: c.r.triangles_any(X(c).tri.cpu()), V, "triangles must reside on a GPU"),
    (lambda c: c.r.triangles_count(X(c).tri.reshape(-1, 3)), V, r"triangles must have shape \[\*b, 3, 3\]"),
    (lambda c: c.r.faces_meeting_triangles(X(c).tri[:, :2]), V, r"triangles must have shape \[\*b, 3, 3\]"),
    (lambda c: c.r.mesh_collides(VERTICES, FACES, chunk=0), V, "chunk must be positive"),
    (lambda c: c.r.mesh_contacts(VERTICES[:, :2], FACES), V, r"vertices must have shape \[v, 3\]"),
    (lambda c: c.r.mesh_collides(VERTICES, FACES[:, :2]), V, r"faces must have shape \[m, 3\]"),
    (lambda c: c.r.mesh_contacts(VERTICES, FACES + 2), V, "faces index outside the 4 vertices"),
    (lambda c: c.r.intersects_any_range(X(c).o.cpu(), X(c).d), V, "origins must reside on a GPU"),
    (lambda c: c.r.intersects_closest_range(X(c).o, X(c).d.cpu()), V, "directions must reside on a GPU"),
    (lambda c: c.r.intersects_count_range(X(c).o, X(c).d[:2]), V, "origins and directions must have the same shape"),
    (lambda c: c.r.intersects_all_range(X(c).o[:, :2], X(c).d[:, :2]), V, "origins and directions must have the same shape"),
    (lambda c: c.r.intersects_any_range(X(c).o, X(c).d, tmin=X(c).tmin[:2]), V, "tmin of shape .* does not broadcast"),
    (lambda c: c.r.intersects_all_range(X(c).o, X(c).d, tmax=[1.0, 2.0]), V, "tmax of shape .* does not broadcast"),
    (lambda c: c.r.segments_any(X(c).o.cpu(), X(c).p1), V, "p0 must reside on a GPU"),
    (lambda c: c.r.segments_closest(X(c).o, X(c).p1.cpu()), V, "p1 must reside on a GPU"),
    (lambda c: c.r.segments_count(X(c).o, X(c).p1[:2]), V, "p0 and p1 must have the same shape"),
    (lambda c: c.r.segments_all(X(c).o[:, :2], X(c).p1[:, :2]), V, "p0 and p1 must have the same shape"),
    (lambda c: c.r.surface_voxels(0.0), V, "pitch must be finite and positive"),
    (lambda c: c.r.surface_voxels(0.5, chunk=0), V, "chunk must be positive"),
    (lambda c: c.r.surface_voxels(0.5, origin=[0, 0]), V, "origin must be three finite numbers"),
    (lambda c: c.r.refit(VERTICES[:3]), V, "refit needs the same number of vertices"),
    # RaySceneIntersector: the scene
    (lambda c: type(c.s)([c.r, None], [0], PLACEMENTS[:1]), V, r"meshes\[1\] is not a RayMeshIntersector"),
    (lambda c: type(c.s)([c.r], [[0, 0]], PLACEMENTS), V, r"mesh_of_instance must have shape \[n\]"),
    (lambda c: type(c.s)([c.r], [0.0, 0.5], PLACEMENTS), V, "mesh_of_instance must hold integers"),
    (lambda c: type(c.s)([c.r], [0, 1], PLACEMENTS), V, "mesh_of_instance names a mesh outside"),
    (lambda c: type(c.s)([c.r], [0, 0], PLACEMENTS[:1]), V, "2 instances but 1 transforms"),
    (lambda c: c.s.set_transforms(PLACEMENTS.reshape(2, 12)), V, r"transforms must have shape \[n, 4, 4\] or \[n, 3, 4\]"),
    (lambda c: c.s.set_transforms(np.ones((2, 4, 4), np.float32)), V, "last row"),
    (lambda c: hops().scene_commit(c.sh, [c.aw._inner], [0, 0], PLACEMENTS[:1], c.di), V, "2 instances but 1 transforms"),
    # RaySceneIntersector: rays, segments and points go through the same rules
    (lambda c: c.s.intersects_any(X(c).o.cpu(), X(c).d), V, "origins must reside on a GPU"),
    (lambda c: c.s.intersects_closest(X(c).o, X(c).d[:2]), V, "origins and directions must have the same shape"),
    (lambda c: c.s.intersects_count(X(c).o, X(c).d, tmin=X(c).tmin[:2]), V, "tmin of shape .* does not broadcast"),
    (lambda c: c.s.intersects_all(X(c).o, X(c).d, tmax=[1.0, 2.0]), V, "tmax of shape .* does not broadcast"),
    (lambda c: c.s.segments_any(X(c).o.cpu(), X(c).p1), V, "p0 must reside on a GPU"),
    (lambda c: c.s.segments_closest(X(c).o, X(c).p1[:2]), V, "p0 and p1 must have the same shape"),
    (lambda c: c.s.segments_count(X(c).o, X(c).p1.cpu()), V, "p1 must reside on a GPU"),
    (lambda c: c.s.segments_all(X(c).o[:, :2], X(c).p1[:, :2]), V, "p0 and p1 must have the same shape"),
    (lambda c: c.s.contains_points(X(c).p.cpu()), V, "points must reside on a GPU"),
    (lambda c: c.s.contains_count(X(c).p[:, :2]), V, r"points must have shape \[\*b, 3\]"),
    (lambda c: c.s.containing_instances(X(c).p, check_direction=[0, 1]), V, "check_direction must hold three numbers"),
    (lambda c: c.s.signed_distance(X(c).p.cpu()), V, "points must reside on a GPU"),
    (lambda c: c.s.closest_point(X(c).p[:, :2]), V, r"points must have shape \[\*b, 3\]"),
    (lambda c: c.s.closest_point(X(c).p, max_distance=X(c).r[:2]), V, "max_distance of shape .* does not broadcast"),
    # (new rows go to the end: the ids of the rows above hold their index)
    # RayMeshIntersector.triangles_nearest and mesh_distance, and the native entry under them
    (lambda c: c.r.triangles_nearest(X(c).tri.cpu()), V, "triangles must reside on a GPU"),
    (lambda c: c.r.triangles_nearest(X(c).tri[:, :2]), V, r"triangles must have shape \[\*b, 3, 3\]"),
    (lambda c: c.r.triangles_nearest(X(c).tri.reshape(-1, 9)), V, r"triangles must have shape \[\*b, 3, 3\]"),
    (lambda c: c.r.triangles_nearest(X(c).tri, X(c).r[:2]), V, "max_distance of shape .* does not broadcast"),
    (lambda c: c.r.triangles_nearest(X(c).tri, [0.5, 0.5]), V, "max_distance of shape .* does not broadcast"),
    (lambda c: c.r.mesh_distance(VERTICES, FACES, chunk=0), V, "chunk must be positive"),
    (lambda c: c.r.mesh_distance(VERTICES[:, :2], FACES), V, r"vertices must have shape \[v, 3\]"),
    (lambda c: c.r.mesh_distance(VERTICES, FACES[:, :2]), V, r"faces must have shape \[m, 3\]"),
    (lambda c: c.r.mesh_distance(VERTICES, FACES + 2), V, "faces index outside the 4 vertices"),
    (lambda c: c.r.mesh_distance(VERTICES, FACES - 1), V, "faces index outside the 4 vertices"),
    (lambda c: hops().triangles_nearest_native(c.unbuilt, X(c).tri), R, "has not been built"),
    (lambda c: hops().triangles_nearest_native(c.aw, X(c).tri.cpu()), V, "triangles must be a float32 GPU tensor"),
    (lambda c: hops().triangles_nearest_native(c.aw, X(c).tri.double()), V, "triangles must be a float32 GPU tensor"),
    (lambda c: hops().triangles_nearest_native(c.aw, X(c).tri.reshape(-1, 3)), V, r"triangles must be .* \[n, 3, 3\]"),
    (lambda c: hops().triangles_nearest_native(c.aw, X(c).tri, X(c).r[:2]), V, "max_distance must be a number or a contiguous float32"),
    (lambda c: hops().triangles_nearest_native(c.aw, X(c).tri, X(c).r.cpu()), V, "max_distance must be a number or a contiguous float32"),
    (lambda c: hops().triangles_nearest_native(c.aw, X(c).tri, X(c).r.double()), V, "max_distance must be a number or a contiguous float32"),
    # RaySceneIntersector: triangles and another mesh go through the rules of the mesh class, on the scene's device
    (lambda c: c.s.triangles_any(X(c).tri.cpu()), V, "triangles must reside on a GPU"),
    (lambda c: c.s.triangles_count(X(c).tri.reshape(-1, 3)), V, r"triangles must have shape \[\*b, 3, 3\]"),
    (lambda c: c.s.faces_meeting_triangles(X(c).tri[:, :2]), V, r"triangles must have shape \[\*b, 3, 3\]"),
    (lambda c: c.s.mesh_collides(VERTICES, FACES, chunk=0), V, "chunk must be positive"),
    (lambda c: c.s.colliding_instances(VERTICES, FACES, chunk=-1), V, "chunk must be positive"),
    (lambda c: c.s.mesh_contacts(VERTICES[:, :2], FACES), V, r"vertices must have shape \[v, 3\]"),
    (lambda c: c.s.mesh_collides(VERTICES, FACES[:, :2]), V, r"faces must have shape \[m, 3\]"),
    (lambda c: c.s.mesh_contacts(VERTICES, FACES + 2), V, "faces index outside the 4 vertices"),
    (lambda c: c.s.colliding_instances(VERTICES, FACES - 1), V, "faces index outside the 4 vertices"),
    (lambda c: hops().scene_tris_native(c.sh, c.di, X(c).tri.cpu()), V, "triangles must be a float32 GPU tensor"),
    (lambda c: hops().scene_tris_native(c.sh, c.di, X(c).tri.double(), "count"), V, "triangles must be a float32 GPU tensor"),
    (lambda c: hops().scene_faces_meeting_triangles_native(c.sh, c.di, X(c).tri.reshape(-1, 3)), V, r"triangles must be .* \[n, 3, 3\]"),
    (lambda c: hops().scene_tris_fill_native(c.sh, c.di, X(c).tri[:, :2], c.count, c.offsets, 0), V, r"triangles must be .* \[n, 3, 3\]"),
    (lambda c: hops().scene_tris_native(c.sh, c.di, X(c).tri, "list"), V, "query must be 'any' or 'count'"),
    (lambda c: hops().scene_tris_native(c.sh, c.di, X(c).tri, None), V, "query must be 'any' or 'count'"),
    (lambda c: hops().scene_tris_native(c.sh, c.di + 1, X(c).tri), V, "triangles are on .* but the scene lives on"),
    (lambda c: hops().scene_tris_fill_native(c.sh, c.di + 1, X(c).tri, c.count, c.offsets, 0), V, "triangles are on .* but the scene lives on"),
    (lambda c: hops().scene_tris_native(None, c.di, X(c).tri), V, "scene == NULL"),      # (a scene is built or it has no handle)
]


@pytest.mark.parametrize("row", range(len(REJECTED)), ids=lambda k: f"{k}-{REJECTED[k][2][:40]}")
def test_rejected_arguments(c, row):
    call, exc, fragment = REJECTED[row]
    with pytest.raises(exc, match=fragment):
        call(c)


@pytest.mark.parametrize("bad", ("dtype", "shape", "contiguity", "length"))
@pytest.mark.parametrize("name", ("intersects_closest", "closest_from_slots", "closest_expand_slots", "closest_expand"))
def test_rejected_outs(c, name, bad):
    """`outs` is five contiguous tensors (bool[n], bool[n], int32[n], float32[n,3], float32[n,2]) on the device of the query"""
    outs = list(c.outs())
    c.with_outs[name](tuple(outs))             # what is rejected below is one step from what is accepted
    if bad == "dtype":
        outs[2] = outs[2].long()
    elif bad == "shape":
        outs[3] = outs[3][:2]
    elif bad == "contiguity":
        outs[4] = torch.zeros((2, 3), dtype=f32, device=c.dev).t()
    else:
        outs = outs[:4]
    with pytest.raises(ValueError, match="outs must be contiguous .*bool.*int32.*float32"):
        c.with_outs[name](tuple(outs))


@pytest.mark.parametrize("bad", ("count dtype", "count length", "offsets dtype", "offsets length", "offsets contiguity", "total"))
@pytest.mark.parametrize("family", ("within", "boxes", "tris", "planes", "cross", "scene_cross", "scene_points", "scene_tris"))
def test_rejected_fill_arguments(c, family, bad):
    """every fill takes count int32[n] and offsets int64[n], contiguous on the queries' device, and a total that is not negative"""
    name, args = c.fills[family]
    fill = getattr(hops(), name)
    fill(*args, c.count, c.offsets, 0)         # accepted: nothing to fill
    count, offsets, total = c.count, c.offsets, 0
    if bad == "count dtype":
        count, fragment = count.long(), "count must be a contiguous torch.int32 tensor of 3 elements"
    elif bad == "count length":
        count, fragment = count[:2], "count must be a contiguous torch.int32 tensor of 3 elements"
    elif bad == "offsets dtype":
        offsets, fragment = offsets.int(), "offsets must be a contiguous torch.int64 tensor of 3 elements"
    elif bad == "offsets length":
        offsets, fragment = torch.zeros(4, dtype=i64, device=c.dev), "offsets must be a contiguous torch.int64 tensor of 3 elements"
    elif bad == "offsets contiguity":
        offsets, fragment = torch.zeros(6, dtype=i64, device=c.dev)[::2], "offsets must be a contiguous"
    else:
        total, fragment = -1, "total must not be negative"
    with pytest.raises(ValueError, match=fragment):
        fill(*args, count, offsets, total)


def test_rejected_tensors_of_another_gpu(c):
    """a tensor on a GPU that is not the acceleration structure's (the scene's) is rejected, never moved: only where two GPUs
    are visible"""
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: there is no other device to be on")
    far = torch.device("cuda", (c.dev.index or 0) ^ 1)
    x = X(c)
    F = lambda t: t.to(far)
    rows = [
        (lambda: c.r.intersects_any(F(x.o), x.d), "different devices"),
        (lambda: c.r.intersects_any(F(x.o), F(x.d)), "acceleration structure lives on"),
        (lambda: c.r.intersects_closest_into(x.o, x.d, tuple(F(t) for t in c.outs())), "outs must be contiguous"),
        (lambda: hops().closest_expand(c.packed, F(c.r.mesh_vertices), c.r.mesh_faces), "same GPU"),
        (lambda: hops().scene_any_native(c.sh, c.di, F(x.o), F(x.d)), "rays are on .* but the scene lives on"),
        (lambda: hops().scene_points_any_native(c.sh, c.di, F(x.p), F(c.direction)), "points are on .* but the scene lives on"),
        (lambda: hops().scene_closest_point_native(c.sh, c.di, F(x.p)), "points are on .* but the scene lives on"),
        (lambda: hops().scene_points_any_native(c.sh, c.di, x.p, F(c.direction)), "direction must be"),
        (lambda: hops().range_any_native(c.aw, x.o, x.d, tmin=F(x.tmin)), "tmin must be None or"),
        (lambda: hops().within_native(c.aw, x.p, F(x.r)), "radius must be a number or"),
        (lambda: hops().boxes_native(c.aw, x.lo, F(x.hi)), "one shape and one device"),
        (lambda: hops().boxes_fill_native(c.aw, x.lo, x.hi, F(c.count), c.offsets, 0), "count must be"),
        (lambda: c.r.closest_point(F(x.p)), "points .* on .* but the acceleration structure lives on"),
        (lambda: c.r.within_any(x.p, F(x.r)), "radius is on .* but the acceleration structure lives on"),
        (lambda: c.r.boxes_any(F(x.lo), x.hi), "lo is on .* but the acceleration structure lives on"),
        (lambda: c.r.planes_any(x.p, F(x.nrm)), "normals is on .* but the acceleration structure lives on"),
        (lambda: c.r.triangles_any(F(x.tri)), "triangles is on .* but the acceleration structure lives on"),
        (lambda: c.r.mesh_collides(F(c.r.mesh_vertices), FACES), "vertices is on .* but the acceleration structure lives on"),
        (lambda: c.r.intersects_any_range(F(x.o), F(x.d)), "origins is on .* but the acceleration structure lives on"),
        (lambda: c.r.intersects_any_range(x.o, x.d, tmax=F(x.tmax)), "tmax is on .* but the acceleration structure lives on"),
        (lambda: c.r.segments_any(x.o, F(x.p1)), "p1 is on .* but the acceleration structure lives on"),
        (lambda: c.s.intersects_any(F(x.o), F(x.d)), "origins is on"),
        (lambda: c.s.contains_points(F(x.p)), "points .* on"),
        (lambda: c.r.triangles_nearest(F(x.tri)), "triangles is on .* but the acceleration structure lives on"),
        (lambda: c.r.triangles_nearest(x.tri, F(x.r)), "max_distance is on .* but the acceleration structure lives on"),
        (lambda: c.r.mesh_distance(F(c.r.mesh_vertices), FACES), "vertices is on .* but the acceleration structure lives on"),
        (lambda: hops().triangles_nearest_native(c.aw, x.tri, F(x.r)), "max_distance must be a number or"),
        (lambda: c.s.triangles_any(F(x.tri)), "triangles is on"),
        (lambda: c.s.triangles_count(F(x.tri)), "triangles is on"),
        (lambda: c.s.faces_meeting_triangles(F(x.tri)), "triangles is on"),
        (lambda: c.s.mesh_collides(F(c.r.mesh_vertices), FACES), "vertices is on"),
        (lambda: c.s.mesh_contacts(c.r.mesh_vertices, F(c.r.mesh_faces)), "faces is on"),
        (lambda: c.s.colliding_instances(F(c.r.mesh_vertices), FACES), "vertices is on"),
        (lambda: hops().scene_tris_native(c.sh, c.di, F(x.tri)), "triangles are on .* but the scene lives on"),
        (lambda: hops().scene_tris_fill_native(c.sh, c.di, x.tri, F(c.count), c.offsets, 0), "count must be"),
    ]
    for call, fragment in rows:
        with pytest.raises(ValueError, match=fragment):
            call()


# ---- 2: batch shapes in, batch shapes out -----------------------------------------------------------------------------------
# an output: (dtype, leading shape, trailing shape).  Leading: "B" the batch shape, "N" the number of queries, "N1" that number
# plus one (offsets), "H" the rows of a list (one length per result, the last offset where there are offsets)
def spec(text):
    """"fB3 lN1" -> [(float32, "B", (3,)), (int64, "N1", ())]: a letter for the dtype, the leading shape, the digits of the tail"""
    dtypes = {"b": b_, "i": i32, "l": i64, "f": f32}
    out = []
    for w in text.split():
        lead = "N1" if w[1:3] == "N1" else w[1]
        out.append((dtypes[w[0]], lead, tuple(int(ch) for ch in w[1 + len(lead):])))
    return out


DENSE = "bB bB iB fB3 fB2"
SCENE_DENSE = "bB bB iB iB fB fB3 fB2"
ALL = "lN1 iH fH bH fH3 fH2"
SCENE_ALL = "lN1 iH iH fH bH fH3 fH2"

# (name, the call on (c, x), its outputs)
MESH_QUERIES = [
    ("intersects_any", lambda c, x: c.r.intersects_any(x.o, x.d), "bB"),
    ("intersects_first", lambda c, x: c.r.intersects_first(x.o, x.d), "iB"),
    ("intersects_closest", lambda c, x: c.r.intersects_closest(x.o, x.d), DENSE),
    ("intersects_closest compacted", lambda c, x: c.r.intersects_closest(x.o, x.d, stream_compaction=True), "bB bH iH iH fH3 fH2"),
    ("intersects_closest_into", lambda c, x: c.r.intersects_closest_into(x.o, x.d, flat_outs(c, x)), "bN bN iN fN3 fN2"),
    ("intersects_closest_packed", lambda c, x: c.r.intersects_closest_packed(x.o, x.d), "iN3"),
    ("intersects_closest_packed slots", lambda c, x: c.r.intersects_closest_packed(x.o, x.d, slots=True), "iN3"),
    ("closest_expand", lambda c, x: c.r.closest_expand(c.r.intersects_closest_packed(x.o, x.d), batch_shape=x.bs), DENSE),
    ("closest_expand flat", lambda c, x: c.r.closest_expand(c.r.intersects_closest_packed(x.o, x.d)), "bN bN iN fN3 fN2"),
    ("closest_expand into", lambda c, x: c.r.closest_expand(c.r.intersects_closest_packed(x.o, x.d), outs=flat_outs(c, x)), "bN bN iN fN3 fN2"),
    ("closest_expand slots", lambda c, x: c.r.closest_expand(c.r.intersects_closest_packed(x.o, x.d, slots=True), batch_shape=x.bs, slots=True), DENSE),
    ("closest_expand slots into", lambda c, x: c.r.closest_expand(c.r.intersects_closest_packed(x.o, x.d, slots=True), outs=flat_outs(c, x), slots=True),
     "bN bN iN fN3 fN2"),
    ("intersects_closest_slots", lambda c, x: c.r.intersects_closest_slots(x.o, x.d), "iN"),
    ("closest_from_slots", lambda c, x: c.r.closest_from_slots(x.o, x.d, c.r.intersects_closest_slots(x.o, x.d)), DENSE),
    ("closest_from_slots into", lambda c, x: c.r.closest_from_slots(x.o, x.d, c.r.intersects_closest_slots(x.o, x.d), outs=flat_outs(c, x)),
     "bN bN iN fN3 fN2"),
    ("intersects_location", lambda c, x: c.r.intersects_location(x.o, x.d), "fH3 iH iH"),
    ("intersects_location two passes", lambda c, x: hops().intersects_location(c.aw, x.o, x.d, fused=False), "fH3 iH iH"),
    ("intersects_count", lambda c, x: c.r.intersects_count(x.o, x.d), "iB"),
    ("intersects_id", lambda c, x: c.r.intersects_id(x.o, x.d), "iH iH"),
    ("intersects_id locations", lambda c, x: c.r.intersects_id(x.o, x.d, return_locations=True), "iH iH fH3"),
    ("intersects_id first", lambda c, x: c.r.intersects_id(x.o, x.d, multiple_hits=False), "iH iH"),
    ("intersects_id first locations", lambda c, x: c.r.intersects_id(x.o, x.d, return_locations=True, multiple_hits=False), "iH iH fH3"),
    ("contains_points", lambda c, x: c.r.contains_points(x.p.reshape(-1, 3)), "bN"),         # (points must be [n, 3]: the reference's quirk)
    ("contains_points direction", lambda c, x: c.r.contains_points(x.p.reshape(-1, 3), c.direction), "bN"),
    ("closest_point", lambda c, x: c.r.closest_point(x.p), "fB3 fB iB"),
    ("closest_point number", lambda c, x: c.r.closest_point(x.p, max_distance=0.5), "fB3 fB iB"),
    ("closest_point tensor", lambda c, x: c.r.closest_point(x.p, max_distance=x.r), "fB3 fB iB"),
    ("within_any", lambda c, x: c.r.within_any(x.p, 0.5), "bB"),
    ("within_any tensor", lambda c, x: c.r.within_any(x.p, x.r), "bB"),
    ("within_count", lambda c, x: c.r.within_count(x.p, 0.5), "iB"),
    ("faces_within", lambda c, x: c.r.faces_within(x.p, 0.5), "lN1 iH"),
    ("faces_within all", lambda c, x: c.r.faces_within(x.p, x.r, return_distance=True, return_closest=True), "lN1 iH fH fH3"),
    ("faces_within closest", lambda c, x: c.r.faces_within(x.p, 0.5, return_closest=True), "lN1 iH fH3"),
    ("boxes_any", lambda c, x: c.r.boxes_any(x.lo, x.hi), "bB"),
    ("boxes_count", lambda c, x: c.r.boxes_count(x.lo, x.hi), "iB"),
    ("faces_in_boxes", lambda c, x: c.r.faces_in_boxes(x.lo, x.hi), "lN1 iH"),
    ("faces_in_boxes inside", lambda c, x: c.r.faces_in_boxes(x.lo, x.hi, return_inside=True), "lN1 iH bH"),
    ("planes_any", lambda c, x: c.r.planes_any(x.p, x.nrm), "bB"),
    ("planes_count", lambda c, x: c.r.planes_count(x.p, x.nrm), "iB"),
    ("planes_count cut", lambda c, x: c.r.planes_count(x.p, x.nrm, cut=True), "iB"),
    ("faces_on_planes", lambda c, x: c.r.faces_on_planes(x.p, x.nrm), "lN1 iH"),
    ("faces_on_planes cut", lambda c, x: c.r.faces_on_planes(x.p, x.nrm, cut=True), "lN1 iH"),
    ("section_segments", lambda c, x: c.r.section_segments(x.p, x.nrm), "lN1 iH fH23"),
    ("section_multiplane", lambda c, x: c.r.section_multiplane([0, 0, 0], [0, 0, 1], x.r.reshape(-1)), "lN1 iH fH23"),
    ("triangles_any", lambda c, x: c.r.triangles_any(x.tri), "bB"),
    ("triangles_count", lambda c, x: c.r.triangles_count(x.tri), "iB"),
    ("faces_meeting_triangles", lambda c, x: c.r.faces_meeting_triangles(x.tri), "lN1 iH"),
    ("triangles_nearest", lambda c, x: c.r.triangles_nearest(x.tri), "iB fB fB3 fB3"),
    ("triangles_nearest number", lambda c, x: c.r.triangles_nearest(x.tri, 0.5), "iB fB fB3 fB3"),
    ("triangles_nearest tensor", lambda c, x: c.r.triangles_nearest(x.tri, max_distance=x.r), "iB fB fB3 fB3"),
    ("signed_distance", lambda c, x: c.r.signed_distance(x.p), "fB"),
    ("intersects_any_range", lambda c, x: c.r.intersects_any_range(x.o, x.d), "bB"),
    ("intersects_any_range bounds", lambda c, x: c.r.intersects_any_range(x.o, x.d, x.tmin, x.tmax), "bB"),
    ("intersects_any_range numbers", lambda c, x: c.r.intersects_any_range(x.o, x.d, 0.5, 8), "bB"),
    ("intersects_closest_range", lambda c, x: c.r.intersects_closest_range(x.o, x.d, x.tmin, 8.0), DENSE + " fB"),
    ("intersects_count_range", lambda c, x: c.r.intersects_count_range(x.o, x.d, None, x.tmax), "iB"),
    ("intersects_all_range", lambda c, x: c.r.intersects_all_range(x.o, x.d, x.tmin, x.tmax), "lN1 iH fH"),
    ("intersects_all_range all", lambda c, x: c.r.intersects_all_range(x.o, x.d, 0.5, None, True, True, True), ALL),
    ("segments_any", lambda c, x: c.r.segments_any(x.o, x.p1), "bB"),
    ("segments_closest", lambda c, x: c.r.segments_closest(x.o, x.p1), DENSE + " fB"),
    ("segments_count", lambda c, x: c.r.segments_count(x.o, x.p1), "iB"),
    ("segments_all", lambda c, x: c.r.segments_all(x.o, x.p1), "lN1 iH fH"),
    ("segments_all all", lambda c, x: c.r.segments_all(x.o, x.p1, True, True, True), ALL),
]
SCENE_QUERIES = [
    ("intersects_any", lambda c, x: c.s.intersects_any(x.o, x.d), "bB"),
    ("intersects_any bounds", lambda c, x: c.s.intersects_any(x.o, x.d, x.tmin, 8.0), "bB"),
    ("intersects_closest", lambda c, x: c.s.intersects_closest(x.o, x.d, None, x.tmax), SCENE_DENSE),
    ("segments_any", lambda c, x: c.s.segments_any(x.o, x.p1), "bB"),
    ("segments_closest", lambda c, x: c.s.segments_closest(x.o, x.p1), SCENE_DENSE),
    ("intersects_count", lambda c, x: c.s.intersects_count(x.o, x.d, x.tmin, x.tmax), "iB"),
    ("intersects_all", lambda c, x: c.s.intersects_all(x.o, x.d), "lN1 iH iH fH"),
    ("intersects_all all", lambda c, x: c.s.intersects_all(x.o, x.d, x.tmin, 8, True, True, True), SCENE_ALL),
    ("segments_count", lambda c, x: c.s.segments_count(x.o, x.p1), "iB"),
    ("segments_all", lambda c, x: c.s.segments_all(x.o, x.p1), "lN1 iH iH fH"),
    ("segments_all all", lambda c, x: c.s.segments_all(x.o, x.p1, True, True, True), SCENE_ALL),
    ("contains_points", lambda c, x: c.s.contains_points(x.p), "bB"),
    ("contains_points direction", lambda c, x: c.s.contains_points(x.p, c.direction), "bB"),
    ("contains_count", lambda c, x: c.s.contains_count(x.p), "iB"),
    ("containing_instances", lambda c, x: c.s.containing_instances(x.p, [0.0, 0.0, 1.0]), "lN1 iH"),
    ("closest_point", lambda c, x: c.s.closest_point(x.p), "fB3 fB iB iB"),
    ("closest_point number", lambda c, x: c.s.closest_point(x.p, max_distance=0.5), "fB3 fB iB iB"),
    ("closest_point tensor", lambda c, x: c.s.closest_point(x.p, max_distance=x.r), "fB3 fB iB iB"),
    ("signed_distance", lambda c, x: c.s.signed_distance(x.p), "fB"),
    ("triangles_any", lambda c, x: c.s.triangles_any(x.tri), "bB"),
    ("triangles_count", lambda c, x: c.s.triangles_count(x.tri), "iB"),
    ("faces_meeting_triangles", lambda c, x: c.s.faces_meeting_triangles(x.tri), "lN1 iH iH"),
]


def flat_outs(c, x):
    return (torch.zeros(x.n, dtype=b_, device=c.dev), torch.zeros(x.n, dtype=b_, device=c.dev), torch.zeros(x.n, dtype=i32, device=c.dev),
            torch.zeros((x.n, 3), dtype=f32, device=c.dev), torch.zeros((x.n, 2), dtype=f32, device=c.dev))


def check_shapes(name, out, outputs, x, dev):
    out = out if isinstance(out, tuple) else (out,)
    want = spec(outputs)
    assert len(out) == len(want), f"{name}: {len(out)} outputs, {len(want)} documented"
    rows = None
    for k, (t, (dtype, lead, tail)) in enumerate(zip(out, want)):
        what = f"{name}, batch shape {x.bs}, output {k}"
        assert isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype, f"{what}: {t.dtype} on {t.device}"
        if lead == "H":
            rows = t.shape[0] if rows is None else rows
            assert tuple(t.shape) == (rows, *tail), f"{what}: shape {tuple(t.shape)}, {(rows, *tail)} expected"
        else:
            shape = {"B": (*x.bs, *tail), "N": (x.n, *tail), "N1": (x.n + 1,)}[lead]
            assert tuple(t.shape) == shape, f"{what}: shape {tuple(t.shape)}, {shape} expected"
    if want[0][1] == "N1":
        assert int(out[0][0]) == 0 and int(out[0][-1]) == rows, f"{name}, batch shape {x.bs}: offsets {out[0].tolist()} for {rows} rows"
    if x.n == 0:
        assert all(t.numel() == 0 for t in out[1 if want[0][1] == "N1" else 0:]), f"{name}: an empty batch returned something"


def test_the_specs_read_as_written():
    assert spec("bB fH23 lN1 iN3") == [(b_, "B", ()), (f32, "H", (2, 3)), (i64, "N1", ()), (i32, "N", (3,))]


@pytest.mark.parametrize("bs", BATCHES, ids=str)
def test_mesh_queries_return_the_documented_shapes(c, bs):
    for name, call, outputs in MESH_QUERIES:
        check_shapes(name, call(c, c.x[bs]), outputs, c.x[bs], c.dev)


@pytest.mark.parametrize("bs", BATCHES, ids=str)
def test_scene_queries_return_the_documented_shapes(c, bs):
    for name, call, outputs in SCENE_QUERIES:
        check_shapes(name, call(c, c.x[bs]), outputs, c.x[bs], c.dev)


@pytest.mark.parametrize("bs", BATCHES, ids=str)
def test_mesh_against_mesh_queries_return_the_documented_shapes(c, bs):
    """the other mesh has one face per query triangle of the batch shape (none for (0,)): what comes back does not have the
    batch shape but scalars and rows"""
    x = c.x[bs]
    v, f = x.tri.reshape(3 * x.n, 3), torch.arange(3 * x.n, device=c.dev).reshape(x.n, 3)
    d, other, own, on_other, on_self = c.r.mesh_distance(v, f)
    assert all(t.device == c.dev for t in (d, other, own, on_other, on_self))
    assert d.dtype == f32 and d.shape == () and other.dtype == own.dtype == i64 and other.shape == own.shape == ()
    assert on_other.dtype == on_self.dtype == f32 and on_other.shape == on_self.shape == (3,)
    assert (int(other) == -1 and int(own) == -1 and bool(torch.isinf(d))) if x.n == 0 else (0 <= int(other) < x.n and 0 <= int(own) < len(FACES))
    for r in (c.r, c.s):
        assert isinstance(r.mesh_collides(v, f), bool) and (x.n > 0 or not r.mesh_collides(v, f))
    rows, hit = c.s.mesh_contacts(v, f), c.s.colliding_instances(v, f)
    assert rows.dtype == hit.dtype == i64 and rows.device == hit.device == c.dev and rows.dim() == 2 and rows.shape[1] == 3 and hit.dim() == 1
    assert x.n > 0 or (rows.shape[0] == 0 and hit.shape[0] == 0)
    assert torch.equal(hit, torch.unique(rows[:, 1]))


def test_the_optional_columns_come_in_their_order(c):
    """front, loc and uv: each present exactly when asked for, after the fixed columns, in this order"""
    x = X(c)
    columns = ("bH", "fH3", "fH2")
    for flags in itertools.product((False, True), repeat=3):
        tail = " ".join(col for col, on in zip(columns, flags) if on)
        check_shapes(f"intersects_all_range{flags}", c.r.intersects_all_range(x.o, x.d, None, None, *flags), "lN1 iH fH " + tail, x, c.dev)
        check_shapes(f"segments_all{flags}", c.r.segments_all(x.o, x.p1, *flags), "lN1 iH fH " + tail, x, c.dev)
        check_shapes(f"scene.intersects_all{flags}", c.s.intersects_all(x.o, x.d, None, None, *flags), "lN1 iH iH fH " + tail, x, c.dev)
        check_shapes(f"scene.segments_all{flags}", c.s.segments_all(x.o, x.p1, *flags), "lN1 iH iH fH " + tail, x, c.dev)
    for flags in itertools.product((False, True), repeat=2):
        tail = " ".join(col for col, on in zip(("fH", "fH3"), flags) if on)
        check_shapes(f"faces_within{flags}", c.r.faces_within(x.p, 0.5, *flags), "lN1 iH " + tail, x, c.dev)


def test_the_batch_shape_does_not_change_the_answers(c):
    """(2, 2) is the same four queries as (4,): the outputs are reshapes of one another"""
    x = c.x[(2, 2)]
    flat = SimpleNamespace(bs=(4,), n=4, **{k: v.reshape(4, *v.shape[2:]) for k, v in vars(x).items() if isinstance(v, torch.Tensor)})
    for name, call, outputs in MESH_QUERIES + SCENE_QUERIES:
        a, b = call(c, x), call(c, flat)
        for s, t in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert same(s.reshape(t.shape), t), name


# ---- 3: array-like inputs ---------------------------------------------------------------------------------------------------
def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# where lists and numpy arrays are accepted today: (name, the call on (c, K, x); K converts an argument)
ARRAY_LIKE = [
    ("closest_point", lambda c, K, x: c.r.closest_point(K(x.p))),
    ("closest_point bounded", lambda c, K, x: c.r.closest_point(K(x.p), max_distance=K(x.r))),
    ("within_any", lambda c, K, x: c.r.within_any(K(x.p), K(x.r))),
    ("within_count", lambda c, K, x: c.r.within_count(K(x.p), 0.5)),
    ("faces_within", lambda c, K, x: c.r.faces_within(K(x.p), K(x.r), True, True)),
    ("boxes_any", lambda c, K, x: c.r.boxes_any(K(x.lo), K(x.hi))),
    ("boxes_count", lambda c, K, x: c.r.boxes_count(K(x.lo), x.hi)),
    ("faces_in_boxes", lambda c, K, x: c.r.faces_in_boxes(x.lo, K(x.hi), True)),
    ("planes_any", lambda c, K, x: c.r.planes_any(K(x.p), K(x.nrm))),
    ("planes_count", lambda c, K, x: c.r.planes_count(K(x.p), [0, 0, 1], cut=True)),
    ("faces_on_planes", lambda c, K, x: c.r.faces_on_planes(K(x.p), K(x.nrm))),
    ("section_segments", lambda c, K, x: c.r.section_segments(K(x.p), K(x.nrm))),
    ("section_multiplane", lambda c, K, x: c.r.section_multiplane(K(x.p[0]), K(x.nrm[0]), K(x.r))),
    ("triangles_any", lambda c, K, x: c.r.triangles_any(K(x.tri))),
    ("triangles_count", lambda c, K, x: c.r.triangles_count(K(x.tri))),
    ("faces_meeting_triangles", lambda c, K, x: c.r.faces_meeting_triangles(K(x.tri))),
    ("mesh_collides", lambda c, K, x: torch.tensor(c.r.mesh_collides(K(x.tri.reshape(-1, 3)), [[0, 1, 2], [3, 4, 5], [6, 7, 8]]))),
    ("mesh_contacts", lambda c, K, x: c.r.mesh_contacts(K(x.tri.reshape(-1, 3)), np.arange(9).reshape(3, 3))),
    ("signed_distance", lambda c, K, x: c.r.signed_distance(K(x.p))),
    ("triangles_nearest", lambda c, K, x: c.r.triangles_nearest(K(x.tri), K(x.r))),
    ("mesh_distance", lambda c, K, x: c.r.mesh_distance(K(x.tri.reshape(-1, 3)), np.arange(9).reshape(3, 3))),
    ("intersects_any_range", lambda c, K, x: c.r.intersects_any_range(K(x.o), K(x.d), K(x.tmin), K(x.tmax))),
    ("intersects_closest_range", lambda c, K, x: c.r.intersects_closest_range(K(x.o), K(x.d), 0.5, K(x.tmax))),
    ("intersects_count_range", lambda c, K, x: c.r.intersects_count_range(K(x.o), x.d, K(x.tmin))),
    ("intersects_all_range", lambda c, K, x: c.r.intersects_all_range(x.o, K(x.d), None, K(x.tmax), True, True, True)),
    ("segments_any", lambda c, K, x: c.r.segments_any(K(x.o), K(x.p1))),
    ("segments_closest", lambda c, K, x: c.r.segments_closest(K(x.o), K(x.p1))),
    ("segments_count", lambda c, K, x: c.r.segments_count(K(x.o), K(x.p1))),
    ("segments_all", lambda c, K, x: c.r.segments_all(K(x.o), K(x.p1), True, True, True)),
    ("scene.intersects_any", lambda c, K, x: c.s.intersects_any(K(x.o), K(x.d), K(x.tmin), K(x.tmax))),
    ("scene.intersects_closest", lambda c, K, x: c.s.intersects_closest(K(x.o), K(x.d))),
    ("scene.intersects_count", lambda c, K, x: c.s.intersects_count(K(x.o), K(x.d), None, K(x.tmax))),
    ("scene.intersects_all", lambda c, K, x: c.s.intersects_all(K(x.o), K(x.d), K(x.tmin), None, True, True, True)),
    ("scene.segments_any", lambda c, K, x: c.s.segments_any(K(x.o), K(x.p1))),
    ("scene.segments_closest", lambda c, K, x: c.s.segments_closest(K(x.o), K(x.p1))),
    ("scene.segments_count", lambda c, K, x: c.s.segments_count(K(x.o), K(x.p1))),
    ("scene.segments_all", lambda c, K, x: c.s.segments_all(K(x.o), K(x.p1), True, True, True)),
    ("scene.contains_points", lambda c, K, x: c.s.contains_points(K(x.p), K(c.direction))),
    ("scene.contains_count", lambda c, K, x: c.s.contains_count(K(x.p))),
    ("scene.containing_instances", lambda c, K, x: c.s.containing_instances(K(x.p), K(c.direction))),
    ("scene.closest_point", lambda c, K, x: c.s.closest_point(K(x.p), max_distance=K(x.r))),
    ("scene.signed_distance", lambda c, K, x: c.s.signed_distance(K(x.p), K(c.direction))),
    ("scene.triangles_any", lambda c, K, x: c.s.triangles_any(K(x.tri))),
    ("scene.triangles_count", lambda c, K, x: c.s.triangles_count(K(x.tri))),
    ("scene.faces_meeting_triangles", lambda c, K, x: c.s.faces_meeting_triangles(K(x.tri))),
    ("scene.mesh_collides", lambda c, K, x: torch.tensor(c.s.mesh_collides(K(x.tri.reshape(-1, 3)), [[0, 1, 2], [3, 4, 5], [6, 7, 8]]))),
    ("scene.mesh_contacts", lambda c, K, x: c.s.mesh_contacts(K(x.tri.reshape(-1, 3)), np.arange(9).reshape(3, 3))),
    ("scene.colliding_instances", lambda c, K, x: c.s.colliding_instances(K(x.tri.reshape(-1, 3)), np.arange(9).reshape(3, 3))),
]
CONVERSIONS = {"list": lambda t: t.cpu().tolist(), "float64 array": lambda t: t.cpu().numpy().astype(np.float64),
               "float64 tensor on the GPU": lambda t: t.double(), "float32 array": lambda t: t.cpu().numpy()}


@pytest.mark.parametrize("bs", ((3,), (2, 2)), ids=str)
@pytest.mark.parametrize("how", CONVERSIONS)
def test_array_likes_give_what_the_gpu_tensor_gives(c, how, bs):
    x = c.x[bs]
    for name, call in ARRAY_LIKE:
        if bs != (3,) and name in ("section_multiplane", "mesh_collides", "mesh_contacts"):
            continue                                   # (their arguments have no batch shape)
        want, got = call(c, lambda t: t, x), call(c, CONVERSIONS[how], x)
        want, got = (want if isinstance(want, tuple) else (want,)), (got if isinstance(got, tuple) else (got,))
        assert len(want) == len(got) and all(same(a, b) for a, b in zip(want, got)), f"{name} on a {how}"


def test_a_mesh_given_as_lists_is_the_mesh_given_as_tensors(c):
    r = type(c.r)(vertices=VERTICES.tolist(), faces=FACES.tolist(), device=c.dev)
    x = X(c)
    assert r.mesh_vertices.dtype == f32 and r.mesh_faces.dtype == i32 and r.mesh_vertices.device == c.dev
    for a, b in zip(r.intersects_closest(x.o, x.d), c.r.intersects_closest(x.o, x.d)):
        assert same(a, b)


# ---- 4: strided rays --------------------------------------------------------------------------------------------------------
def strided(t):
    """two views of the values of t [n, 3] that are not contiguous: a transposed one and every other row of a longer one"""
    transposed = t.t().contiguous().t()
    longer = torch.zeros((2 * t.shape[0], 3), dtype=t.dtype, device=t.device)
    longer[::2] = t
    assert not transposed.is_contiguous() and not longer[::2].is_contiguous()
    return transposed, longer[::2]


def test_strided_rays_are_taken_as_they_are(c):
    """float32 rays keep their strides down to make_rays: no copy is made of them, and the answer is that of the copy"""
    x = X(c)
    seen = []
    original = hops().make_rays
    hops().make_rays = lambda o, d: (seen.append((o.stride(), d.stride())), original(o, d))[1]
    try:
        for o, d in zip(strided(x.o), strided(x.d)):
            for call in (lambda o, d: c.r.intersects_any_range(o, d, x.tmin, x.tmax), lambda o, d: c.s.intersects_any(o, d, x.tmin, x.tmax),
                         lambda o, d: c.r.intersects_closest_range(o, d), lambda o, d: c.s.intersects_closest(o, d),
                         lambda o, d: c.r.intersects_count_range(o, d), lambda o, d: c.s.intersects_count(o, d),
                         lambda o, d: c.r.intersects_all_range(o, d, None, None, True, True, True),
                         lambda o, d: c.s.intersects_all(o, d, None, None, True, True, True),
                         lambda o, d: c.r.intersects_any(o, d), lambda o, d: c.r.intersects_closest(o, d)):
                del seen[:]
                got = call(o, d)
                assert seen and all(s == (o.stride(), d.stride()) for s in seen), seen
                want = call(o.contiguous(), d.contiguous())
                got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
                assert all(same(a, b) for a, b in zip(got, want))
    finally:
        hops().make_rays = original
