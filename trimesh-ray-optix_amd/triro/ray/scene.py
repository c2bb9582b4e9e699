"""RaySceneIntersector -- ray queries over placed copies of several meshes (libtriro_scene.so, include/triro_scene.h).

A scene holds references to RayMeshIntersector members and a list of instances: a member index and a placement, object
to world, any invertible affine map.  One BVH serves every copy of a member, and moving an object is a commit of twelve
floats, not a rebuild.  Distances are the world ray's own parameter (an affine map preserves it), so the answer is the
minimum over the instances of the range query on the transformed ray: csrc/tr_scene.h has the contract.  Point and triangle
queries (closest_point, triangles_any, mesh_contacts, ...) walk the members as they are and place what they meet into world space.

Not in the reference (which has one mesh in one coordinate system): what OptiX answers with instance acceleration
structures."""
from __future__ import annotations

import numpy as np
import torch

import triro.backend.ops as hops
from triro.ray.ray_optix import (RayMeshIntersector, _default_device, _flat_queries, _other_triangles, _query_bound, _range_rays,
                                 _segment_rays, _with_columns)


def _transforms(transforms) -> np.ndarray:
    """[n, 4, 4] (last row 0 0 0 1) or [n, 3, 4], a tensor or an array -> float32 [n, 12] on the host"""
    t = transforms.detach().cpu().numpy() if isinstance(transforms, torch.Tensor) else np.asarray(transforms)
    if t.size == 0 and t.ndim <= 1:
        t = t.reshape(0, 3, 4)
    if t.ndim != 3 or t.shape[1:] not in ((4, 4), (3, 4)):
        raise ValueError(f"transforms must have shape [n, 4, 4] or [n, 3, 4], got {tuple(t.shape)}")
    if t.shape[1] == 4:
        if not (t[:, 3, :] == np.array([0, 0, 0, 1], t.dtype)).all():
            raise ValueError("the last row of every [4, 4] transform must be 0 0 0 1 (placements are affine maps)")
        t = t[:, :3, :]
    return np.ascontiguousarray(t, np.float32).reshape(-1, 12)


class RaySceneIntersector:
    """RaySceneIntersector(meshes, mesh_of_instance, transforms): `meshes` a list of RayMeshIntersector on one GPU (held by
    reference), instance k places meshes[mesh_of_instance[k]] by transforms[k] (object -> world)."""

    def __init__(self, meshes, mesh_of_instance, transforms):
        self.meshes = list(meshes)
        for k, m in enumerate(self.meshes):
            if not isinstance(m, RayMeshIntersector):
                raise ValueError(f"meshes[{k}] is not a RayMeshIntersector")
        # (no mesh at all is a scene too, as for the C entries: it has no instance and every ray misses)
        self.device = self.meshes[0].mesh_vertices.device if self.meshes else _default_device()
        for k, m in enumerate(self.meshes):
            if m.mesh_vertices.device != self.device:
                raise ValueError(f"meshes[{k}] lives on {m.mesh_vertices.device}, meshes[0] on {self.device}: a scene is on one device")
        mesh_of = mesh_of_instance.detach().cpu().numpy() if isinstance(mesh_of_instance, torch.Tensor) else np.asarray(mesh_of_instance)
        if mesh_of.ndim != 1 and mesh_of.size:
            raise ValueError(f"mesh_of_instance must have shape [n], got {tuple(mesh_of.shape)}")
        mesh_of = mesh_of.reshape(-1)
        if mesh_of.size and not np.issubdtype(mesh_of.dtype, np.integer):
            raise ValueError("mesh_of_instance must hold integers")
        if mesh_of.size and (mesh_of.min() < 0 or mesh_of.max() >= len(self.meshes)):
            raise ValueError(f"mesh_of_instance names a mesh outside [0, {len(self.meshes)})")
        self.mesh_of_instance = mesh_of.astype(np.int32)
        self.transforms = np.zeros((0, 12), np.float32)
        self._handle = None
        self._handle = hops.scene_create(self.device.index)
        self.set_transforms(transforms)

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                hops.scene_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    # -- the scene ---------------------------------------------------------------------------
    def set_transforms(self, transforms):
        """New placements for the same instances ([n, 4, 4] or [n, 3, 4]) and a commit: no member is rebuilt."""
        M = _transforms(transforms)
        if len(M) != len(self.mesh_of_instance):
            raise ValueError(f"{len(self.mesh_of_instance)} instances but {len(M)} transforms")
        self._commit(M)
        self.transforms = M      # (only now: a commit that raised leaves the object with the placements the native scene has)

    def _commit(self, M):
        hops.scene_commit(self._handle, [m.as_wrapper._inner for m in self.meshes], self.mesh_of_instance, M, self.device.index)

    def commit(self):
        """Read the members' acceleration structures again and upload the scene's table.  Needed after a member's
        update_raw (or anything else that moves its arrays: include/triro_scene.h); a member's refit needs none."""
        self._commit(self.transforms)

    def info(self) -> dict:
        return hops.scene_info(self._handle)

    # -- queries -----------------------------------------------------------------------------
    def _rays(self, origins, directions, tmin, tmax):
        return _range_rays(origins, directions, tmin, tmax, self.device)

    def intersects_any(self, origins, directions, tmin=None, tmax=None) -> torch.Tensor:
        """Bool[*b]: does the world ray hit any instance at a distance t (P = o + t d) with tmin <= t <= tmax.  The interval
        is closed, distances are measured from the origin given.  tmin / tmax: None (0 / 1e7), a scalar or anything that
        broadcasts to [*b]."""
        o, d, lo, hi = self._rays(origins, directions, tmin, tmax)
        return hops.scene_any_native(self._handle, self.device.index, o, d, lo, hi)

    def intersects_closest(self, origins, directions, tmin=None, tmax=None):
        """(hit[*b], front[*b], instance[*b], tri[*b], t[*b], loc[*b,3], uv[*b,2]): the first hit with tmin <= t <= tmax over
        all instances -- the one that minimises (t, instance, face).  tri is the face index in the member mesh, loc is in
        world space, uv in object space, front what the placed triangle looks like from the ray.  A miss: False, False,
        -1, -1, +Inf, 0, 0."""
        o, d, lo, hi = self._rays(origins, directions, tmin, tmax)
        return hops.scene_closest_native(self._handle, self.device.index, o, d, lo, hi)

    def segments_any(self, p0, p1) -> torch.Tensor:
        """Bool[*b]: is the segment from p0 to p1 blocked by any instance: the ray (p0, the float32 p1 - p0) on [0, 1]."""
        o, d, one = _segment_rays(p0, p1, self.device)
        return hops.scene_any_native(self._handle, self.device.index, o, d, None, one)

    def segments_closest(self, p0, p1):
        """The tuple of intersects_closest for the segment from p0 to p1; t is the fraction along it."""
        o, d, one = _segment_rays(p0, p1, self.device)
        return hops.scene_closest_native(self._handle, self.device.index, o, d, None, one)

    # -- every crossing within a range (libtriro_scene_cross.so, include/triro_scene_cross.h) ---------------------------
    def intersects_count(self, origins, directions, tmin=None, tmax=None) -> torch.Tensor:
        """int32[*b]: how many (instance, triangle) pairs the world ray crosses at a distance t with tmin <= t <= tmax,
        uncapped.  The interval, its ends and the rays are those of intersects_any; count > 0 is its answer."""
        o, d, lo, hi = self._rays(origins, directions, tmin, tmax)
        return hops.scene_cross_count_native(self._handle, self.device.index, o, d, lo, hi)

    def _all(self, o, d, lo, hi, return_front, return_locations, return_uv):
        offsets, inst, face, t, front, loc, uv, _ = hops.scene_cross_all_native(self._handle, self.device.index, o, d, lo, hi, return_front,
                                                                               return_locations, return_uv)
        return _with_columns((offsets, inst, face, t), (return_front, front), (return_locations, loc), (return_uv, uv))

    def intersects_all(self, origins, directions, tmin=None, tmax=None, return_front=False, return_locations=False, return_uv=False):
        """(offsets int64[n + 1], instance int32[h], tri_idx int32[h], t float32[h][, front bool[h]][, loc float32[h, 3]]
        [, uv float32[h, 2]]) for the rays flattened in order: EVERY crossing of ray i with tmin <= t <= tmax over all
        instances is a row of offsets[i]:offsets[i + 1], ordered by (t, instance, triangle index) ascending, uncapped.
        tri_idx is the face index in the member mesh; front, loc (world space) and uv (object space) are intersects_closest's
        values for that (ray, instance, triangle), and the first row of a ray is its answer.  One count launch, one scan, one
        host read of the total to size the outputs, one fill (two launches): RayMeshIntersector.intersects_all_range on a
        scene."""
        o, d, lo, hi = self._rays(origins, directions, tmin, tmax)
        return self._all(o, d, lo, hi, return_front, return_locations, return_uv)

    def segments_count(self, p0, p1) -> torch.Tensor:
        """int32[*b]: how many (instance, triangle) pairs the segment from p0 to p1 crosses: the ray (p0, the float32
        p1 - p0) on the closed interval [0, 1], as segments_any."""
        o, d, one = _segment_rays(p0, p1, self.device)
        return hops.scene_cross_count_native(self._handle, self.device.index, o, d, None, one)

    def segments_all(self, p0, p1, return_front=False, return_locations=False, return_uv=False):
        """intersects_all for the segments from p0 to p1; t is the fraction along the segment."""
        o, d, one = _segment_rays(p0, p1, self.device)
        return self._all(o, d, None, one, return_front, return_locations, return_uv)

    # -- which instances hold a point (libtriro_scene_points.so, include/triro_scene_points.h) ------------------------------
    def _points(self, points, check_direction):
        """points [*b, 3] and the direction as the native entries take them: (flat float32 [n, 3] on the scene's GPU, float32
        [3] there, the batch shape).  Conversion and device rules for the points are those of the box queries of
        RayMeshIntersector; check_direction is None (the reference's default direction) or three numbers."""
        flat, b = _flat_queries(points, "points", (3,), self.device)
        if check_direction is None:
            direction = torch.tensor(RayMeshIntersector._DEFAULT_DIRECTION, dtype=torch.float32, device=self.device)
        else:
            direction = torch.as_tensor(check_direction).to(device=self.device, dtype=torch.float32)
            if direction.numel() != 3:
                raise ValueError(f"check_direction must hold three numbers, got shape {tuple(direction.shape)}")
            direction = direction.reshape(3)
        return flat, direction, b

    def contains_points(self, points, check_direction=None) -> torch.Tensor:
        """bool[*b]: is each of points [*b, 3] inside some instance -- one launch (tr_scene_points_any).  A point is inside
        instance k when the rays (p, d) and (p, -d), taken into the instance's frame, each cross an odd number of the
        member's triangles: RayMeshIntersector.contains_points per placed copy, without baking the copies (containment is
        invariant under an invertible affine map).  d is check_direction, or the reference's default direction.  There is
        no box test, no `broken` flag and no retry direction: an OPEN member contains nothing on the side where one of the
        two rays escapes.  A point or a direction with a NaN or an infinity is inside nothing."""
        flat, direction, b = self._points(points, check_direction)
        return hops.scene_points_any_native(self._handle, self.device.index, flat, direction).reshape(b)

    def contains_count(self, points, check_direction=None) -> torch.Tensor:
        """int32[*b]: how many instances each point is inside (tr_scene_points_count); see contains_points.  Two instances
        with the same placement count twice."""
        flat, direction, b = self._points(points, check_direction)
        return hops.scene_points_count_native(self._handle, self.device.index, flat, direction).reshape(b)

    def containing_instances(self, points, check_direction=None):
        """(offsets int64[n + 1], instance int32[h]) for the points flattened in order: the instances that hold point i are
        instance[offsets[i]:offsets[i + 1]], ascending, uncapped; see contains_points.  One count launch, one scan, one host
        read of the total to size the output, one fill."""
        flat, direction, _ = self._points(points, check_direction)
        return hops.scene_points_list_native(self._handle, self.device.index, flat, direction)

    # -- the nearest placed triangle (libtriro_scene_nearest.so, include/triro_scene_nearest.h) ------------------------------
    def closest_point(self, points, max_distance=None):
        """(closest[*b,3] float32, distance[*b] float32, instance[*b] int32, triangle_id[*b] int32) of points [*b, 3]: the
        nearest placed triangle over all instances, one launch (tr_scene_closest_point).  The members' hierarchies are walked
        as they are; boxes and triangles are placed into world space by the scene's own float32 chain and measured there in
        float64, so the answer is RayMeshIntersector.closest_point on the mesh that bakes every placed copy, bit for bit,
        without baking.  Among triangles at exactly the same distance the smaller (instance, face index) wins;
        triangle_id is the face index in the member mesh, closest is in world space.  A placed triangle with a non-finite
        coordinate is never returned.  A point with a non-finite component, a scene without a usable instance:
        (NaN, +Inf, -1, -1).

        max_distance (a number or a tensor that broadcasts to the batch shape; None: unbounded): the nearest placed triangle
        within that distance or none.  A triangle at exactly max_distance is within; NaN or negative: (NaN, +Inf, -1, -1)."""
        flat, b = _flat_queries(points, "points", (3,), self.device)
        r = _query_bound(max_distance, "max_distance", b, self.device, number_ok=True)
        closest, distance, inst, tri = hops.scene_closest_point_native(self._handle, self.device.index, flat, r)
        return closest.reshape(*b, 3), distance.reshape(b), inst.reshape(b), tri.reshape(b)

    def signed_distance(self, points, check_direction=None) -> torch.Tensor:
        """float32[*b]: closest_point's distance with the sign of contains_points -- POSITIVE inside any placed copy, negative
        elsewhere (trimesh's convention, as RayMeshIntersector.signed_distance).  `check_direction` is contains_points'."""
        flat, direction, b = self._points(points, check_direction)
        _, distance, _, _ = hops.scene_closest_point_native(self._handle, self.device.index, flat, None, want_closest=False)
        inside = hops.scene_points_any_native(self._handle, self.device.index, flat, direction)
        return torch.where(inside, distance, -distance).reshape(b)

    # -- triangle queries: a mesh against the placed copies (libtriro_scene_tris.so, include/triro_scene_tris.h) -------------
    def _query_triangles(self, triangles):
        return _flat_queries(triangles, "triangles", (3, 3), self.device)

    def triangles_any(self, triangles) -> torch.Tensor:
        """bool[*b]: does any face of any placed copy meet each of the world triangles [*b, 3, 3] -- one launch
        (tr_scene_tris_any), RayMeshIntersector.triangles_any on the mesh that bakes every placed copy, without baking.  The
        members' hierarchies are walked as they are; boxes and faces are placed into world space by the scene's own float32
        chain and tested there by triangles_any's predicate (csrc/tr_tris.h: both triangles have area and the closed triangles
        share a point, touching included).  A query with a NaN or an infinity, or one without area, meets nothing; a placed
        face with a non-finite coordinate or without area is never met."""
        flat, b = self._query_triangles(triangles)
        return hops.scene_tris_native(self._handle, self.device.index, flat, "any").reshape(b)

    def triangles_count(self, triangles) -> torch.Tensor:
        """int32[*b]: how many (instance, face) pairs meet each triangle (tr_scene_tris_count); see triangles_any.  Two
        instances with the same placement count twice."""
        flat, b = self._query_triangles(triangles)
        return hops.scene_tris_native(self._handle, self.device.index, flat, "count").reshape(b)

    def faces_meeting_triangles(self, triangles):
        """(offsets int64[n + 1], instance int32[h], tri_idx int32[h]) for the triangles flattened in order -- the pairs that
        meet triangle i are rows offsets[i]:offsets[i + 1], ascending by (instance, face index in the member mesh), uncapped.
        One count launch, one scan, one host read of the total to size the outputs, one fill (two launches)."""
        flat, _ = self._query_triangles(triangles)
        return hops.scene_faces_meeting_triangles_native(self._handle, self.device.index, flat)

    def mesh_collides(self, vertices, faces, chunk=1 << 20) -> bool:
        """does any face of the other mesh (vertices [v, 3], faces [m, 3], world space) meet any face of any placed copy
        (triangles_any's predicate)?  Host code on triangles_any, `chunk` faces per launch; stops at the first chunk that says
        yes."""
        tri, chunk = _other_triangles(vertices, faces, chunk, self.device)
        for start in range(0, tri.shape[0], chunk):
            if bool(hops.scene_tris_native(self._handle, self.device.index, tri[start:start + chunk], "any").any()):
                return True
        return False

    def mesh_contacts(self, vertices, faces, chunk=1 << 20) -> torch.Tensor:
        """int64[m, 3]: every triple (face of the other mesh, instance, face of the member) that meets, in lexicographic
        order -- the contact pairs of a mesh and a scene.  Host code on faces_meeting_triangles, `chunk` faces of the other
        mesh per count / scan / fill; the result does not depend on `chunk`."""
        tri, chunk = _other_triangles(vertices, faces, chunk, self.device)
        found = []
        for start in range(0, tri.shape[0], chunk):
            offsets, inst, own = hops.scene_faces_meeting_triangles_native(self._handle, self.device.index, tri[start:start + chunk])
            rows = torch.arange(own.shape[0], dtype=torch.int64, device=self.device)
            other = torch.searchsorted(offsets[1:].contiguous(), rows, right=True) + start      # the query each row belongs to
            found.append(torch.stack((other, inst.long(), own.long()), dim=1))
        return torch.cat(found) if found else torch.zeros((0, 3), dtype=torch.int64, device=self.device)

    def colliding_instances(self, vertices, faces, chunk=1 << 20) -> torch.Tensor:
        """int64[c]: the instances the other mesh touches, ascending -- the distinct instances of mesh_contacts' rows."""
        return torch.unique(self.mesh_contacts(vertices, faces, chunk)[:, 1])
