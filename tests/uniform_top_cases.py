"""The inputs of tests/test_uniform_top_cpu.py (host simulation) and tests/test_gpu_uniform_top.py (the kernels against the
oracle): what the uniform top of wave_traverse_steal can get wrong, each at the smallest shape that reaches it.  A wave is 64
consecutive rays.  CASES: name -> () -> (vertices, faces, origins (n, 3), directions (n, 3))."""
import numpy as np

import workloads as W


def image(w, h, distance=2.5, vfov=40.0):
    o, d = W.pinhole_grid(w, h, vfov_deg=vfov, distance=distance)
    return (np.ascontiguousarray(np.broadcast_to(o, d.shape), np.float32).reshape(-1, 3),
            np.ascontiguousarray(d, np.float32).reshape(-1, 3))


def tiles(w, h, distance=2.5, vfov=40.0):
    """the image 8 x 8 tile after 8 x 8 tile, as the launches of large images walk it: a wave is a tile"""
    o, d = image(w, h, distance, vfov)
    k = np.arange(h * w).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    return o[k], d[k]


def small_mesh(n):
    """1 triangle: no internal node; 2: a root with two leaf children; 3: a root with a leaf and an internal child"""
    v, f = W.two_triangles()
    if n == 1:
        return v[:3].copy(), f[:1].copy()
    if n == 3:
        v = np.concatenate([v, v[:3] + np.float32([10.0, 0.0, 0.0])]).astype(np.float32)      # far off to the side: the root's leaf child
        f = np.concatenate([f, [[6, 7, 8]]]).astype(np.int32)
    return v, f


def small(n):
    """two waves at the pair of triangles and two beside it: a leaf child at the root ends the loop on its first trip"""
    v, f = small_mesh(n)
    o, d = image(16, 16, distance=3.0, vfov=30.0)
    rows = np.arange(8)[:, None] * 16 + np.arange(8)[None, :]
    k = np.concatenate([rows.reshape(-1), (rows + 8 * 16 + 8).reshape(-1)])      # two quadrants of the image: one octant per wave
    o, d = o[k], d[k]
    return v, f, np.concatenate([o, o + np.float32([10.0, 0.0, 0.0])]), np.concatenate([d, d])


def sphere(rays):
    v, f = W.icosphere(3)
    o, d = rays()
    return v, f, o, d


BASE = 64 * 40 + 41      # a pixel of the 64 x 64 image that hits the sphere off its centre: direction (+, -, -)


def identical():
    """64 copies of one ray: one node, one octant, down to the trip that accepts the first leaf"""
    o, d = image(64, 64)
    return np.repeat(o[BASE][None], 64, 0), np.repeat(d[BASE][None], 64, 0)


# lane 37's origin, in steps of (1/8, 1/8, -1/4) from the others': a parallel ray (the same octant) that goes the wave's way
# for k - 1 trips and another way -- another child, or none -- on trip k (found with the host simulation, which
# tests/test_uniform_top_cpu.py holds them to: the loop of that wave runs exactly k trips)
LEAVES_AT = {1: (-12, -12, 0), 2: (0, 2, 0), 3: (2, -8, 11), 4: (5, -6, 0), 5: (0, -6, 0)}


def one_lane_leaves_at(k):
    def rays():
        o, d = identical()
        o = o.copy()
        o[37] += np.float32([0.125, 0.125, -0.25]) * np.float32(LEAVES_AT[k])
        return o, d
    return rays


def one_tile():
    """8 x 8 pixels beside the image's centre: one octant"""
    o, d = image(64, 64)
    k = (np.arange(32, 40)[:, None] * 64 + np.arange(36, 44)[None, :]).reshape(-1)
    return o[k], d[k]


def mixed_octants():
    """8 x 8 pixels around the image's centre: directions of both signs in x and in y -- the wave must skip the loop"""
    o, d = image(64, 64)
    k = (np.arange(28, 36)[:, None] * 64 + np.arange(28, 36)[None, :]).reshape(-1)
    return o[k], d[k]


def lane_0_invalid():
    """the first lanes of each wave have no valid ray (a NaN in the direction or in the origin): the octant is that of the
    first lane that has one.  (A zero direction is a valid ray that hits nothing, of the octant + + +.)"""
    o, d = tiles(32, 16)
    o, d = o.copy(), d.copy()
    d[0::64] = np.nan
    d[1::64, 1] = np.nan
    o[64:67, 2] = np.inf
    return o, d


def inside():
    """origins inside the sphere: unrelated rays, nearly every wave of mixed octants; and one point inside with an image's
    directions"""
    o, d = W.hash_rays(2048, 11, np.float32([-0.5] * 3), np.float32([0.5] * 3))
    o2, d2 = tiles(32, 32)
    return np.concatenate([o, np.zeros_like(o2) + np.float32([0.1, -0.2, 0.3])]), np.concatenate([d, d2])


def away():
    o, d = tiles(16, 16)
    return o + np.float32([0, 0, 1]), -d      # looking away: every ray misses the root's box


def stretch(n):
    def rays():
        o, d = image(64, 64)
        s = 64 * 30 + 20                      # a stretch of the image that crosses the silhouette
        return o[s:s + n], d[s:s + n]
    return rays


def hash_rays():
    v, _ = W.icosphere(3)
    return W.hash_rays(4096, 4, v.min(0) * 1.5, v.max(0) * 1.5)


def dense_soup():
    """tests/test_gpu_descent.py's: 2^18 triangles that all overlap, seen through a narrow image -- every ray pushes a
    seventeenth far child before its wave has a leaf"""
    v, f = W.random_soup(1 << 18, seed=8, extent=0.2, size=3.0)
    o, d = image(16, 8, distance=4.0 * float(np.abs(v).max()), vfov=5.0)
    return v, f, o, d


CASES = {
    "one triangle": lambda: small(1),
    "two triangles": lambda: small(2),
    "three triangles": lambda: small(3),
    "sphere from outside": lambda: sphere(lambda: tiles(64, 64)),
    "sphere from inside": lambda: sphere(inside),
    "64 identical rays": lambda: sphere(identical),
    "one 8 x 8 tile": lambda: sphere(one_tile),
    "image of 20 x 12": lambda: sphere(lambda: image(20, 12)),
    "1 ray": lambda: sphere(stretch(1)),
    "63 rays": lambda: sphere(stretch(63)),
    "65 rays": lambda: sphere(stretch(65)),
    "193 rays": lambda: sphere(stretch(193)),
    "lane 0 invalid": lambda: sphere(lane_0_invalid),
    "rays that miss the root box": lambda: sphere(away),
    "mixed octants": lambda: sphere(mixed_octants),
    "one lane leaves at trip 1": lambda: sphere(one_lane_leaves_at(1)),
    "one lane leaves at trip 2": lambda: sphere(one_lane_leaves_at(2)),
    "one lane leaves at trip 3": lambda: sphere(one_lane_leaves_at(3)),
    "one lane leaves at trip 4": lambda: sphere(one_lane_leaves_at(4)),
    "one lane leaves at trip 5": lambda: sphere(one_lane_leaves_at(5)),
    "4096 hash rays": lambda: sphere(hash_rays),
    "dense soup": dense_soup,
}
STEAL_MINS = (4, 64, 5, 1)
