"""Shared by tests/test_nearest_cpu.py and tests/test_gpu_nearest.py (not a test module): the meshes and points of the
closest_point checks, an independent numpy float64 point-triangle distance, and the tolerance checks against it.

The numpy side shares no code and no formulation with csrc/tr_nearest.h: the in-plane candidate comes from the 2x2 Gram
system of (b - a, c - a) and its barycentric coordinates (the core: the normal and three edge functions), everything is
evaluated for all (point, triangle) pairs at once, nothing is clamped into the triangle's coordinate range.  A triangle with
a NaN or an infinite coordinate is inactive (csrc/tr_nearest.h): its distance from every point is +Inf here."""
import os

import numpy as np

import workloads as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lattice(lo, hi, k):
    """k^3 points that include both bounds on every axis: face, edge and vertex positions of the box, and its centre"""
    ax = [np.linspace(lo[a], hi[a], k, dtype=np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def hash_points(n, seed, lo, hi):
    return np.ascontiguousarray(W.hash_rays(n, seed, np.asarray(lo, np.float32), np.asarray(hi, np.float32))[0], np.float32)


def cube():
    g = np.load(os.path.join(GOLD, "cube_axis_rays.npz"))
    v, f = g["vertices"], g["faces"]
    return v, f, lattice(v.min(0), v.max(0), 9)


def icosphere():
    g = np.load(os.path.join(GOLD, "c1_icosphere80_ortho64.npz"))
    v, f = g["vertices"], g["faces"]
    return v, f, hash_points(1500, 11, v.min(0) * 1.5, v.max(0) * 1.5)


def soup_with_degenerates():
    """the golden soup plus six zero-area triangles: three with collinear vertices (the middle vertex first, last, and a
    doubled end), three with coincident vertices -- all on dyadic coordinates, so they are EXACTLY degenerate"""
    g = np.load(os.path.join(GOLD, "soup400_hash4096.npz"))
    v, f = g["vertices"], g["faces"]
    extra = np.array([
        [[0.25, 0.25, 0.25], [-0.5, -0.5, -0.5], [0.75, 0.75, 0.75]],      # collinear, a between b and c
        [[-0.75, 0.5, 0.0], [0.25, 0.5, 0.0], [-0.25, 0.5, 0.0]],          # collinear, c between a and b
        [[0.5, -0.25, 0.75], [0.5, -0.25, 0.75], [0.5, 0.5, -0.75]],       # collinear: a doubled vertex
        [[0.125, 0.25, -0.5]] * 3,                                         # a point
        [[-0.625, -0.375, 0.875]] * 3,
        [[0.0, 0.0, 0.0]] * 3,
    ], np.float32)
    v2 = np.concatenate([v, extra.reshape(-1, 3)]).astype(np.float32)
    f2 = np.concatenate([f, np.arange(len(v), len(v) + 18, dtype=np.int32).reshape(-1, 3)]).astype(np.int32)
    return v2, f2, np.ascontiguousarray(g["origins"][:1500], np.float32)


def deep_tree():
    """a hierarchy of more than 32 levels with 3 000 coincident triangles at the origin: exact ties in bulk"""
    v, f = W.deep_tree_mesh(3000)
    p = np.concatenate([hash_points(190, 13, [-0.2] * 3, [1.2] * 3),
                        np.array([[0, 0, 0], [1e-10, 1e-10, 0.5], [3e-10, 2e-10, -0.5], [-1, -1, -1], [1, 1, 1], [0.5e-9, 0, 0],
                                  [2.0 ** -21, 0, 0], [0, 0, 2.0 ** -10], [0, 2.0 ** -3, 0], [5e-10, 5e-10, 0]], np.float32)])
    return v, f, np.ascontiguousarray(p, np.float32)


HIERARCHICAL = {"cube": cube, "icosphere": icosphere, "soup": soup_with_degenerates, "deep": deep_tree}
TOLERANCE_CASES = ("cube", "icosphere", "soup")


# ---- the independent evaluation ------------------------------------------------------------------------------------
def _segment(p, a, e):
    """distance of points p to the segments a + t e, t in [0, 1] (broadcast over the leading axes)"""
    ee = (e * e).sum(-1)
    w = p - a
    t = np.where(ee > 0, (w * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0).clip(0.0, 1.0)
    return np.linalg.norm(w - t[..., None] * e, axis=-1)


def _distance(p, a, b, c):
    """float64 distance of points p to triangles (a, b, c), broadcast over the leading axes"""
    e1, e2, w = b - a, c - a, p - a
    g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    r1, r2 = (w * e1).sum(-1), (w * e2).sum(-1)
    det = g11 * g22 - g12 * g12
    ok = det > 1e-10 * g11 * g22                      # an angle above 1e-5 rad: the triangle has a plane
    sd = np.where(ok, det, 1.0)
    s, t = (g22 * r1 - g12 * r2) / sd, (g11 * r2 - g12 * r1) / sd
    inside = ok & (s >= 0) & (t >= 0) & (s + t <= 1)
    face = np.linalg.norm(w - s[..., None] * e1 - t[..., None] * e2, axis=-1)
    d = np.minimum(np.minimum(_segment(p, a, e1), _segment(p, b, c - b)), _segment(p, c, a - c))
    return np.where(inside, np.minimum(face, d), d)


def active(v, f):
    """[F] bool: the triangles whose nine coordinates are finite"""
    return np.isfinite(np.asarray(v, np.float64)[np.asarray(f)]).all(axis=(1, 2))


def numpy_distances(v, f, p):
    """[n, F] float64 distances from every point to every triangle, +Inf to an inactive one"""
    v = np.asarray(v, np.float64)
    ok = active(v, f)
    v = np.where(np.isfinite(v), v, 0.0)                  # (placeholders: the columns of inactive triangles are overwritten)
    a, b, c = (v[f[:, k]][None] for k in range(3))
    return np.where(ok[None, :], _distance(np.asarray(p, np.float64)[:, None, :], a, b, c), np.inf)


def numpy_distances_paired(v, f, tri, p):
    """[n] float64 distances from point k to triangle tri[k]"""
    v = np.asarray(v, np.float64)
    a, b, c = (v[f[tri, k]] for k in range(3))
    return _distance(np.asarray(p, np.float64), a, b, c)


def u32(x):
    return np.spacing(np.asarray(x, np.float32)).astype(np.float64)


def check_against_numpy(v, f, p, closest, distance, tri, what):
    """the four tolerance checks of the closest_point contract on finite points p; prints each figure before it asserts"""
    v, f, p = np.asarray(v, np.float32), np.asarray(f, np.int32), np.asarray(p, np.float32)
    assert np.isfinite(p).all() and len(f) > 0
    assert active(v, f)[tri].all(), f"{what}: an inactive triangle is returned"
    S = float(max(np.abs(v[f[active(v, f)].reshape(-1)]).max(), np.abs(p).max()))
    eps = 2.0 ** -40 * S
    D = numpy_distances(v, f, p)
    d_min = D.min(1)
    rows = np.arange(len(p))
    assert ((tri >= 0) & (tri < len(f))).all(), what
    dist64 = distance.astype(np.float64)
    e_dist = np.abs(dist64 - d_min) - (u32(d_min) + eps)
    to_tri = numpy_distances_paired(v, f, tri, closest)
    e_closest = to_tri - 2 * u32(S)
    e_cons = np.abs(np.linalg.norm(p.astype(np.float64) - closest.astype(np.float64), axis=1) - dist64) - (2 * u32(S) + u32(distance))
    e_win = D[rows, tri] - (d_min + eps)
    print(f"{what}: S = {S:g}, worst excess over the bound (<= 0 passes): distance {e_dist.max():.3g}, closest {e_closest.max():.3g}, "
          f"consistency {e_cons.max():.3g}, winner {e_win.max():.3g}; largest |distance - numpy| {np.abs(dist64 - d_min).max():.3g}")
    assert (e_dist <= 0).all(), f"{what}: distance, {int((e_dist > 0).sum())} points, worst excess {e_dist.max()}"
    assert (e_closest <= 0).all(), f"{what}: closest point off its triangle, worst excess {e_closest.max()}"
    assert (e_cons <= 0).all(), f"{what}: |p - closest| against distance, worst excess {e_cons.max()}"
    assert (e_win <= 0).all(), f"{what}: the returned triangle is not a minimiser, worst excess {e_win.max()}"


def bits(x):
    """float32 arrays compared as bits (NaN == NaN, -0 != +0)"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    """(closest, distance, tri) against (closest, distance, tri), bit for bit"""
    gc, gd, gt = got
    wc, wd, wt = want
    assert np.array_equal(gt, wt), f"{what}: tri differs at {np.flatnonzero(gt != wt)[:8]}: {gt[gt != wt][:8]} != {wt[gt != wt][:8]}"
    if gc is not None:
        assert np.array_equal(bits(gc), bits(wc)), f"{what}: closest differs at {np.flatnonzero((bits(gc) != bits(wc)).any(1))[:8]}"
    if gd is not None:
        assert np.array_equal(bits(gd), bits(wd)), f"{what}: distance differs at {np.flatnonzero(bits(gd) != bits(wd))[:8]}"
