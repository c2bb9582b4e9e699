"""Cross-check "from outside the contract": the oracle (CPU) and the HIP path (GPU) against a
textbook float64 Moller-Trumbore (tests/geom64.py).  The reference holds no golden vectors and
cannot run here (oracle header: parity unpinned), so this is the independent evidence that the
contract arithmetic describes the geometry: on every ray whose nearest hit is robust (not within
1e-4 barycentric of a triangle border, no second hit within 1e-4 of the first) hit / tri_idx must
agree exactly and loc within 1e-5 relative (BASELINE.json north_star tolerance)."""
import numpy as np
import pytest

import workloads as W
from geom64 import closest_f64
from oracle.oracle import OracleIntersector
from poison import poisoned_outputs  # noqa: F401  (autouse: every output is born poisoned, every eager result checked)

CASES = {
    "icosphere3_hash": lambda: (W.icosphere(3), W.hash_rays(6000, 11, [-1.6] * 3, [1.6] * 3)),
    "soup_hash": lambda: (W.random_soup(600, seed=4), W.hash_rays(6000, 12, [-1.2] * 3, [1.2] * 3)),
    "shells_pinhole": lambda: (W.nested_shells(2), tuple(x.reshape(-1, 3) for x in W.pinhole_grid(64, 64))),
    "displaced_ortho": lambda: ((lambda vf: (W.displaced(vf[0], seed=3), vf[1]))(W.icosphere(3)),
                                tuple(x.reshape(-1, 3) for x in W.ortho_grid(72))),
}


def check(got_hit, got_tri, got_loc, ref):
    hit, tri, t, loc, robust = ref
    assert robust.mean() > 0.9, "the robust subset must cover almost all rays"
    assert np.array_equal(got_hit[robust], hit[robust])
    assert np.array_equal(got_tri[robust], tri[robust])
    m = robust & hit
    np.testing.assert_allclose(got_loc[m], loc[m], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_float64_geometry(name):
    (v, f), (o, d) = CASES[name]()
    ref = closest_f64(v, f, o, d)
    eh, ef, et, el, eu = OracleIntersector(v, f, 1).closest_raw(o, d)[:5]
    check(eh, et, el, ref)
    # front flag = sign of (b-a)x(c-a) . d, in float64
    vv = np.asarray(v, np.float64)
    m = ref[4] & ref[0]
    tri = ref[1][m]
    nrm = np.cross(vv[f[tri, 1]] - vv[f[tri, 0]], vv[f[tri, 2]] - vv[f[tri, 0]])
    facing = np.einsum("ij,ij->i", nrm, np.asarray(d, np.float64).reshape(-1, 3)[m]) < 0
    assert np.array_equal(ef[m], facing)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_matches_float64_geometry(name, device):
    import torch
    from triro.ray.ray_optix import RayMeshIntersector
    (v, f), (o, d) = CASES[name]()
    ref = closest_f64(v, f, o, d)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    r = RayMeshIntersector(vertices=T(v), faces=T(f))
    hit, front, tri, loc, uv = [x.cpu().numpy() for x in r.intersects_closest(T(o), T(d))]
    check(hit, tri, loc, ref)
