"""Shared by tests/test_range_cpu.py and tests/test_gpu_range.py (not a test module): the meshes, rays and bounds of the
range-query checks (csrc/tr_range.h), the sheet scene whose hit distances are exact, and the bit-for-bit comparison."""
import os

import numpy as np

import nearest_cases as NC
import workloads as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_RAYS = 20000
KEYS_ANY = ("any",)
KEYS_CLOSEST = ("hit", "front", "tri", "loc", "uv", "t")


def extent(v):
    return float((v.max(0) - v.min(0)).max())


def hash_bounds(n, seed, top):
    """tmin <= tmax, both uniform in [0, top): the smaller and the larger of two hash values"""
    u = W.hash_rays(n, seed, np.zeros(3, np.float32), np.ones(3, np.float32))[0]
    a, b = u[:, 0] * np.float32(top), u[:, 1] * np.float32(top)
    return np.minimum(a, b).astype(np.float32), np.maximum(a, b).astype(np.float32)


def rays_in_box(v, n, seed):
    """n hash rays with origins inside the mesh's box and 0 <= tmin <= tmax <= 1.5 x extent"""
    o, d = W.hash_rays(n, seed, v.min(0), v.max(0))
    lo, hi = hash_bounds(n, seed + 1, 1.5 * extent(v))
    return np.ascontiguousarray(o), np.ascontiguousarray(d), lo, hi


def icosphere():
    v, f = W.icosphere(3)
    assert len(f) == 1280
    return (v, f) + rays_in_box(v, N_RAYS, 41)


def shells5():
    g = np.load(os.path.join(GOLD, "shells5_pinhole48.npz"))
    v, f = g["vertices"], g["faces"]
    assert len(f) == 1600
    return (v, f) + rays_in_box(v, N_RAYS, 43)


def deep():
    """the hierarchy of more than 32 levels of nearest_cases: 63 triangles of 1e-9 spread over the unit box and 3 000
    coincident ones at the origin.  Hash rays hit none of them, so the last 1 000 rays are aimed at a point inside the
    pile (distance 1 along d = target - o): 3 000 exact ties per ray, bounds around 1."""
    v, f, _ = NC.deep_tree()
    o, d, lo, hi = rays_in_box(v, N_RAYS, 47)
    k = 1000
    target = np.array([3e-10, 2e-10, 0.0], np.float32)
    d[-k:] = (target[None, :] - o[-k:]).astype(np.float32)
    return v, f, o, np.ascontiguousarray(d), lo, hi


MESHES = {"icosphere": icosphere, "shells5": shells5, "deep": deep}


# ---- the sheet scene: every hit distance is an even integer, exactly ---------------------------------------------------
SHEETS = 8
TRIS_PER_SHEET = 32


def sheets():
    """eight sheets at z = 1 .. 8, each a 4 x 4 grid of unit squares split along the diagonal (i, j) - (i + 1, j + 1)"""
    vs, fs = [], []
    for z in range(1, SHEETS + 1):
        base = len(vs)
        for i in range(5):
            for j in range(5):
                vs.append((i, j, z))
        for i in range(4):
            for j in range(4):
                a, b, c, d = base + 5 * i + j, base + 5 * (i + 1) + j, base + 5 * (i + 1) + j + 1, base + 5 * i + j + 1
                fs += [(a, c, b), (a, d, c)]      # normals point to -z: front faces for the rays from below
    return np.array(vs, np.float32), np.array(fs, np.int32)


def sheet_origins(kind):
    """xy of the rays: 'interior' (i + .25, j + .5): inside a triangle; 'diagonal' (i + .5, j + .5): on the shared diagonal of a
    square; 'vertex' (i, j), i, j = 1 .. 3: on an interior grid vertex, six triangles around it"""
    if kind == "interior":
        xy = [(i + 0.25, j + 0.5) for i in range(4) for j in range(4)]
    elif kind == "diagonal":
        xy = [(i + 0.5, j + 0.5) for i in range(4) for j in range(4)]
    else:
        xy = [(i, j) for i in range(1, 4) for j in range(1, 4)]
    return np.array([(x, y, 0.0) for x, y in xy], np.float32)


def sheet_cases(kind):
    """(origins, directions, tmin, tmax, first, count): every ray of `kind` under every bound case; d = (0, 0, .5), so sheet k
    is hit at t = 2 k exactly.  first = the sheet of the closest accepted hit (0: a miss), count = the number of sheets in
    range = the number of accepted triangles (one owner per edge)."""
    f32 = np.float32
    inf, nan = f32(np.inf), f32(np.nan)
    cases = []      # (tmin, tmax, first, count)
    for k in range(1, SHEETS + 1):
        t = f32(2 * k)
        below, above = np.nextafter(t, f32(0)), np.nextafter(t, inf)
        cases += [
            (f32(0), t, 1, k),                                             # tmax = 2k accepts sheet k ...
            (f32(0), below, 1 if k > 1 else 0, k - 1),                     # ... one ulp less rejects it
            (t, f32(1e7), k, SHEETS - k + 1),                              # tmin = 2k accepts it ...
            (above, f32(1e7), k + 1 if k < SHEETS else 0, SHEETS - k),     # ... one ulp more rejects it
            (t, t, k, 1),                                                  # exactly that sheet
            (t, below, 0, 0), (above, t, 0, 0),                            # lo > hi
            (f32(-5), t, 1, k), (-inf, t, 1, k),                           # a negative tmin is 0
            (t, inf, k, SHEETS - k + 1),                                   # tmax = +Inf is TR_TMAX
            (nan, t, 0, 0), (t, nan, 0, 0), (nan, nan, 0, 0),              # a NaN bound misses
        ]
    cases += [(f32(0), f32(1e7), 1, SHEETS), (f32(0), inf, 1, SHEETS), (inf, inf, 0, 0), (f32(17), f32(1e7), 0, 0), (f32(0), f32(1.5), 0, 0)]
    xy = sheet_origins(kind)
    m, c = len(xy), len(cases)
    o = np.tile(xy, (c, 1))
    d = np.tile(np.array([[0, 0, 0.5]], np.float32), (m * c, 1))
    col = lambda j, ty: np.repeat(np.array([x[j] for x in cases], ty), m)      # noqa: E731
    return o, d, col(0, np.float32), col(1, np.float32), col(2, np.int32), col(3, np.int32)


def check_sheet_results(res, first, count, what):
    """brute-force results of sheet_cases against what the scene says"""
    hit = first > 0
    assert np.array_equal(res["any"], hit) and np.array_equal(res["hit"], hit), what
    assert np.array_equal(res["count"], count), f"{what}: accepted triangles per ray {res['count'][res['count'] != count][:8]}"
    assert np.array_equal(np.where(hit, res["tri"] // TRIS_PER_SHEET + 1, 0), first), what
    assert np.array_equal(res["t"], np.where(hit, 2.0 * first, np.inf).astype(np.float32)), what
    assert (res["tri"][~hit] == -1).all() and (res["loc"][~hit] == 0).all() and (res["uv"][~hit] == 0).all() and not res["front"][~hit].any()
    assert res["front"][hit].all(), what      # counter-clockwise seen from below
    if "accepted" in res:
        acc = res["accepted"]
        sheets_hit = np.where(acc >= 0, acc // TRIS_PER_SHEET, -1)
        for row in sheets_hit:
            got = row[row >= 0]
            assert len(set(got)) == len(got), f"{what}: two accepted triangles on one sheet"


def segment_rays(p0, p1):
    """the arithmetic of segments_*: d = the float32 p1 - p0, the range [0, 1]"""
    p0, p1 = np.asarray(p0, np.float32), np.asarray(p1, np.float32)
    return p0, (p1 - p0).astype(np.float32), np.float32(0), np.float32(1)


def hostile_rays(o, d, lo, hi):
    """(origins, directions, tmin, tmax, bad): 512 ordinary rays with NaN, +-Inf, 3e38 and denormal components, a zero
    direction, NaN / infinite / empty bounds, a whole wave of invalid rays, one of invalid bounds and a whole block of
    infinite origins put in.  bad: the rays that must miss by the contract's rule (a non-finite component, a NaN bound or an
    empty range)."""
    o, d, lo, hi = (np.array(x[:512], np.float32) for x in (o, d, lo, hi))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    k = 0
    for value in (nan, inf, -inf):
        for axis in range(3):
            o[5 + 11 * k, axis] = value
            d[8 + 11 * k, axis] = value
            k += 1
    d[110] = 0                                                          # a zero direction: a valid ray that goes nowhere
    o[111] = [3e38, -3e38, 3e38]; d[112] = [3e38, 3e38, -3e38]; o[113] = [3e38, 0, 0]; d[113] = [-3e38, 0, 0]
    d[114] = [1e-42, 0, 1e-45]; o[115] = [1e-40, -1e-42, 0]
    lo[120], hi[121] = nan, nan
    lo[122], hi[122] = nan, nan
    lo[123] = inf; hi[124] = -inf; lo[125], hi[125] = -inf, inf; lo[126], hi[126] = 3e38, 3e38; hi[127] = 0.0; lo[119] = -0.0
    o[128:192] = nan                                                    # a whole wave of invalid rays ...
    lo[192:256] = nan                                                   # ... and one of invalid bounds
    o, d = np.concatenate([o, np.full((128, 3), inf, np.float32), o[:70]]), np.concatenate([d, d[:128], d[:70]])      # ... and a whole block
    lo, hi = np.concatenate([lo, lo[:128], lo[:70]]), np.concatenate([hi, hi[:128], hi[:70]])
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(o).all(1) | ~np.isfinite(d).all(1) | np.isnan(lo) | np.isnan(hi) | (np.maximum(lo, 0) > np.minimum(hi, np.float32(1e7)))
    assert bad.sum() >= 18 + 64 + 64 + 128 + 5 and not bad[[110, 111, 112, 113, 114, 115, 119, 125]].any()
    return o, d, lo, hi, bad


def check_miss_rule(res, bad, what):
    """every ray of `bad` has the miss values in every output, and no t is NaN"""
    for key, miss in (("any", 0), ("hit", 0), ("front", 0), ("tri", -1), ("loc", 0), ("uv", 0)):
        assert (res[key][bad] == miss).all(), f"{what}: {key}"
    assert np.isposinf(res["t"][bad]).all() and not np.isnan(res["t"]).any(), what


# ---- comparison ----------------------------------------------------------------------------------------------------
def bits(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.float32:
        return x.view(np.uint32)
    return x.astype(np.int64) if x.dtype == bool else x


def assert_same_bits(got, want, what, keys=KEYS_ANY + KEYS_CLOSEST):
    """dicts of arrays, bit for bit (NaN == NaN, -0 != +0); a key missing or None in `got` was not asked for"""
    for k in keys:
        g = got.get(k)
        if g is None:
            continue
        w = want[k]
        g = np.asarray(g).reshape(w.shape)
        same = bits(g) == bits(w)
        if not same.all():
            rows = np.flatnonzero(~same.reshape(len(w), -1).all(1))
            raise AssertionError(f"{what}: {k} differs on {len(rows)} of {len(w)} rays, first {rows[:8]}: {g[rows[:4]]} != {w[rows[:4]]}")
