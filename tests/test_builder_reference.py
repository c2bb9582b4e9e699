"""The numpy references of tests/bvh_checks.py against the host construction (tests/host_sim), on a machine without a GPU.

Three things are shown here, so that tests/test_gpu_builder_matrix.py can hold the GPU builder to the same references:
  * the references and the host builder agree on every input the GPU matrix names (a GPU disagreement is the GPU's);
  * check_structure has bite: a tree corrupted in one of five small ways fails it, each for its own reason;
  * node_layout = 0 (Karras numbering) and 1 (treelets) are the same tree under one permutation of the node ids."""
import numpy as np
import pytest

import bvh_checks as K
import sim
import workloads as W
from sim import SimBVH
from test_host_sim import compare_all

LADDER = (2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 30000, 262145)


def copies_of_one_triangle(n):
    """n copies of one triangle, each with vertices of its own (a refit can move them apart): every key is equal"""
    tri = np.array([[0.25, 0.5, 0.125], [0.75, 0.5, 0.25], [0.5, 1.0, 0.375]], np.float32)
    return np.tile(tri, (n, 1)), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def named_mesh(name):
    if name == "ties":
        return copies_of_one_triangle(10000)
    if name == "flat":
        v, f = W.icosphere(3)
        v = v.copy()
        v[:, 2] = np.float32(0.25)
        return v, f
    if name == "line":
        v, f = W.icosphere(3)
        v = v.copy()
        v[:, 1] = np.float32(-0.5)
        v[:, 2] = np.float32(0.25)
        return v, f
    if name == "huge":
        v, f = W.icosphere(3)
        return (v * np.float32(3e12)).astype(np.float32), f
    if name == "tiny":
        v, f = W.icosphere(3)
        return (v * np.float32(1e-12) + np.float32(1e-9)).astype(np.float32), f
    if name == "far":
        v, f = W.icosphere(3)
        return (v * np.float32(0.01) + np.float32([1000.0, -2000.0, 512.25])).astype(np.float32), f
    if name == "soup_x3":
        v, f = W.random_soup(5000, seed=11)
        return v, np.concatenate([f, f, f])
    if name == "sphere_x4":
        v, f = W.icosphere(4)
        return v, np.concatenate([f, f, f, f])
    if name == "ties1025":
        return copies_of_one_triangle(1025)
    if name.startswith("deep"):
        return W.deep_tree_mesh(int(name[4:]))
    raise KeyError(name)


def sim_structure(v, f):
    B = SimBVH(v, f)
    info = dict(depth=B.depth)
    mn, mx = K.bounds_of(K.padded_boxes(v, f))
    info["aabb_min"], info["aabb_max"] = mn.tolist(), mx.tolist()      # (the host builder keeps no bounds: its frame is checked)
    K.check_structure(v, f, B.nodes, B.links, B.tris, B.qnodes, B.frame, info, ref_frame=B.frame)
    assert np.array_equal(B.frame[:3], mn)                               # the frame's base IS the lower bound
    return B


@pytest.mark.parametrize("n", LADDER)
def test_references_agree_with_the_host_builder_over_the_size_ladder(n):
    v, f = W.random_soup(n, seed=n)
    B = sim_structure(v, f)
    assert B.key_mode == 0
    keys = K.morton_keys(v, f)
    assert np.all(np.diff(keys[B.tris[:, K.FACE].view(np.int32)].astype(np.int64)) >= 0)


def test_single_triangle_has_a_record_and_no_nodes():
    v, f = W.random_soup(1, seed=1)
    B = SimBVH(v, f)
    assert len(B.nodes) == 0 and np.array_equal(B.tris, K.tri_records(v, f, [0])) and B.tris[0, K.PAD1] == 0


@pytest.mark.parametrize("name,height,key_mode", [
    ("ties", 14, 0), ("ties1025", 11, 0), ("flat", None, 0), ("line", None, 0), ("huge", None, 0), ("tiny", None, 0),
    ("far", None, 0), ("soup_x3", None, 0), ("sphere_x4", 19, 0),
    ("deep1", 62, 0), ("deep2", 63, 0), ("deep3", 63, 0), ("deep4", 64, 0), ("deep5", 64, 0), ("deep8", 36, 1), ("deep4000", None, 1)])
def test_references_agree_with_the_host_builder_on_named_meshes(name, height, key_mode):
    v, f = named_mesh(name)
    B = sim_structure(v, f)
    assert B.key_mode == key_mode and B.depth <= 64
    if height is not None:
        assert B.depth == height
    if name.startswith("ties"):
        assert np.array_equal(B.tris[:, K.FACE].view(np.int32), np.arange(len(f)))     # all keys equal: the input order
        assert len(np.unique(K.morton_keys(v, f))) == 1
    if name == "deep8":
        assert SimBVH(v, f, force_mode=0).depth == 65                                # one level too many for plain keys


# ---- the checker has bite ---------------------------------------------------------------------------------------------
def _valid_tree():
    v, f = W.random_soup(3000, seed=21)
    f = np.concatenate([f, f[:700]])                  # 700 triangles twice: pairs of equal keys, face ids 3000 apart
    B = SimBVH(v, f)
    mn, mx = K.bounds_of(K.padded_boxes(v, f))
    info = dict(depth=B.depth, aabb_min=mn.tolist(), aabb_max=mx.tolist())
    return v, f, B, info


def _check(v, f, B, info, **arrays):
    a = dict(nodes=B.nodes, links=B.links, tris=B.tris, qnodes=B.qnodes, frame=B.frame)
    a.update(arrays)
    K.check_structure(v, f, a["nodes"], a["links"], a["tris"], a["qnodes"], a["frame"], info, ref_frame=B.frame)


def _ulp_outward(word, lower):
    x = np.array([word], np.uint32).view(np.float32)
    return np.nextafter(x, np.float32(-np.inf if lower else np.inf)).view(np.uint32)[0]


@pytest.mark.parametrize("case", ["none", "unstable_sort", "leaf_box", "internal_box", "parent_links", "grid_plane",
                                  "height", "bounds"])
def test_check_structure_rejects_each_corruption_for_its_own_reason(case):
    v, f, B, info = _valid_tree()
    nodes, links, tris, qnodes = B.nodes.copy(), B.links.copy(), B.tris.copy(), B.qnodes.copy()
    c = nodes[:, 12:14].view(np.int32)
    par = nodes[:, 14].view(np.int32)
    if case == "none":
        _check(v, f, B, info)
        return
    if case == "unstable_sort":
        # (a) two records with equal keys change places, as an unstable scatter would leave them: every box stays right
        keys = K.morton_keys(v, f)[tris[:, K.FACE].view(np.int32)]
        s = int(np.flatnonzero(keys[1:] == keys[:-1])[0])
        tris[[s, s + 1]] = tris[[s + 1, s]]
        want, part = "order", "stable sort"
    elif case == "leaf_box":
        # (b) one bound of one leaf box, one float spacing outward: still contains its triangle, answers every ray
        m = int(np.flatnonzero(c[:, 1] < 0)[5])
        nodes[m, 6 + 4] = _ulp_outward(nodes[m, 6 + 4], lower=False)            # child 1, hi.x
        want, part = "leaf_boxes", "padded triangle box"
    elif case == "internal_box":
        # (c) the same on a box of an internal child
        m = int(np.flatnonzero(c[:, 0] >= 0)[7])
        nodes[m, 0] = _ulp_outward(nodes[m, 0], lower=True)                     # child 0, lo.x
        want, part = "tree: box nesting", "boxes[m, 6 * k"
    elif case == "parent_links":
        # (d) two nodes with different parents exchange their parent links (in both copies of the links)
        a = 5
        b = int(np.flatnonzero((par != par[a]) & (par >= 0))[9])
        assert par[a] != par[b]
        nodes[[a, b], 14] = nodes[[b, a], 14]
        links[[a, b], 0] = links[[b, a], 0]
        want, part = "tree: links", "par[ch[m]]"
    elif case == "grid_plane":
        # (e) one upper grid plane one cell down: the grid box no longer contains the exact box
        hx = qnodes[:, 2] & 0xffff
        m = int(np.flatnonzero(hx > 0)[3])
        qnodes[m, 2] -= 1
        want, part = "tree: grid nodes", ">= ex_hi"
    elif case == "height":
        info = dict(info, depth=info["depth"] + 1)
        want, part = "height", "reported"
    else:
        info = dict(info, aabb_max=[np.nextafter(np.float32(x), np.float32(np.inf)) for x in info["aabb_max"]])
        want, part = "bounds", "union of the padded boxes"
    with pytest.raises(K.StructureError) as e:
        _check(v, f, B, info, nodes=nodes, links=links, tris=tris, qnodes=qnodes)
    assert e.value.check == want and part in str(e.value), str(e.value)


# (a leaf box holds a NaN only where all three vertices are NaN, or infinite with one sign, on one axis: the all-NaN triangle)
HOSTILE_BITE = [(name, seed, case) for name, seed in (("nonfinite", 0), ("faraway_nonfinite", 1), ("deep_nan", 0), ("holed_sphere", None),
                                                      ("all_nan_triangle", None))
                for case in ("none", "leaf_box", "internal_box", "nan_for_a_number") + (("nan_payload", "number_for_a_nan") if name == "all_nan_triangle" else ())]


@pytest.mark.parametrize("name,seed,case", HOSTILE_BITE)
def test_check_structure_keeps_its_bite_on_a_hostile_mesh(name, seed, case):
    """a tree over NaN and infinite vertices (tests/hostile_meshes.py) passes with any NaN payload, and is still rejected
    when one finite bound is off by one float spacing, when a NaN stands where a number belongs and the other way round"""
    import hostile_meshes as M
    m = M.case(name, seed)
    B = SimBVH(m.v, m.f)
    mn, mx = K.bounds_of(K.padded_boxes(m.v, m.f))
    info = dict(depth=B.depth, aabb_min=mn.tolist(), aabb_max=mx.tolist())
    nodes = B.nodes.copy()
    c = nodes[:, 12:14].view(np.int32)
    boxes = nodes[:, :12].view(np.float32)
    nan = np.isnan(boxes)
    assert np.isfinite(boxes).any() and (nan.any() or name != "all_nan_triangle") and not np.isfinite(m.v[m.f]).all()
    leaf = np.repeat(c < 0, 6, axis=1)
    want = None
    if case == "nan_payload":
        nodes[:, :12][nan] = np.uint32(0xffc12345)                                      # another sign, another payload
    elif case in ("leaf_box", "internal_box"):
        rows, cols = np.nonzero(np.isfinite(boxes) & (boxes != 0) & (leaf if case == "leaf_box" else ~leaf))
        r, k = int(rows[len(rows) // 2]), int(cols[len(rows) // 2])
        nodes[r, k] = _ulp_outward(nodes[r, k], lower=(k % 6) < 3)
        want = "leaf_boxes" if case == "leaf_box" else "tree: box nesting"
    elif case == "nan_for_a_number":
        rows, cols = np.nonzero(np.isfinite(boxes) & leaf)
        nodes[rows[0], cols[0]] = np.uint32(0x7fc00000)
        want = "leaf_boxes"
    elif case == "number_for_a_nan":
        rows, cols = np.nonzero(nan & leaf)
        nodes[rows[0], cols[0]] = np.float32(0.5).view(np.uint32)
        want = "leaf_boxes"
    if want is None:
        _check(m.v, m.f, B, info, nodes=nodes)
        return
    with pytest.raises(K.StructureError) as e:
        _check(m.v, m.f, B, info, nodes=nodes)
    assert e.value.check == want, str(e.value)


# ---- node_layout = 0 ----------------------------------------------------------------------------------------------------
def node_permutation(A, B):
    """p with p[0] = 0 such that node i of tree A is node p[i] of tree B (walked from the root, leaf ids must be equal)"""
    ca, cb = A.nodes[:, 12:14].view(np.int32), B.nodes[:, 12:14].view(np.int32)
    p = np.full(len(ca), -1, np.int64)
    p[0] = 0
    frontier = np.zeros(1, np.int64)
    while len(frontier):
        a, b = ca[frontier], cb[p[frontier]]
        leaf = a < 0
        assert np.array_equal(leaf, b < 0) and np.array_equal(a[leaf], b[leaf])
        p[a[~leaf]] = b[~leaf]
        frontier = a[~leaf].astype(np.int64)
    assert np.array_equal(np.sort(p), np.arange(len(p)))
    return p


def same_tree_under_a_permutation(A, B):
    assert np.array_equal(A.tris, B.tris) and np.array_equal(A.frame, B.frame) and A.depth == B.depth
    p = node_permutation(A, B)

    def mapped(ids):                                     # child / parent / sibling ids of A in B's numbering
        ids = ids.astype(np.int64)
        return np.where(ids >= 0, p[np.maximum(ids, 0)], ids)
    assert np.array_equal(A.nodes[:, :12], B.nodes[p, :12]) and np.array_equal(A.qnodes[:, :6], B.qnodes[p, :6])
    assert np.array_equal(mapped(A.nodes[:, 12:14].view(np.int32)), B.nodes[p, 12:14].view(np.int32))
    assert np.array_equal(mapped(A.qnodes[:, 6:8].view(np.int32)), B.qnodes[p, 6:8].view(np.int32))
    par_a = A.links[:, 0]
    assert np.array_equal(mapped(par_a), B.links[p, 0])
    assert np.array_equal(mapped(A.links[1:, 1]), B.links[p[1:], 1]) and A.links[0, 1] == B.links[0, 1] == 0
    # the same multiset of (child-box pair, leaf ids) per node, internal ids blanked
    def rows(T):
        c = T.nodes[:, 12:14].view(np.int32)
        r = np.concatenate([T.nodes[:, :12], np.where(c < 0, c, 0).view(np.uint32)], axis=1)
        return r[np.lexsort(r.T[::-1])]
    assert np.array_equal(rows(A), rows(B))
    return p


def leaf_ranges(T):
    """(first, last) leaf slot below every node"""
    c = T.nodes[:, 12:14].view(np.int32).astype(np.int64)
    n = len(c)
    lo, hi = np.zeros(n, np.int64), np.zeros(n, np.int64)
    order, frontier = [], np.zeros(1, np.int64)
    while len(frontier):
        order.append(frontier)
        ch = c[frontier].ravel()
        frontier = ch[ch >= 0]
    for level in reversed(order):                        # children before parents
        l, r = c[level, 0], c[level, 1]
        lo[level] = np.where(l < 0, ~l, lo[np.maximum(l, 0)])
        hi[level] = np.where(r < 0, ~r, hi[np.maximum(r, 0)])
    return lo, hi


@pytest.mark.parametrize("name", ["soup2", "soup65", "soup4097", "soup30000", "deep5", "sphere_x4"])
def test_node_layouts_0_and_1_are_the_same_tree(name):
    v, f = W.random_soup(int(name[4:]), seed=int(name[4:])) if name.startswith("soup") else named_mesh(name)
    B1 = SimBVH(v, f)
    sim.use_node_layout(0)
    try:
        B0 = SimBVH(v, f)
    finally:
        sim.use_node_layout(1)
    info = dict(depth=B0.depth)
    mn, mx = K.bounds_of(K.padded_boxes(v, f))
    info["aabb_min"], info["aabb_max"] = mn.tolist(), mx.tolist()
    K.check_structure(v, f, B0.nodes, B0.links, B0.tris, B0.qnodes, B0.frame, info, ref_frame=B1.frame)
    p = same_tree_under_a_permutation(B0, B1)
    if len(f) > 8:
        assert not np.array_equal(p, np.arange(len(p)))              # the two layouts really differ
    # Karras numbering: an internal node over the leaves [first, last] split after leaf g has the children g and g + 1,
    # so a left child's id is the LAST leaf of its range, a right child's the FIRST
    lo, hi = leaf_ranges(B0)
    c = B0.nodes[:, 12:14].view(np.int32)
    l, r = c[c[:, 0] >= 0, 0], c[c[:, 1] >= 0, 1]
    assert np.array_equal(l, hi[l]) and np.array_equal(r, lo[r])
    assert lo[0] == 0 and hi[0] == len(f) - 1
    assert np.array_equal(SimBVH(v, f).nodes, B1.nodes)               # the switch is back: default builds are treelets


def test_host_traversal_of_layout_0_matches_the_oracle():
    sim.use_node_layout(0)
    try:
        v, f = W.icosphere(4)
        compare_all(v, f, *W.readme_perspective(128))
        v, f = W.random_soup(2500, seed=8)
        o, d = W.hash_rays(12000, 4, v.min(0) * 1.5, v.max(0) * 1.5)
        compare_all(v, f, o, d)
    finally:
        sim.use_node_layout(1)
