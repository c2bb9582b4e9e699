"""Plain numpy references of what the BVH builder has to produce (helper module: no tests in it).

Everything here is written from the DEFINITIONS in csrc/tr_math.h (tr_tri_box, tr_pad, tr_tri_scale), csrc/tr_lbvh.h
(tr_morton63, tr_spread21) and csrc/tr_bvh.h (the node, link and triangle records), in float32 numpy arithmetic -- not
by calling tests/host_sim, which compiles those very headers.  The GPU builder (csrc/bvh_build.hip) and the host
simulation are both compared with it, so that an error in a header cannot hide in a comparison of the header with
itself.  numpy rounds every float32 operation once and never contracts a multiply and an add; the expressions of the
headers that a compiler may contract (tr_pad, the centre of tr_morton63) multiply by powers of two, which is exact, so
a contracted and an uncontracted evaluation have to agree bit for bit.

check_structure raises StructureError (an AssertionError) whose `check` names the check that failed:
    "order"        tris[:, face] is not what a stable sort of the Morton keys gives
    "records"      a triangle record is not (vertices, face, esum, 0) of its face
    "leaf_boxes"   a leaf child box is not the padded box of that leaf's triangle
    "tree: ..."    test_host_sim.check_tree failed; the rest names the part (topology / links / box nesting / grid nodes)
                   and the message quotes the assertion
    "height"       the height walked from the root differs from info["depth"] or exceeds 64
    "bounds"       info["aabb_min/max"] is not the union of the padded boxes
    "frame"        the grid frame is not the one derived from those bounds

Meshes with NaN or infinite vertices (tests/hostile_meshes.py) are judged by the same checks: minima and maxima are those
of fminf / fmaxf (np.fmin / np.fmax: a NaN operand is ignored, two NaN give NaN), reductions start from +Inf / -Inf as the
builder's do, and floats are compared as bits with EVERY NaN EQUAL TO EVERY NaN (canon_bits): which payload and sign an
Inf - Inf or a propagated NaN carries differs between an x86 and a gfx950 build and is nobody's contract.  -0 and +0 stay
different, and so does everything finite.
"""
import traceback

import numpy as np

F32 = np.float32
PAD_REL = F32(2.0 ** -21)      # TR_PAD_REL
PAD_ABS = F32(2.0 ** -100)     # TR_PAD_ABS
FACE, ESUM, PAD1 = 9, 10, 11   # words of a 48-byte triangle record after the nine vertex floats


class StructureError(AssertionError):
    def __init__(self, check, message=""):
        super().__init__(f"{check}: {message}" if message else check)
        self.check = check


def _require(ok, check, message=""):
    if not ok:
        raise StructureError(check, message)


def _corners(v, f):
    v = np.ascontiguousarray(v, F32)
    f = np.asarray(f).astype(np.int64)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def _pad(x):
    return np.abs(x) * PAD_REL + PAD_ABS


def _padded(a, b, c):
    lo = np.fmin(np.fmin(a, b), c)
    hi = np.fmax(np.fmax(a, b), c)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([lo - _pad(lo), hi + _pad(hi)], axis=1).astype(F32)


def padded_boxes(v, f):
    """[n, 6] float32 = lo.xyz, hi.xyz of every triangle, each bound moved outward by |x| * 2^-21 + 2^-100 (tr_tri_box)"""
    return _padded(*_corners(v, f))


def bounds_of(boxes):
    """union of padded boxes: (mn[3], mx[3]) float32"""
    return (np.fmin.reduce(boxes[:, :3], axis=0, initial=F32(np.inf)).astype(F32),
            np.fmax.reduce(boxes[:, 3:], axis=0, initial=F32(-np.inf)).astype(F32))


def _spread21(x):
    x = x.astype(np.uint64) & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f),
                        (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def morton_keys(v, f):
    """uint64 [n]: tr_morton63 of every padded box inside the union of all of them"""
    box = padded_boxes(v, f)
    mn, mx = bounds_of(box)
    q = []
    with np.errstate(all="ignore"):
        for k in range(3):
            c = F32(0.5) * box[:, k] + F32(0.5) * box[:, 3 + k]
            ext = F32(mx[k] - mn[k])
            u = (c - mn[k]) / ext if ext > 0 else np.zeros(len(box), F32)
            u = np.fmin(np.fmax(u.astype(F32), F32(0)), F32(1))      # fminf(fmaxf(u, 0), 1): a NaN becomes 0
            s = (u * F32(2097152.0)).astype(F32)
            q.append(np.minimum(s.astype(np.int64), 2097151))      # truncation, capped at 2^21 - 1
    return (_spread21(q[0]) << np.uint64(2)) | (_spread21(q[1]) << np.uint64(1)) | _spread21(q[2])


def expected_order(v, f):
    """face ids in the order a STABLE sort by Morton key leaves them in"""
    return np.lexsort((np.arange(len(f)), morton_keys(v, f))).astype(np.int32)


def tri_records(v, f, order):
    """uint32 [n, 12]: the 48-byte triangle records of the faces `order`: nine vertex floats, face, esum, 0.
    esum = tr_tri_scale: ((|e1x| + |e1y|) + |e1z|) + ((|e2x| + |e2y|) + |e2z|), e1 = b - a, e2 = c - a, in float32"""
    order = np.asarray(order).astype(np.int64)
    a, b, c = _corners(v, np.asarray(f)[order])
    rec = np.zeros((len(order), 12), np.uint32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9] = a.view(np.uint32), b.view(np.uint32), c.view(np.uint32)
    rec[:, FACE] = order.astype(np.int32).view(np.uint32)
    with np.errstate(all="ignore"):
        e1, e2 = np.abs(b - a), np.abs(c - a)
        esum = ((e1[:, 0] + e1[:, 1]) + e1[:, 2]) + ((e2[:, 0] + e2[:, 1]) + e2[:, 2])
    rec[:, ESUM] = esum.astype(F32).view(np.uint32)
    return rec


def record_boxes(tris):
    """padded boxes of the triangles as the records hold them, [n, 6] float32, in slot order"""
    t = np.ascontiguousarray(tris[:, :9]).view(F32)
    return _padded(t[:, 0:3], t[:, 3:6], t[:, 6:9])


def _bits(x):
    return canon_bits(np.ascontiguousarray(x, F32))


def canon_bits(x):
    """float32 array (or its uint32 words) -> uint32 words with every NaN replaced by 0x7fc00000"""
    w = np.ascontiguousarray(x).view(np.uint32).copy()
    w[(w & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)] = np.uint32(0x7fc00000)
    return w


FLOAT_WORDS = {"nodes": slice(0, 12), "tris": [0, 1, 2, 3, 4, 5, 6, 7, 8, ESUM]}      # (the other words are ids: never touched)


def canon_arrays(nodes, links, tris, qnodes, frame):
    """the five arrays of a hierarchy with the NaNs of their float words made canonical, for byte comparisons"""
    nodes, tris = np.array(nodes, np.uint32), np.array(tris, np.uint32)
    if len(nodes):
        nodes[:, FLOAT_WORDS["nodes"]] = canon_bits(nodes[:, FLOAT_WORDS["nodes"]])
    if len(tris):
        tris[:, FLOAT_WORDS["tris"]] = canon_bits(tris[:, FLOAT_WORDS["tris"]])
    return nodes, links, tris, qnodes, canon_bits(np.asarray(frame, F32)).view(F32)


def check_leaf_boxes(nodes, tris):
    """every LEAF child box of every node == the padded box of that leaf's triangle, bit for bit
    (a node stores a child box as lo.x lo.y lo.z | hi.z hi.x hi.y)"""
    want = record_boxes(tris)[:, [0, 1, 2, 5, 3, 4]]
    c = nodes[:, 12:14].view(np.int32)
    for k in (0, 1):
        m = c[:, k] < 0
        slot = ~c[m, k].astype(np.int64)
        _require(np.all((slot >= 0) & (slot < len(tris))), "leaf_boxes", "a leaf id points outside the triangle array")
        got = canon_bits(nodes[m, 6 * k:6 * k + 6])
        bad = np.flatnonzero(np.any(got != _bits(want[slot]), axis=1))
        _require(len(bad) == 0, "leaf_boxes", f"{len(bad)} leaf boxes of child {k} differ from the padded triangle box, "
                                              f"first at node {np.flatnonzero(m)[bad[0]] if len(bad) else -1}")


def tree_height(nodes):
    """levels of internal nodes below and including the root, walked along the child ids (= the refit rounds the root
    needs: a node over two leaves has height 1)"""
    c = nodes[:, 12:14].view(np.int32)
    frontier = np.zeros(1, np.int64)
    seen, h = 0, 0
    while len(frontier):
        h += 1
        seen += len(frontier)
        _require(seen <= len(nodes), "height", "the child ids do not form a tree")
        ch = c[frontier].ravel()
        frontier = ch[ch >= 0].astype(np.int64)
    _require(seen == len(nodes), "height", f"{len(nodes) - seen} nodes cannot be reached from the root")
    return h


def _tree_part(line):
    if "qb[" in line or "qnodes" in line or "slack" in line:
        return "grid nodes"
    if "boxes[" in line:
        return "box nesting"
    if "par" in line or "sib" in line or "links" in line:
        return "links"
    return "topology"


def check_tree_named(B):
    """test_host_sim.check_tree, its AssertionError turned into a StructureError that names the part"""
    from test_host_sim import check_tree
    try:
        check_tree(B)
    except StructureError:
        raise
    except AssertionError as e:
        tb = traceback.extract_tb(e.__traceback__)
        line = next((fr.line for fr in reversed(tb) if fr.name == "check_tree"), "") or ""
        raise StructureError("tree: " + _tree_part(line), line) from e


def check_bounds(info, boxes):
    mn, mx = bounds_of(boxes)
    _require(np.array_equal(_bits(np.asarray(info["aabb_min"], F32)), _bits(mn)) and
             np.array_equal(_bits(np.asarray(info["aabb_max"], F32)), _bits(mx)), "bounds",
             f"aabb {info['aabb_min']} .. {info['aabb_max']}, union of the padded boxes {mn.tolist()} .. {mx.tolist()}")


def check_structure(v, f, nodes, links, tris, qnodes, frame, info, ref_frame=None, order=None):
    """All structural checks of one built (or refitted) hierarchy over the mesh (v, f); see the module docstring.
    info: dict with "depth", "aabb_min", "aabb_max" (RayMeshIntersector.bvh_info()).
    ref_frame: the grid frame of a SimBVH(v, f) if the caller has one already (it is built here otherwise).
    order: the face order the records must have -- expected_order(v, f) of a build (the default); a refit keeps the
    order of the mesh it was built from."""
    from sim import SimBVH
    nf = len(f)
    _require(len(tris) == nf and len(nodes) == max(nf - 1, 0) and len(links) == len(nodes) and len(qnodes) == len(nodes),
             "tree: topology", f"array sizes {len(nodes)} / {len(links)} / {len(qnodes)} / {len(tris)} for {nf} faces")
    want_order = expected_order(v, f) if order is None else np.asarray(order, np.int32)
    got_order = tris[:, FACE].view(np.int32)
    bad = np.flatnonzero(got_order != want_order)
    _require(len(bad) == 0, "order", f"{len(bad)} slots hold another face than the stable sort, first slot "
                                     f"{bad[0] if len(bad) else -1}")
    rec = tri_records(v, f, want_order)
    rec[:, FLOAT_WORDS["tris"]] = canon_bits(rec[:, FLOAT_WORDS["tris"]])
    bad = np.flatnonzero(np.any(rec != canon_arrays(np.zeros((0, 16), np.uint32), None, tris, None, np.zeros(6, F32))[2], axis=1))
    _require(len(bad) == 0, "records", f"{len(bad)} triangle records differ, first slot {bad[0] if len(bad) else -1}")
    boxes = padded_boxes(v, f)
    if nf >= 2:
        check_leaf_boxes(nodes, tris)
        check_tree_named(SimBVH(arrays=(nodes, links, tris), qarrays=(qnodes, frame)))
        h = tree_height(nodes)
        _require(h == info["depth"] and h <= 64, "height", f"walked {h}, reported {info['depth']}")
    check_bounds(info, boxes)
    if ref_frame is None:
        ref_frame = SimBVH(v, f).frame
    _require(np.array_equal(_bits(frame), _bits(ref_frame)), "frame", f"{np.asarray(frame).tolist()} != {np.asarray(ref_frame).tolist()}")
