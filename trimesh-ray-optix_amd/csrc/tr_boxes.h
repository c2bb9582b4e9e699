// tr_boxes.h -- box queries (include/triro_boxes.h): the faces of a mesh that meet an axis-aligned box.  Host + device, as
// tr_within.h, whose ordering it uses UNCHANGED, on the set walk and the row limit of tr_walk.h: k_boxes<> and k_boxes_rows (boxes.hip) instantiate the walk
// per lane, tests/host_sim/boxes_sim.cpp compiles the very same functions with g++.  Not a CPU fallback: nothing in the C
// ABI reaches the host instantiation.
//
// THE CONTRACT.  Query: a closed axis-aligned box [lo, hi] of six float32; the mesh of the handle.
//
//  * The query is VALID iff all six values are finite and lo_k <= hi_k on every axis.  Flat boxes, lines and points are
//    valid, +-FLT_MAX bounds are valid (the box [-FLT_MAX, FLT_MAX]^3 meets every active face: THE SHORTCUT).  A NaN, an
//    infinity or lo_k > hi_k on any axis makes it invalid.
//  * A triangle with a non-finite coordinate is INACTIVE (tr_near_active, as everywhere) and is never met.
//  * Face T = (a, b, c) MEETS the box iff T is active and tr_box_meets says so: the closed triangle and the closed box share
//    a point -- touching counts.  tr_box_meets is ONE FIXED SEQUENCE:
//      1. the three box axes, in float32, exact: max(a_k, b_k, c_k) < lo_k or min(a_k, b_k, c_k) > hi_k -> separated.
//      2. THE SHORTCUT, float32, exact: a vertex with lo_k <= v_k <= hi_k on every axis -> met.
//      3. the triangle's plane, float64 from the float32 inputs (-ffp-contract=off holds, fma only where written): e0 = b - a,
//         e1 = c - b, n = e0 x e1; with the box's extreme corners along n, m_k = (n_k >= 0 ? lo_k : hi_k) and M_k the other
//         one: dmin = n . (m - a), dmax = n . (M - a) (tr_near_dot of the rounded differences); dmin > 0 or dmax < 0 ->
//         separated.
//      4. the nine axes L = u_i x e_j (u_i a box axis, e_j the edge from vertex v to the next; w = the third vertex), j outer,
//         i = x, y, z inner.  L has two non-zero components (L_p, L_q) = (-e_z, e_y), (e_z, -e_x), (-e_y, e_x) on the
//         coordinates (p, q) = (y, z), (x, z), (x, y).  Everything is measured from v: the triangle spans [min(0, t),
//         max(0, t)] with t = fma(L_q, w_q - v_q, L_p * (w_p - v_p)) (both ends of the edge project to 0), the box spans
//         [bmin, bmax], the same expression at the corners (L_p >= 0 ? lo_p : hi_p, ..) and the opposite ones;
//         bmin > max(0, t) or bmax < min(0, t) -> separated.
//      5. otherwise met.
//    Separation is always strict: equality never separates.  Everything is in lo / hi form, measured from a vertex: no centre,
//    no half size, no rounding that the inputs did not ask for.  Differences of float32 are at most 6.9e38, n at most 1e78,
//    the dots at most 2e117: nothing overflows, finite inputs never give NaN.  A triangle that is a segment or a point needs
//    no special case: n = 0 or L = 0 gives 0 on both sides, which separates nothing, and the remaining axes are complete for
//    a segment (3 box axes, 3 cross axes) and a point (3 box axes).
//    On inputs whose coordinates are all k * 2^-10 with |k| <= 2^12 every operation is EXACT (differences <= 2^13 units,
//    products and n <= 2^27, dots <= 2^42 < 2^53): there the predicate IS the separating-axis theorem.
//  * INSIDE (optional per row): 1 iff all three vertices lie in the box -- exact float32 comparisons (tr_box_has).
//  * any = at least one face meets the box (uint8); count = how many do (int32); list = those faces by ORIGINAL FACE INDEX,
//    ASCENDING, at rows offsets[i] .. offsets[i] + count[i] (uncapped; int64 offsets from tr_hits_scan), `inside` at the same
//    rows where asked for.
//  * An invalid query, a mesh of zero triangles or one without an active triangle: any = 0, count = 0, an empty list.  Every
//    element of every output is written.
//  * Everything is a pure function of (box, the set of triangles): independent of traversal order, stack capacity and launch
//    shape.
//
// CULLING.  A subtree is skipped iff its node box and the query box are disjoint on some axis: node_hi_k < lo_k or
// node_lo_k > hi_k, strict float32 comparisons (tr_box_apart); a NaN in a node box compares false and never culls.
// PROOF: every triangle below a node has its vertices in the node's box (the leaf box in a parent is the padded triangle box,
// a superset), so max(a_k, b_k, c_k) <= node_hi_k < lo_k or min(a_k, b_k, c_k) >= node_lo_k > hi_k: step 1 of the predicate
// separates it, with the same exact comparisons.  A skipped subtree holds no face that meets the box.  No rounding argument.
//
// THE WALK is THE SET WALK of tr_walk.h with this culling and this leaf: of the internal children that survive, child 0 is
// visited next and child 1 pushed (no order is better than another: the whole set is wanted); TR_BOXES_STACK = 32 node ids
// per lane.  The stack, the row limit and the ordering are the shared ones; tr_boxes_visit, tr_boxes_rewalk, tr_boxes_query and
// the body of k_boxes are tr_set_visit, tr_rewalk, tr_set_query and tr_set_kernel WRITTEN OUT: built on those (as tr_tris.h
// is, through tr_set_probe below) the kernels kept their registers and LDS but the FILL instantiation was laid out anew,
// and faces_in_boxes on hashed boxes measured 0.5 % slower than the commit before, outside the spread of that commit
// against itself -- so this kernel keeps its text, and compiles to the same instructions as before.
// FILL writes, in walk order and never beyond `limit` = tr_rows_limit(count, offset, total) rows, one KEY per face:
// tr_boxes_key = (2 * face + inside) with the top bit flipped, an int32 whose signed order is the order of the faces -- the
// `inside` flag rides through the ordering without scratch.  tr_boxes_rows then orders the segment (tr_within_sort) and
// unpacks face and inside.
#pragma once
#include "tr_within.h"

#define TR_BOXES_STACK 32      // node ids per lane: 32 x 4 B x 128 lanes = 16 KB of LDS per workgroup

enum tr_boxes_mode { TR_BOXES_ANY = TR_SET_ANY, TR_BOXES_COUNT = TR_SET_COUNT, TR_BOXES_FILL = TR_SET_FILL };

struct tr_box { float lox, loy, loz, hix, hiy, hiz; };

// what a lane has found: `count` faces, of which the first min(count, limit) were written (FILL)
struct tr_boxes_acc {
    int32_t count;
    int32_t limit;      // FILL: rows this box may write
    int32_t* key;       // FILL: its rows of the face list (keys until tr_boxes_rows)
};

TR_HD bool tr_box_valid(const tr_box& q) {
    return tr_finite(q.lox) && tr_finite(q.loy) && tr_finite(q.loz) && tr_finite(q.hix) && tr_finite(q.hiy) && tr_finite(q.hiz) &&
           q.lox <= q.hix && q.loy <= q.hiy && q.loz <= q.hiz;
}
// a point in the closed box
TR_HD bool tr_box_has(const tr_box& q, float x, float y, float z) {
    return q.lox <= x && x <= q.hix && q.loy <= y && y <= q.hiy && q.loz <= z && z <= q.hiz;
}
TR_HD bool tr_box_inside(const tr_box& q, const tr_tri& t) {
    return tr_box_has(q, t.ax, t.ay, t.az) && tr_box_has(q, t.bx, t.by, t.bz) && tr_box_has(q, t.cx, t.cy, t.cz);
}
// CULLING: the box [lo, hi] of a node and the query are disjoint on some axis (a NaN compares false: never apart)
TR_HD bool tr_box_apart(const tr_box& q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    return hix < q.lox || lox > q.hix || hiy < q.loy || loy > q.hiy || hiz < q.loz || loz > q.hiz;
}

// step 4 of the predicate: one axis L = (L_p, L_q) on the coordinates (p, q), measured from the edge's first vertex v
TR_HD bool tr_box_axis(double Lp, double Lq, double lop, double hip, double loq, double hiq, double vp, double vq, double wp, double wq) {
    const double t = fma(Lq, wq - vq, Lp * (wp - vp));
    const bool sp = Lp >= 0.0, sq = Lq >= 0.0;
    const double bmin = fma(Lq, (sq ? loq : hiq) - vq, Lp * ((sp ? lop : hip) - vp));
    const double bmax = fma(Lq, (sq ? hiq : loq) - vq, Lp * ((sp ? hip : lop) - vp));
    return bmin > (t > 0.0 ? t : 0.0) || bmax < (t < 0.0 ? t : 0.0);
}
// the three axes u_i x e of the edge e = (v -> next vertex), w = the third vertex
TR_HD bool tr_box_edge(const double* lo, const double* hi, double vx, double vy, double vz, double ex, double ey, double ez, double wx,
                       double wy, double wz) {
    return tr_box_axis(-ez, ey, lo[1], hi[1], lo[2], hi[2], vy, vz, wy, wz) ||
           tr_box_axis(ez, -ex, lo[0], hi[0], lo[2], hi[2], vx, vz, wx, wz) ||
           tr_box_axis(-ey, ex, lo[0], hi[0], lo[1], hi[1], vx, vy, wx, wy);
}
// THE PREDICATE on finite coordinates (see THE CONTRACT; activity is the caller's)
TR_HD bool tr_box_meets(const tr_box& q, float axf, float ayf, float azf, float bxf, float byf, float bzf, float cxf, float cyf, float czf) {
    // 1. the box axes
    if (fmaxf(fmaxf(axf, bxf), cxf) < q.lox || fminf(fminf(axf, bxf), cxf) > q.hix) return false;
    if (fmaxf(fmaxf(ayf, byf), cyf) < q.loy || fminf(fminf(ayf, byf), cyf) > q.hiy) return false;
    if (fmaxf(fmaxf(azf, bzf), czf) < q.loz || fminf(fminf(azf, bzf), czf) > q.hiz) return false;
    // 2. the shortcut
    if (tr_box_has(q, axf, ayf, azf) || tr_box_has(q, bxf, byf, bzf) || tr_box_has(q, cxf, cyf, czf)) return true;
    const double lo[3] = {(double)q.lox, (double)q.loy, (double)q.loz}, hi[3] = {(double)q.hix, (double)q.hiy, (double)q.hiz};
    const double ax = axf, ay = ayf, az = azf, bx = bxf, by = byf, bz = bzf, cx = cxf, cy = cyf, cz = czf;
    const double e0x = bx - ax, e0y = by - ay, e0z = bz - az;
    const double e1x = cx - bx, e1y = cy - by, e1z = cz - bz;
    {   // 3. the plane
        const double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
        const bool sx = nx >= 0.0, sy = ny >= 0.0, sz = nz >= 0.0;
        const double dmin = tr_near_dot((sx ? lo[0] : hi[0]) - ax, (sy ? lo[1] : hi[1]) - ay, (sz ? lo[2] : hi[2]) - az, nx, ny, nz);
        const double dmax = tr_near_dot((sx ? hi[0] : lo[0]) - ax, (sy ? hi[1] : lo[1]) - ay, (sz ? hi[2] : lo[2]) - az, nx, ny, nz);
        if (dmin > 0.0 || dmax < 0.0) return false;
    }
    // 4. the nine cross axes
    if (tr_box_edge(lo, hi, ax, ay, az, e0x, e0y, e0z, cx, cy, cz)) return false;
    if (tr_box_edge(lo, hi, bx, by, bz, e1x, e1y, e1z, ax, ay, az)) return false;
    if (tr_box_edge(lo, hi, cx, cy, cz, ax - cx, ay - cy, az - cz, bx, by, bz)) return false;
    return true;
}

// a face and its `inside` flag as one int32 whose signed order is the order of the faces (face >= 0)
TR_HD int32_t tr_boxes_key(int32_t face, bool inside) { return (int32_t)((2u * (uint32_t)face + (inside ? 1u : 0u)) ^ 0x80000000u); }
TR_HD int32_t tr_boxes_key_face(int32_t key) { return (int32_t)(((uint32_t)key ^ 0x80000000u) >> 1); }
TR_HD bool tr_boxes_key_inside(int32_t key) { return ((uint32_t)key & 1u) != 0; }

// one triangle against the box
template <int MODE>
TR_HD void tr_boxes_leaf(const tr_bvh_view& b, int32_t slot, const tr_box& q, tr_boxes_acc& acc) {
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    if (tr_near_active(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz) &&
        tr_box_meets(q, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz)) {
        if (MODE == TR_BOXES_FILL && acc.count < acc.limit) acc.key[acc.count] = tr_boxes_key(t.face, tr_box_inside(q, t));
        acc.count++;
    }
}

// both child ids of an internal node and whether the query is apart from each child box
struct tr_boxes_node { int32_t c0, c1; bool apart0, apart1; };
TR_HD tr_boxes_node tr_boxes_load(const tr_bvh_view& b, int32_t node, const tr_box& q) {
    const tr_f4* p = reinterpret_cast<const tr_f4*>(b.nodes + node);
    const tr_f4 n0 = p[0], n1 = p[1], n2 = p[2], n3 = p[3];      // lo.x lo.y lo.z hi.z | hi.x hi.y lo.x lo.y | lo.z hi.z hi.x hi.y | c0 c1 ..
    tr_boxes_node r;
    r.apart0 = tr_box_apart(q, n0.x, n0.y, n0.z, n1.x, n1.y, n0.w);
    r.apart1 = tr_box_apart(q, n1.z, n1.w, n2.x, n2.z, n2.w, n2.y);
    r.c0 = (int32_t)tr_f2u(n3.x); r.c1 = (int32_t)tr_f2u(n3.y);
    return r;
}

// visit st.node (>= 0): see THE WALK
template <int MODE>
TR_HD void tr_boxes_visit(const tr_bvh_view& b, const tr_box& q, tr_walk_state& st, tr_boxes_acc& acc, const tr_ring stack, uint32_t cap2) {
    const tr_boxes_node n = tr_boxes_load(b, st.node, q);
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? n.c1 : n.c0;
        const bool apart = k ? n.apart1 : n.apart0;
        if (c < 0 && !apart && !tr_set_full<MODE>(acc)) tr_boxes_leaf<MODE>(b, ~c, q, acc);
    }
    if (tr_set_full<MODE>(acc)) { st.node = -1; return; }
    const bool go0 = n.c0 >= 0 && !n.apart0, go1 = n.c1 >= 0 && !n.apart1;
    if (go0) {
        if (go1) tr_walk_push(stack, cap2, st.sp, n.c1);
        st.node = n.c0;
    } else if (go1) {
        st.node = n.c1;
    } else {
        st.node = tr_walk_pop(stack, st.sp);
    }
}

// the whole tree again without a stack (after a lost push; the caller has reset acc.count): the loop of tr_rewalk (tr_walk.h)
// written out, as the visit above and tr_boxes_query below are tr_set_visit's and tr_set_query's -- see THE WALK for why
template <int MODE>
TR_HD void tr_boxes_rewalk(const tr_bvh_view& b, const tr_box& q, tr_boxes_acc& acc) {
    int32_t node = 0;
    int phase = 0;
    for (;;) {
        if (tr_set_full<MODE>(acc)) break;
        if (phase == 2) {
            const int32_t parent = b.links[node].parent;
            if (parent < 0) break;
            phase = b.nodes[parent].c0 == node ? 1 : 2;
            node = parent;
            continue;
        }
        const tr_boxes_node n = tr_boxes_load(b, node, q);
        const int32_t c = phase ? n.c1 : n.c0;
        const bool apart = phase ? n.apart1 : n.apart0;
        phase++;
        if (apart) continue;
        if (c < 0) {
            tr_boxes_leaf<MODE>(b, ~c, q, acc);
        } else {
            node = c;
            phase = 0;
        }
    }
}

// THE SET WALK ON A BOX (tr_walk.h), for a query that culls by an axis-aligned box `box` and evaluates a leaf with
// leaf(slot, acc): tris with the box of the query triangle.  Visit st.node (>= 0): of the internal children whose boxes the
// query's box is not apart from, child 0 is visited next and child 1 pushed.
template <int MODE, class Leaf>
TR_HD void tr_set_visit(const tr_bvh_view& b, const tr_box& box, const Leaf& leaf, tr_walk_state& st, tr_boxes_acc& acc,
                        const tr_ring stack, uint32_t cap2) {
    const tr_boxes_node n = tr_boxes_load(b, st.node, box);
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? n.c1 : n.c0;
        const bool apart = k ? n.apart1 : n.apart0;
        if (c < 0 && !apart && !tr_set_full<MODE>(acc)) leaf(~c, acc);
    }
    if (tr_set_full<MODE>(acc)) { st.node = -1; return; }
    const bool go0 = n.c0 >= 0 && !n.apart0, go1 = n.c1 >= 0 && !n.apart1;
    if (go0) {
        if (go1) tr_walk_push(stack, cap2, st.sp, n.c1);
        st.node = n.c0;
    } else if (go1) {
        st.node = n.c1;
    } else {
        st.node = tr_walk_pop(stack, st.sp);
    }
}
// ... and the query as tr_walk.h sees it (tr_rewalk, tr_set_query, tr_set_kernel)
template <int MODE, class Leaf>
struct tr_set_probe {
    const tr_bvh_view& b;
    const tr_box& box;
    const Leaf test;
    tr_boxes_acc& acc;
    TR_HDM bool done() const { return tr_set_full<MODE>(acc); }
    TR_HDM void leaf(int32_t slot) const { test(slot, acc); }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_boxes_node n = tr_boxes_load(b, node, box);
        c = phase ? n.c1 : n.c0;
        return !(phase ? n.apart1 : n.apart0);
    }
    TR_HDM void visit(tr_walk_state& st, const tr_ring stack, uint32_t cap2) const {
        tr_set_visit<MODE>(b, box, test, st, acc, stack, cap2);
    }
};
// order the m rows (keys) of a box, then unpack them: face in place, inside where asked for
TR_HD void tr_boxes_rows(int32_t* face, uint8_t* inside, int32_t m) {
    tr_within_sort(face, nullptr, m);
    for (int32_t k = 0; k < m; k++) {
        const int32_t key = face[k];
        face[k] = tr_boxes_key_face(key);
        if (inside) inside[k] = tr_boxes_key_inside(key) ? 1 : 0;
    }
}

// one box, start to end, on one lane (the host simulation; the kernel runs the first walk as a wave loop).
// stack_entries: 1 .. TR_BOXES_STACK, 0 = all of them.  Returns the number of faces met (FILL: min(it, acc.limit) keys are
// written and still in walk order); *lost (may be null): the first walk overflowed its stack.
template <int MODE>
TR_HD int32_t tr_boxes_query(const tr_bvh_view& b, const tr_box& q, const tr_ring stack, int stack_entries, tr_boxes_acc& acc, bool* lost) {
    const bool valid = tr_box_valid(q) && b.num_tris > 0;
    acc.count = 0;
    if (lost) *lost = false;
    if (valid && b.num_tris >= 2 && !tr_set_full<MODE>(acc)) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_BOXES_STACK);
        tr_walk_state st;
        st.node = 0; st.sp = 0;
        while (st.node >= 0) tr_boxes_visit<MODE>(b, q, st, acc, stack, cap2);
        if (lost) *lost = tr_walk_lost(st.sp);
        if (tr_walk_lost(st.sp) && !tr_set_full<MODE>(acc)) {
            acc.count = 0;
            tr_boxes_rewalk<MODE>(b, q, acc);
        }
    } else if (valid && !tr_set_full<MODE>(acc)) {
        tr_boxes_leaf<MODE>(b, 0, q, acc);      // no hierarchy below two triangles
    }
    return acc.count;
}
