// tr_tris.h -- triangle queries (include/triro_tris.h): the faces of a mesh that meet a triangle, the narrow phase of mesh
// against mesh.  Host + device, as tr_boxes.h, whose culling (tr_box_apart, tr_boxes_load), result record (tr_boxes_acc,
// tr_set_probe) and -- through tr_within.h and tr_walk.h -- stack, row limit and ordering it uses UNCHANGED: k_tris<> and k_tris_rows
// (tris.hip) instantiate the walk per lane, tests/host_sim/tris_sim.cpp compiles the very same functions with g++.  Not a CPU
// fallback: nothing in the C ABI reaches the host instantiation.
//
// THE CONTRACT.  Query: a triangle Q = (p, q, r) of nine float32; the mesh of the handle.
//
//  * The query is VALID iff all nine values are finite.
//  * A mesh face with a non-finite coordinate is INACTIVE (tr_near_active, as everywhere) and is never met.
//  * DEGENERATE TRIANGLES.  A triangle, on either side, is degenerate when its float64 normal, computed by the fixed
//    expression of step 2 below, is exactly (0, 0, 0).  A degenerate mesh face is never met; a degenerate query meets nothing,
//    although it is valid.  THIS IS DELIBERATE AND DIFFERS FROM THE BOX QUERY (tr_boxes.h), which accepts segments and points:
//    the seventeen axes below are complete only for two triangles with area -- a segment coplanar with a triangle would need
//    more axes.  A float32 difference cannot underflow in float64 (the smallest non-zero one is 2^-149) and neither can a
//    product of two (>= 2^-298), so n is 0 only through cancellation; on the lattice of EXACTNESS that is exact collinearity.
//  * Face T = (a, b, c) MEETS Q iff T is active, both have area and tr_tris_meets says so: the closed triangles share a point
//    -- touching counts.  tr_tris_meets is ONE FIXED SEQUENCE (-ffp-contract=off holds, fma only where written):
//      1. the three coordinate axes, in float32, exact: max(a_k, b_k, c_k) < min(p_k, q_k, r_k) or min(a_k, b_k, c_k) >
//         max(p_k, q_k, r_k) -> separated.
//      2. in float64 from the float32 inputs: the edges of T, e0 = b - a, e1 = c - b, e2 = a - c, those of Q, f0 = q - p,
//         f1 = r - q, f2 = p - r, and the vertices of Q seen from a: dp = p - a, dq = q - a, dr = r - a.  Every cross product is
//         x x y = (x_y y_z - x_z y_y, x_z y_x - x_x y_z, x_x y_y - x_y y_x), two rounded products and their rounded
//         difference per component.  n_T = e0 x e1, n_Q = f0 x f1; n_T = 0 or n_Q = 0 -> not met (DEGENERATE).
//      3. seventeen axes L: n_T, n_Q, the nine e_i x f_j, n_T x e_0, n_T x e_1, n_T x e_2, n_Q x f_0, n_Q x f_1, n_Q x f_2.
//         The result is the OR over them and no comparison involves a NaN, so the order is immaterial; tr_tris_sat walks
//         n_T, n_Q, then per edge e_i of T: n_T x e_i, e_i x f_0, e_i x f_1, e_i x f_2, then the n_Q x f_j.  Everything is
//         measured from a: with x . y = tr_near_dot(x, y) = fma(x_z, y_z,
//         fma(x_y, y_y, x_x y_x)), T spans [min(0, t1, t2), max(0, t1, t2)], t1 = e0 . L, t2 = (-e2) . L (c - a = -e2, the
//         same float64 number), Q spans [min, max] of dp . L, dq . L, dr . L.  Q's minimum > T's maximum or Q's maximum < T's
//         minimum -> separated.
//      4. otherwise met.
//    Separation is always strict: equality never separates.  An axis L = 0 (parallel edges) projects everything to 0 and
//    separates nothing.
//  * OVERFLOW.  |float32| <= 3.41e38, so a difference is at most 6.81e38 < 6.9e38; a component of a cross product of two
//    differences (n_T, n_Q, e_i x f_j) at most 2 * (6.81e38)^2 = 9.3e77 < 1e78; a component of n x e at most 2 * 9.3e77 *
//    6.81e38 = 1.27e117 < 1.3e117; a dot of such an axis with a difference at most 3 * 1.27e117 * 6.81e38 = 2.6e155 < 3e155,
//    far below DBL_MAX = 1.8e308.  Nothing overflows, no Inf - Inf or 0 * Inf arises: finite inputs never give NaN, and every
//    comparison above is between numbers.
//  * EXACTNESS.  On inputs whose coordinates are all k * 2^-10 with |k| <= 2^11 every operation is EXACT, in units of the
//    lattice: differences <= 2^12, products <= 2^24 and the components of n and e x f <= 2^25, products n_k e_l <= 2^37 and
//    the components of n x e <= 2^38, the products of a dot <= 2^50 and its partial and full sums <= 3 * 2^50 < 2^52 < 2^53:
//    integers that float64 holds, so every fma and every subtraction rounds nothing.  There the predicate IS the
//    separating-axis theorem on the seventeen axes, and those suffice: two normals and nine edge crosses for a pair in
//    general position, and for a coplanar pair, where all of those are parallel to the one normal or zero, the six in-plane
//    edge normals n x e of the two convex polygons.
//  * any = at least one face meets Q (uint8); count = how many do (int32); list = those faces by ORIGINAL FACE INDEX,
//    ASCENDING, at rows offsets[i] .. offsets[i] + count[i] (uncapped; int64 offsets from tr_hits_scan).
//  * An invalid or degenerate query, a mesh of zero triangles or one without an active face with area: any = 0, count = 0, an
//    empty list.  Every element of every output is written.
//  * Everything is a pure function of (Q, the set of triangles): independent of traversal order, stack capacity and launch
//    shape.
//
// CULLING.  A subtree is skipped iff the float32 box of Q (min / max of its three vertices, exact; computed once per query,
// tr_tris_box) and the node box are disjoint on some axis: tr_box_apart on Q's box; a NaN in a node box compares false and
// never culls.  PROOF (the box query's): every triangle below a node has its vertices in the node's box (the leaf box in a
// parent is the padded triangle box, a superset), so max(a_k, b_k, c_k) <= node_hi_k < min(p_k, q_k, r_k) or the mirror image:
// step 1 of the predicate separates it, with the same exact comparisons.  A skipped subtree holds no face that meets Q.  No
// rounding argument.
//
// THE WALK is the set walk of tr_boxes.h on Q's box (tr_set_probe; THE SET WALK of tr_walk.h) with this leaf;
// TR_TRIS_STACK = 32 node ids per lane.
// FILL writes, in walk order and never beyond `limit` = tr_rows_limit(count, offset, total) rows, the face index itself (no
// flag rides along: the rows are plain face indices); tr_tris_rows then orders the segment (tr_within_sort).
//
// REGISTERS.  The float64 part never holds the seventeen axes: tr_tris_sat keeps the frame (e0, -e2, dp, dq, dr), the edges
// e1, f0, f1, f2 and the two normals, and forms one axis at a time (tr_tris_axis) in rolled loops, testing it before the next
// is computed: written as one straight-line expression the compiler evaluates several axes at once (134 - 138 VGPRs, three
// waves per SIMD); rolled it is 122 - 126, four waves, no scratch.
#pragma once
#include "tr_boxes.h"

#define TR_TRIS_STACK 32       // node ids per lane: 32 x 4 B x 128 lanes = 16 KB of LDS per workgroup

enum tr_tris_mode { TR_TRIS_ANY = TR_BOXES_ANY, TR_TRIS_COUNT = TR_BOXES_COUNT, TR_TRIS_FILL = TR_BOXES_FILL };

struct tr_tris_q { float px, py, pz, qx, qy, qz, rx, ry, rz; };

struct tr_tris_v3 { double x, y, z; };

// what every axis is measured against: T's and Q's vertices seen from vertex a of T (a itself is 0)
struct tr_tris_frame { tr_tris_v3 u1, u2, dp, dq, dr; };

TR_HD tr_tris_v3 tr_tris_sub(float ax, float ay, float az, float bx, float by, float bz) {
    tr_tris_v3 r;
    r.x = (double)ax - (double)bx; r.y = (double)ay - (double)by; r.z = (double)az - (double)bz;
    return r;
}
TR_HD tr_tris_v3 tr_tris_cross(const tr_tris_v3& a, const tr_tris_v3& b) {
    tr_tris_v3 r;
    r.x = a.y * b.z - a.z * b.y; r.y = a.z * b.x - a.x * b.z; r.z = a.x * b.y - a.y * b.x;
    return r;
}
TR_HD bool tr_tris_zero(const tr_tris_v3& n) { return n.x == 0.0 && n.y == 0.0 && n.z == 0.0; }

TR_HD bool tr_tris_valid(const tr_tris_q& q) {
    return tr_finite(q.px) && tr_finite(q.py) && tr_finite(q.pz) && tr_finite(q.qx) && tr_finite(q.qy) && tr_finite(q.qz) &&
           tr_finite(q.rx) && tr_finite(q.ry) && tr_finite(q.rz);
}
// a triangle of finite float32 coordinates has area: its float64 normal (step 2) is not exactly 0
TR_HD bool tr_tris_area(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    return !tr_tris_zero(tr_tris_cross(tr_tris_sub(bx, by, bz, ax, ay, az), tr_tris_sub(cx, cy, cz, bx, by, bz)));
}
// a query that can meet a face at all: valid and with area (the walk is skipped otherwise)
TR_HD bool tr_tris_live(const tr_tris_q& q) {
    return tr_tris_valid(q) && tr_tris_area(q.px, q.py, q.pz, q.qx, q.qy, q.qz, q.rx, q.ry, q.rz);
}
// CULLING: the float32 box of Q, exact
TR_HD tr_box tr_tris_box(const tr_tris_q& q) {
    tr_box b;
    b.lox = fminf(fminf(q.px, q.qx), q.rx); b.loy = fminf(fminf(q.py, q.qy), q.ry); b.loz = fminf(fminf(q.pz, q.qz), q.rz);
    b.hix = fmaxf(fmaxf(q.px, q.qx), q.rx); b.hiy = fmaxf(fmaxf(q.py, q.qy), q.ry); b.hiz = fmaxf(fmaxf(q.pz, q.qz), q.rz);
    return b;
}

// step 3 of the predicate: the axis L separates T and Q
TR_HD bool tr_tris_axis(const tr_tris_frame& w, const tr_tris_v3& L) {
    const double t1 = tr_near_dot(w.u1.x, w.u1.y, w.u1.z, L.x, L.y, L.z), t2 = tr_near_dot(w.u2.x, w.u2.y, w.u2.z, L.x, L.y, L.z);
    const double s0 = tr_near_dot(w.dp.x, w.dp.y, w.dp.z, L.x, L.y, L.z), s1 = tr_near_dot(w.dq.x, w.dq.y, w.dq.z, L.x, L.y, L.z);
    const double s2 = tr_near_dot(w.dr.x, w.dr.y, w.dr.z, L.x, L.y, L.z);
    double tlo = t1 < t2 ? t1 : t2, thi = t1 < t2 ? t2 : t1;
    tlo = tlo < 0.0 ? tlo : 0.0; thi = thi > 0.0 ? thi : 0.0;
    double slo = s0 < s1 ? s0 : s1, shi = s0 < s1 ? s1 : s0;
    slo = slo < s2 ? slo : s2; shi = shi > s2 ? shi : s2;
    return slo > thi || shi < tlo;
}
// the k-th of three vectors (selects, no memory: the loops of tr_tris_sat stay rolled so that one axis is live at a time)
TR_HD tr_tris_v3 tr_tris_pick(int k, const tr_tris_v3& v0, const tr_tris_v3& v1, const tr_tris_v3& v2) {
    tr_tris_v3 r;
    r.x = k == 0 ? v0.x : (k == 1 ? v1.x : v2.x); r.y = k == 0 ? v0.y : (k == 1 ? v1.y : v2.y); r.z = k == 0 ? v0.z : (k == 1 ? v1.z : v2.z);
    return r;
}

// steps 2 - 4 of the predicate on finite coordinates: the degenerate rule and the seventeen axes
TR_HD bool tr_tris_sat(const tr_tris_q& q, float axf, float ayf, float azf, float bxf, float byf, float bzf, float cxf, float cyf, float czf) {
    tr_tris_frame w;
    w.u1 = tr_tris_sub(bxf, byf, bzf, axf, ayf, azf);                       // e0
    const tr_tris_v3 e1 = tr_tris_sub(cxf, cyf, czf, bxf, byf, bzf);
    const tr_tris_v3 e2 = tr_tris_sub(axf, ayf, azf, cxf, cyf, czf);
    w.u2.x = -e2.x; w.u2.y = -e2.y; w.u2.z = -e2.z;                         // c - a
    const tr_tris_v3 nT = tr_tris_cross(w.u1, e1);
    if (tr_tris_zero(nT)) return false;
    const tr_tris_v3 f0 = tr_tris_sub(q.qx, q.qy, q.qz, q.px, q.py, q.pz);
    const tr_tris_v3 f1 = tr_tris_sub(q.rx, q.ry, q.rz, q.qx, q.qy, q.qz);
    const tr_tris_v3 nQ = tr_tris_cross(f0, f1);
    if (tr_tris_zero(nQ)) return false;
    const tr_tris_v3 f2 = tr_tris_sub(q.px, q.py, q.pz, q.rx, q.ry, q.rz);
    w.dp = tr_tris_sub(q.px, q.py, q.pz, axf, ayf, azf);
    w.dq = tr_tris_sub(q.qx, q.qy, q.qz, axf, ayf, azf);
    w.dr = tr_tris_sub(q.rx, q.ry, q.rz, axf, ayf, azf);
    if (tr_tris_axis(w, nT) || tr_tris_axis(w, nQ)) return false;
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        const tr_tris_v3 e = tr_tris_pick(i, w.u1, e1, e2);
        if (tr_tris_axis(w, tr_tris_cross(nT, e))) return false;
#pragma unroll 1
        for (int j = 0; j < 3; j++)
            if (tr_tris_axis(w, tr_tris_cross(e, tr_tris_pick(j, f0, f1, f2)))) return false;
    }
#pragma unroll 1
    for (int j = 0; j < 3; j++)
        if (tr_tris_axis(w, tr_tris_cross(nQ, tr_tris_pick(j, f0, f1, f2)))) return false;
    return true;
}

// THE PREDICATE on finite coordinates (see THE CONTRACT; activity is the caller's).  qb = tr_tris_box(q)
TR_HD bool tr_tris_meets(const tr_tris_q& q, const tr_box& qb, float axf, float ayf, float azf, float bxf, float byf, float bzf, float cxf,
                         float cyf, float czf) {
    // 1. the coordinate axes
    if (fmaxf(fmaxf(axf, bxf), cxf) < qb.lox || fminf(fminf(axf, bxf), cxf) > qb.hix) return false;
    if (fmaxf(fmaxf(ayf, byf), cyf) < qb.loy || fminf(fminf(ayf, byf), cyf) > qb.hiy) return false;
    if (fmaxf(fmaxf(azf, bzf), czf) < qb.loz || fminf(fminf(azf, bzf), czf) > qb.hiz) return false;
    return tr_tris_sat(q, axf, ayf, azf, bxf, byf, bzf, cxf, cyf, czf);
}

// one face against the query (qb = tr_tris_box(q)): the leaf of the set walk of tr_boxes.h on qb
template <int MODE>
struct tr_tris_leaf {
    const tr_bvh_view& b;
    const tr_tris_q& q;
    const tr_box& qb;
    TR_HDM void operator()(int32_t slot, tr_boxes_acc& acc) const {
        tr_counters* nc = nullptr;
        const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
        if (tr_near_active(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz) &&
            tr_tris_meets(q, qb, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz)) {
            if (MODE == TR_TRIS_FILL && acc.count < acc.limit) acc.key[acc.count] = t.face;
            acc.count++;
        }
    }
};
template <int MODE>
TR_HD tr_set_probe<MODE, tr_tris_leaf<MODE>> tr_tris_probe(const tr_bvh_view& b, const tr_tris_q& q, const tr_box& qb, tr_boxes_acc& acc) {
    return {b, qb, {b, q, qb}, acc};
}

// order the m rows of a query: plain face indices, ascending
TR_HD void tr_tris_rows(int32_t* face, int32_t m) { tr_within_sort(face, nullptr, m); }

// one query, start to end, on one lane (the host simulation: tr_set_query); stack_entries: 1 .. TR_TRIS_STACK, 0 = all of them
template <int MODE>
TR_HD int32_t tr_tris_query(const tr_bvh_view& b, const tr_tris_q& q, const tr_ring stack, int stack_entries, tr_boxes_acc& acc, bool* lost) {
    const tr_box qb = tr_tris_box(q);
    return tr_set_query(b, tr_tris_probe<MODE>(b, q, qb, acc), tr_tris_live(q), stack, stack_entries, TR_TRIS_STACK, lost);
}
