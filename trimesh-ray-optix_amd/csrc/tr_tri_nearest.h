// tr_tri_nearest.h -- triangles_nearest (include/triro_tri_nearest.h): the nearest face of a mesh to a TRIANGLE, the distance
// query of mesh against mesh.  Host + device, as tr_nearest.h and tr_tris.h, whose per-triangle distance function
// (tr_near_tri), squared length (tr_near_len2), activity rule (tr_near_active), far-child stack (tr_near_push / tr_near_pop /
// tr_near_floor32), radius rule (tr_within_valid / tr_within_r2) and overlap predicate (tr_tris_meets) it uses UNCHANGED:
// k_triangles_nearest (tri_nearest.hip) instantiates the walk per lane, tests/host_sim/tri_nearest_sim.cpp compiles the very
// same functions with g++.  Not a CPU fallback: nothing in the C ABI reaches the host instantiation.
//
// THE CONTRACT.  Query: a triangle Q = (p, q, r) of nine float32, optionally a bound max_distance (float32, per query or one
// for all); the mesh of the handle, F triangles T = (a, b, c) of float32 vertices with an original face index.
//
//  * The query is VALID iff all nine values are finite (tr_tris_valid) and the bound is a valid radius (tr_within_valid's
//    rule: r >= 0; -0.0 and +Inf are valid, +Inf means unbounded; NaN and negative ones are not).
//  * A mesh face with a non-finite coordinate is INACTIVE (tr_near_active, as everywhere): it offers no candidate and is
//    never returned.
//  * d2(Q, T), the squared distance of ONE pair, is evaluated in float64 from the float32 inputs by ONE FIXED SEQUENCE of
//    + - * /, explicit fma, compares and selects (-ffp-contract=off holds): tr_tn_pair.  It is the minimum, taken in this
//    order with a strict `<`, over FIFTEEN CANDIDATE PAIRS (x on Q, y on T):
//      vertices: p, q, r against T, then a, b, c against Q, each through tr_near_tri: the vertex is one point of the pair,
//                tr_near_tri's closest point the other.  A degenerate triangle, on either side, is thereby the segment or the
//                point it degenerates to, exactly as in closest_point.
//      edges   : pq, qr, rp of Q (outer loop) against ab, bc, ca of T (inner loop) as segments v + s e and w + t f, in the
//                textbook clamped form: A = e.e, C = f.f (tr_near_len2), B = e.f, D = e.r, G = f.r with r = v - w
//                (tr_near_dot), det = A C - B B; s = clamp((B G - C D) / det, 0, 1) where det > 0, else 0;
//                t = (B s + G) / C where C > 0, else 0; where t < 0: t = 0 and s = clamp(-D / A, 0, 1); where t > 1: t = 1 and
//                s = clamp((B - D) / A, 0, 1), both 0 unless A > 0; x = fma(s, e, v), y = fma(t, f, w).
//    Every candidate's x is then CLAMPED, per axis, into the coordinate range of Q's three vertices and y into that of T's, and
//    the squared distance is tr_near_len2(x - y) of the rounded differences.
//  * NEAR-PARALLEL EDGES make s ill-conditioned (det is a difference of nearly equal products).  That does not hurt the
//    minimum: both points still lie on their segments (s and t are clamped to [0, 1] whatever det gave), so the candidate never
//    undercuts the true distance by more than rounding; and the true minimum of a parallel pair of segments is attained at an
//    end of one of them, which the six vertex candidates already cover.  The same holds for a zero-length edge (A = 0 or
//    C = 0: the guarded divisions give 0, the pair is the edge's first vertex and a point of the other edge).
//  * THE MEETING RULE.  Where both triangles have area and tr_tris_meets(T, Q) holds (tr_tris.h: the closed triangles share a
//    point), d2 = 0 EXACTLY: the fifteen candidates of a pair whose interiors cross measure boundary features and are not 0.
//    The witness points of such a pair stay those of the minimal candidate: finite points on the two triangles, THE NEAREST
//    BOUNDARY FEATURES, NOT A COMMON POINT.  The seventeen axes are evaluated only where step 1 of the predicate (the exact
//    float32 box test) does not already separate the pair.
//  * THE DEGENERATE CAVEAT, DELIBERATE.  A triangle without area (tr_tris.h, DEGENERATE TRIANGLES) meets nothing, so a
//    segment or a point that pierces the interior of the other triangle is NOT seen as meeting: its distance is that of the
//    nearest boundary features (the end points against the face, the segment against the three edges), which is positive when
//    it crosses the interior away from the boundary.  This is tr_tris.h's rule carried over, and the reason why there is no
//    segments_nearest on this query.
//  * OVERFLOW.  The bounds of tr_nearest.h and tr_tris.h hold: a difference of float32 values is at most 6.9e38, so A, C, |B|,
//    |D|, |G| <= 3 * (6.9e38)^2 < 1.5e78, the products A C, B B, B G, C D < 2.3e156 and their differences < 5e156, far below
//    DBL_MAX.  A non-zero A or C is at least 2^-298 (the smallest non-zero difference is 2^-149) and every divisor is tested
//    > 0: no division by zero.  A quotient may overflow to +-Inf (a tiny det); the clamp to [0, 1] is two compares and turns it
//    into 0 or 1.  No Inf - Inf, no 0 * Inf (s and t are in [0, 1] before they multiply anything): finite inputs never give
//    NaN, and every candidate is a pair of finite points.
//  * THE WINNER minimises (d2, original face index) lexicographically among the active faces with d2 <= R2 =
//    tr_within_r2(max_distance) (not strict: a face at exactly the bound is admitted; R2 = +Inf admits every active face).
//    A pure function of (Q, max_distance, the set of triangles): independent of traversal order, stack capacity and launch
//    shape, and bit-comparable with a brute force over tr_tn_pair.
//  * OUTPUTS per query: tri = the winner's original face index (int32); distance = tr_near_distance(d2) (float32);
//    closest_mesh = y and closest_query = x of the winning pair's minimal candidate, each float64 component rounded to
//    float32 (they stay inside the coordinate ranges: the clamp).  All but tri are optional.
//  * NO RESULT: an invalid query, a mesh of zero triangles or one without an active face, or no face within the bound:
//    tri = -1, distance = +Inf, both points NaN.  Every element of every output is written.
//
// THE BOUND (culling).  A subtree is skipped only when tr_tn_box(Q's box, its box) > best d2 so far, STRICTLY: a tie is never
// culled.  [qlo, qhi] is the exact float32 box of Q (tr_tris_box, once per query); per axis
//    g_k = max(fl(lo_k - qhi_k), fl(qlo_k - hi_k), 0) in float64, and the bound is tr_near_len2(g).
// MARGIN: NONE IS NEEDED.  It is tr_nearest.h's argument applied to two boxes:
//    1. every candidate has x_k in [qlo_k, qhi_k] and y_k in [min vertex_k, max vertex_k] of T (the clamps), which lies inside
//       [lo_k, hi_k] of every node above T (a node's box contains its triangles' vertices; the leaf box in a parent is the
//       padded triangle box, a superset).  So in real numbers y_k - x_k >= lo_k - qhi_k and x_k - y_k >= qlo_k - hi_k, hence
//       |x_k - y_k| >= max(lo_k - qhi_k, qlo_k - hi_k, 0).
//    2. rounding to nearest is monotone and odd, so the same holds for the rounded differences: |fl(x_k - y_k)| >= g_k.
//    3. tr_near_len2 is one rounded product and two rounded fma, each monotone in every (non-negative) argument, so
//       tr_near_len2(x - y) >= tr_near_len2(g) in the computed float64 values.
//    The bound is a lower bound OF THE COMPUTED d2 of every candidate of every face below, and 0 <= it bounds the d2 = 0 of
//    the meeting rule as well: a pair that meets has overlapping boxes (step 1 of the predicate does not separate it), every
//    g_k is 0 and so is the bound.  Culling on `>` loses neither the winner nor a tie.  A NaN in a node box compares false
//    and selects 0, the smallest bound there is.  In float64 the bound cannot overflow.
// A leaf is first bounded against the face's OWN exact box (min / max of its vertices, the same argument): a face whose bound
// exceeds the best, or equals it while its index is above the best's, cannot win and is not evaluated.
// The far-child stack keeps an entry's bound as a float32 rounded DOWN (tr_near_floor32), still a lower bound.
//
// THE WALK is tr_nearest.h's with this load, leaf and visit: the seed descent (tr_tn_seed) to one leaf, then tr_tn_visit from
// the root, nearer child first, the farther pushed as {node, bound} on the per-lane stack of TR_NEAR_STACK entries; a lost
// push sets the sticky bit and tr_rewalk on a tr_tn_probe follows.  The bound of a query starts the best at {R2, INT_MAX, -1}
// (tr_within_closest_init), which for R2 = +Inf is tr_near_init.  Below two triangles there is no hierarchy.
//
// REGISTERS.  As tr_tris_sat: one frame, one candidate at a time.  The six vertex candidates are two rolled loops, each around
// one tr_near_tri, the nine edge pairs a rolled 3 x 3 loop; each candidate is tested before the next is formed.  The walk needs only d2 (tr_tn_d2: the predicate first, the candidates where it fails); the
// witness points are formed once, for the winner (tr_tn_outputs).
#pragma once
#include "tr_tris.h"

// REGISTERS, continued: tr_tn_fresh.  The compiler hoists whatever depends on the query alone -- the float64 edges and normal of Q
// in the predicate, Q's side of tr_near_tri, the float64 corners of its box -- in front of the WALK, and whatever depends on
// one triangle alone in front of the rolled loop over the other's vertices, and keeps all of it in registers across them: 254
// VGPRs instead of 168.  tr_tn_fresh passes values through an empty statement that the compiler must take to change them, in
// place (no copy: the value before is dead), so that what is derived from them is derived where it is used, per leaf and per
// candidate, as written.  The values do not change; on the host it is nothing.
#if defined(__HIP_DEVICE_COMPILE__)
#define TR_TN_FRESH(x) asm volatile("" : "+v"(x))
#else
#define TR_TN_FRESH(x) ((void)0)
#endif
TR_HD void tr_tn_fresh(float& a, float& b, float& c) { TR_TN_FRESH(a); TR_TN_FRESH(b); TR_TN_FRESH(c); }
TR_HD void tr_tn_fresh(tr_tris_q& q) { tr_tn_fresh(q.px, q.py, q.pz); tr_tn_fresh(q.qx, q.qy, q.qz); tr_tn_fresh(q.rx, q.ry, q.rz); }
TR_HD void tr_tn_fresh(tr_box& b) { tr_tn_fresh(b.lox, b.loy, b.loz); tr_tn_fresh(b.hix, b.hiy, b.hiz); }

struct tr_tn_pt { double d2, xx, xy, xz, yx, yy, yz; };      // a candidate pair: x on Q, y on T, and its squared distance

TR_HD float tr_tn_pick(int k, float v0, float v1, float v2) { return k == 0 ? v0 : (k == 1 ? v1 : v2); }
TR_HD double tr_tn_unit(double t) { return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t); }

// candidate (x, y): clamp x into Q's coordinate range and y into T's, measure, keep if strictly nearer
TR_HD void tr_tn_take(tr_tn_pt& best, double xx, double xy, double xz, double yx, double yy, double yz, const tr_box& qb, const tr_box& tb) {
    xx = tr_near_clamp(xx, (double)qb.lox, (double)qb.hix); xy = tr_near_clamp(xy, (double)qb.loy, (double)qb.hiy);
    xz = tr_near_clamp(xz, (double)qb.loz, (double)qb.hiz);
    yx = tr_near_clamp(yx, (double)tb.lox, (double)tb.hix); yy = tr_near_clamp(yy, (double)tb.loy, (double)tb.hiy);
    yz = tr_near_clamp(yz, (double)tb.loz, (double)tb.hiz);
    const double d2 = tr_near_len2(xx - yx, xy - yy, xz - yz);
    if (d2 < best.d2) { best.d2 = d2; best.xx = xx; best.xy = xy; best.xz = xz; best.yx = yx; best.yy = yy; best.yz = yz; }
}

// the exact float32 box of a face: its coordinate range
TR_HD tr_box tr_tn_face_box(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    tr_box b;
    b.lox = fminf(fminf(ax, bx), cx); b.loy = fminf(fminf(ay, by), cy); b.loz = fminf(fminf(az, bz), cz);
    b.hix = fmaxf(fmaxf(ax, bx), cx); b.hiy = fmaxf(fmaxf(ay, by), cy); b.hiz = fmaxf(fmaxf(az, bz), cz);
    return b;
}

// the minimum over the fifteen candidate pairs of Q and T = (a, b, c), finite coordinates (see THE CONTRACT); qb = tr_tris_box(q).
// (q and the vertices come by reference and by value only to pass through tr_tn_fresh: they leave as they came)
TR_HD tr_tn_pt tr_tn_candidates(tr_tris_q& q, const tr_box& qb, float ax, float ay, float az, float bx, float by, float bz, float cx,
                                float cy, float cz) {
    tr_tn_pt best;
    best.d2 = INFINITY; best.xx = q.px; best.xy = q.py; best.xz = q.pz; best.yx = ax; best.yy = ay; best.yz = az;
    // p, q, r against T, then a, b, c against Q.  tr_near_tri has clamped its point into the coordinate range of the triangle it
    // was given and measured it, and the vertex is in its own triangle's range as it is: the clamps of the contract change
    // nothing here, and tr_near_len2 of the negated differences is the same number
#pragma unroll 1
    for (int m = 0; m < 3; m++) {
        const float px = tr_tn_pick(m, q.px, q.qx, q.rx), py = tr_tn_pick(m, q.py, q.qy, q.ry), pz = tr_tn_pick(m, q.pz, q.qz, q.rz);
        tr_tn_fresh(ax, ay, az); tr_tn_fresh(bx, by, bz); tr_tn_fresh(cx, cy, cz);
        const tr_near_pt c = tr_near_tri(px, py, pz, ax, ay, az, bx, by, bz, cx, cy, cz);
        if (c.d2 < best.d2) { best.d2 = c.d2; best.xx = px; best.xy = py; best.xz = pz; best.yx = c.x; best.yy = c.y; best.yz = c.z; }
    }
#pragma unroll 1
    for (int m = 0; m < 3; m++) {
        const float px = tr_tn_pick(m, ax, bx, cx), py = tr_tn_pick(m, ay, by, cy), pz = tr_tn_pick(m, az, bz, cz);
        tr_tn_fresh(q);
        const tr_near_pt c = tr_near_tri(px, py, pz, q.px, q.py, q.pz, q.qx, q.qy, q.qz, q.rx, q.ry, q.rz);
        if (c.d2 < best.d2) { best.d2 = c.d2; best.xx = c.x; best.xy = c.y; best.xz = c.z; best.yx = px; best.yy = py; best.yz = pz; }
    }
    // pq, qr, rp against ab, bc, ca
    tr_tn_fresh(q);
    tr_tn_fresh(ax, ay, az); tr_tn_fresh(bx, by, bz); tr_tn_fresh(cx, cy, cz);
    const tr_box tb = tr_tn_face_box(ax, ay, az, bx, by, bz, cx, cy, cz);
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        const double vx = tr_tn_pick(i, q.px, q.qx, q.rx), vy = tr_tn_pick(i, q.py, q.qy, q.ry), vz = tr_tn_pick(i, q.pz, q.qz, q.rz);
        const double ex = (double)tr_tn_pick(i, q.qx, q.rx, q.px) - vx, ey = (double)tr_tn_pick(i, q.qy, q.ry, q.py) - vy,
                     ez = (double)tr_tn_pick(i, q.qz, q.rz, q.pz) - vz;
        const double A = tr_near_len2(ex, ey, ez);
#pragma unroll 1
        for (int j = 0; j < 3; j++) {
            const double wx = tr_tn_pick(j, ax, bx, cx), wy = tr_tn_pick(j, ay, by, cy), wz = tr_tn_pick(j, az, bz, cz);
            const double fx = (double)tr_tn_pick(j, bx, cx, ax) - wx, fy = (double)tr_tn_pick(j, by, cy, ay) - wy,
                         fz = (double)tr_tn_pick(j, bz, cz, az) - wz;
            const double rx = vx - wx, ry = vy - wy, rz = vz - wz;
            const double C = tr_near_len2(fx, fy, fz);
            const double B = tr_near_dot(ex, ey, ez, fx, fy, fz);
            const double D = tr_near_dot(ex, ey, ez, rx, ry, rz);
            const double G = tr_near_dot(fx, fy, fz, rx, ry, rz);
            const double det = A * C - B * B;
            double s = det > 0.0 ? tr_tn_unit((B * G - C * D) / (det > 0.0 ? det : 1.0)) : 0.0;
            double t = C > 0.0 ? (B * s + G) / (C > 0.0 ? C : 1.0) : 0.0;
            const double sa = A > 0.0 ? A : 1.0;
            if (t < 0.0) {
                t = 0.0;
                s = A > 0.0 ? tr_tn_unit(-D / sa) : 0.0;
            } else if (t > 1.0) {
                t = 1.0;
                s = A > 0.0 ? tr_tn_unit((B - D) / sa) : 0.0;
            }
            tr_tn_take(best, fma(s, ex, vx), fma(s, ey, vy), fma(s, ez, vz), fma(t, fx, wx), fma(t, fy, wy), fma(t, fz, wz), qb, tb);
        }
    }
    return best;
}

// d2(Q, T) with the witness points of the minimal candidate (see THE MEETING RULE); finite coordinates
TR_HD tr_tn_pt tr_tn_pair(tr_tris_q& q, const tr_box& qb, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                          float cz) {
    tr_tn_pt c = tr_tn_candidates(q, qb, ax, ay, az, bx, by, bz, cx, cy, cz);
    if (tr_tris_meets(q, qb, ax, ay, az, bx, by, bz, cx, cy, cz)) c.d2 = 0.0;
    return c;
}
// d2(Q, T) alone, as the walk needs it: the same value, the candidates only where the pair does not meet
TR_HD double tr_tn_d2(tr_tris_q& q, const tr_box& qb, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                      float cz) {
    if (tr_tris_meets(q, qb, ax, ay, az, bx, by, bz, cx, cy, cz)) return 0.0;
    tr_tn_fresh(q);
    tr_tn_fresh(ax, ay, az); tr_tn_fresh(bx, by, bz); tr_tn_fresh(cx, cy, cz);
    return tr_tn_candidates(q, qb, ax, ay, az, bx, by, bz, cx, cy, cz).d2;
}

// lower bound of the COMPUTED d2 of every face whose vertices lie in the box (see THE BOUND; no margin needed)
TR_HD double tr_tn_box(const tr_box& qb, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    const double ax = (double)lox - (double)qb.hix, bx = (double)qb.lox - (double)hix;
    const double ay = (double)loy - (double)qb.hiy, by = (double)qb.loy - (double)hiy;
    const double az = (double)loz - (double)qb.hiz, bz = (double)qb.loz - (double)hiz;
    const double mx = ax > bx ? ax : bx, my = ay > by ? ay : by, mz = az > bz ? az : bz;
    return tr_near_len2(mx > 0.0 ? mx : 0.0, my > 0.0 ? my : 0.0, mz > 0.0 ? mz : 0.0);
}

// the query of a lane: the triangle, its exact box, the squared bound (the walk takes it by reference for tr_tn_fresh alone)
struct tr_tn_query_t {
    tr_tris_q q;
    tr_box qb;
    double R2;
};
TR_HD bool tr_tn_valid(const tr_tris_q& q, float r) { return tr_tris_valid(q) && r >= 0.0f; }
TR_HD tr_tn_query_t tr_tn_make(const tr_tris_q& q, float r) {
    tr_tn_query_t Q;
    Q.q = q; Q.qb = tr_tris_box(q); Q.R2 = tr_within_r2(r);
    return Q;
}

// one face against the best so far: (d2, face) lexicographic.  An inactive face changes nothing; neither does one whose own
// box already puts it beyond the best (see THE BOUND)
TR_HD void tr_tn_leaf(const tr_bvh_view& b, int32_t slot, tr_tn_query_t& Q, tr_near_best& best) {
    tr_tn_fresh(Q.q); tr_tn_fresh(Q.qb);
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    if (!tr_near_active(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz)) return;
    const tr_box tb = tr_tn_face_box(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
    const double lb = tr_tn_box(Q.qb, tb.lox, tb.loy, tb.loz, tb.hix, tb.hiy, tb.hiz);
    if (lb > best.d2 || (lb == best.d2 && t.face > best.face)) return;
    const double d2 = tr_tn_d2(Q.q, Q.qb, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
    if (d2 < best.d2 || (d2 == best.d2 && t.face < best.face)) { best.d2 = d2; best.face = t.face; best.slot = slot; }
}

// both child boxes and child ids of an internal node (the layout: tr_near_load)
TR_HD tr_near_node tr_tn_load(const tr_bvh_view& b, int32_t node, tr_box& qb) {
    tr_tn_fresh(qb);
    const tr_f4* q = reinterpret_cast<const tr_f4*>(b.nodes + node);
    const tr_f4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];      // lo.x lo.y lo.z hi.z | hi.x hi.y lo.x lo.y | lo.z hi.z hi.x hi.y | c0 c1 ..
    tr_near_node r;
    r.lb0 = tr_tn_box(qb, n0.x, n0.y, n0.z, n1.x, n1.y, n0.w);
    r.lb1 = tr_tn_box(qb, n1.z, n1.w, n2.x, n2.z, n2.w, n2.y);
    r.c0 = (int32_t)tr_f2u(n3.x); r.c1 = (int32_t)tr_f2u(n3.y);
    return r;
}

// visit st.node (>= 0): tr_near_visit with this load and leaf
TR_HD void tr_tn_visit(const tr_bvh_view& b, tr_tn_query_t& Q, tr_near_state& st, tr_near_best& best, const tr_ring stack, uint32_t cap2) {
    const tr_near_node n = tr_tn_load(b, st.node, Q.qb);
    const bool swap = n.lb1 < n.lb0;
    const int32_t cn = swap ? n.c1 : n.c0, cf = swap ? n.c0 : n.c1;
    const double ln = swap ? n.lb1 : n.lb0, lf = swap ? n.lb0 : n.lb1;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? cf : cn;
        const double lb = k ? lf : ln;
        if (c < 0 && !(lb > best.d2)) tr_tn_leaf(b, ~c, Q, best);
    }
    const bool go_n = cn >= 0 && !(ln > best.d2), go_f = cf >= 0 && !(lf > best.d2);
    if (go_n) {
        if (go_f) tr_near_push(stack, cap2, st.sp, cf, lf);
        st.node = cn;
    } else if (go_f) {
        st.node = cf;
    } else {
        st.node = tr_near_pop(stack, st.sp, best.d2);
    }
}

// the seed descent, one node per call (tr_near_seed): to the nearer child, down to one leaf, which is evaluated
TR_HD int32_t tr_tn_seed(const tr_bvh_view& b, int32_t node, tr_tn_query_t& Q, tr_near_best& best) {
    const tr_near_node n = tr_tn_load(b, node, Q.qb);
    const int32_t c = n.lb1 < n.lb0 ? n.c1 : n.c0;
    if (c >= 0) return c;
    tr_tn_leaf(b, ~c, Q, best);
    return -1;
}

// the whole tree again without a stack (after a lost push): tr_rewalk(b, tr_tn_probe{b, Q, best})
struct tr_tn_probe {
    const tr_bvh_view& b;
    tr_tn_query_t& Q;
    tr_near_best& best;
    TR_HDM bool done() const { return false; }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_near_node n = tr_tn_load(b, node, Q.qb);
        c = phase ? n.c1 : n.c0;
        return !((phase ? n.lb1 : n.lb0) > best.d2);
    }
    TR_HDM void leaf(int32_t slot) const { tr_tn_leaf(b, slot, Q, best); }
};

// the four outputs of a query from the best face (best.slot < 0: none).  Any pointer but tri may be null.
TR_HD void tr_tn_outputs(const tr_bvh_view& b, tr_tn_query_t& Q, bool valid, const tr_near_best& best, int32_t* tri, float* distance,
                         float* closest_mesh3, float* closest_query3) {
    const float nan = tr_u2f(0x7fc00000u);
    float xx = nan, xy = nan, xz = nan, yx = nan, yy = nan, yz = nan, d = INFINITY;
    int32_t face = -1;
    if (valid && best.slot >= 0) {
        tr_counters* nc = nullptr;
        const tr_tri t = tr_load_tri<false, false>(b, best.slot, nc);
        const tr_tn_pt c = tr_tn_pair(Q.q, Q.qb, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
        xx = (float)c.xx; xy = (float)c.xy; xz = (float)c.xz; yx = (float)c.yx; yy = (float)c.yy; yz = (float)c.yz;
        d = tr_near_distance(c.d2);
        face = t.face;
    }
    *tri = face;
    if (distance) *distance = d;
    if (closest_mesh3) { closest_mesh3[0] = yx; closest_mesh3[1] = yy; closest_mesh3[2] = yz; }
    if (closest_query3) { closest_query3[0] = xx; closest_query3[1] = xy; closest_query3[2] = xz; }
}

// one query, start to end, on one lane (the host simulation; the kernel runs the first walk as a wave loop).
// stack_entries: 1 .. TR_NEAR_STACK, 0 = all of them; *lost (may be null): the first walk overflowed its stack
TR_HD void tr_tn_query(const tr_bvh_view& b, const tr_tris_q& q, float r, const tr_ring stack, int stack_entries, int32_t* tri,
                       float* distance, float* closest_mesh3, float* closest_query3, bool* lost) {
    const bool valid = tr_tn_valid(q, r) && b.num_tris > 0;
    tr_tn_query_t Q = tr_tn_make(q, r);
    tr_near_best best;
    tr_within_closest_init(best, Q.R2);
    if (lost) *lost = false;
    if (valid && b.num_tris >= 2) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
        tr_near_state st;
        for (int32_t node = 0; node >= 0;) node = tr_tn_seed(b, node, Q, best);
        st.node = 0; st.sp = 0;
        while (st.node >= 0) tr_tn_visit(b, Q, st, best, stack, cap2);
        if (lost) *lost = tr_near_lost(st.sp);
        if (tr_near_lost(st.sp)) tr_rewalk(b, tr_tn_probe{b, Q, best});
    } else if (valid) {
        tr_tn_leaf(b, 0, Q, best);      // no hierarchy below two triangles
    }
    tr_tn_outputs(b, Q, valid, best, tri, distance, closest_mesh3, closest_query3);
}
