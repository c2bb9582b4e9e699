// tr_nearest.h -- closest_point (include/triro_nearest.h): the nearest triangle of a mesh to a point.  Host + device, as
// tr_math.h: k_closest_point (nearest.hip) instantiates the walk per lane, tests/host_sim/nearest_sim.cpp compiles the
// very same functions with g++.  Not a CPU fallback: nothing in the C ABI reaches the host instantiation.
//
// THE CONTRACT.  Query point p (three float32), mesh of F triangles (float32 vertices, original face index).
//
//  * d2(p, T), the squared distance to ONE triangle, is evaluated in float64 from the float32 inputs by one fixed
//    sequence of + - * /, explicit fma, compares and selects (-ffp-contract=off holds): tr_near_tri.  Its form is the
//    minimum over four CANDIDATE POINTS, taken in this order with a strict `<`:
//      face : with e0 = b - a, e1 = c - b, e2 = a - c and n = e0 x e1: taken only where it exists (n.n > 0) and falls
//             inside (the edge functions ((e0 x (p - a)) . n, (e1 x (p - b)) . n, (e2 x (p - c)) . n are all >= 0;
//             the component of p along n drops out of them): q = p - ((p - a) . n / n.n) n;
//      edges: ab, bc, ca as segments: q = v + t e with t = clamp(((p - v) . e) / (e . e), 0, 1), and t = 0 for a
//             zero-length edge (the segment is its first vertex).
//    Every candidate q is then CLAMPED, per axis, into the coordinate range of the triangle's three vertices, and its
//    squared distance is tr_near_len2(p - q) = fma(dz, dz, fma(dy, dy, dx * dx)) of the rounded differences.
//  * Robustness.  A triangle whose vertices are collinear or coincident has n = 0 exactly or a face candidate that
//    the edges beat or match: it is the segment or the point it degenerates to.  Differences of float32 values are at
//    most 6.9e38, their products at most 1e78, n.n and the edge functions at most 1e157: nothing overflows float64;
//    a non-zero n.n of float32 inputs is at least 2^-596 and the divisors are tested > 0: no division by zero, no
//    Inf - Inf, no 0 * Inf.  Finite inputs never give NaN.
//  * The winner is the triangle that minimises (d2, original face index) lexicographically: on exactly equal float64
//    d2 the smaller face index wins.  A pure function of (p, the set of triangles): independent of traversal order,
//    launch shape and stack capacity, and bit-comparable with a brute force over tr_near_tri.
//  * Outputs: closest = the winning triangle's candidate point, each float64 component rounded to float32 (it stays
//    inside the triangle's coordinate range: the clamp); distance = (float)sqrt(d2), the square root in float64, +Inf
//    where it exceeds the float range (tr_near_distance); tri = the original face index.
//  * INACTIVE TRIANGLES.  A triangle with a NaN or an infinite coordinate (tr_near_active is false) offers no candidate: it
//    is not part of "the set of triangles" above, exactly as no ray hits it (arithmetic contract, "Meshes").
//    Without this a triangle with ONE infinite vertex still has finite edges and wins with a finite distance.  The
//    hierarchy keeps such triangles as leaves; their boxes may hold NaN or Inf, which the bound below turns into 0 or into
//    a bound that no finite best exceeds wrongly (a NaN difference selects 0, the smallest bound there is).
//  * A point with a non-finite component, a mesh of zero triangles, or a mesh whose triangles are all inactive: tri = -1,
//    distance = +Inf, closest = NaN.
//
// THE BOUND (culling).  A subtree is skipped only when tr_near_box(p, its box) > best d2 so far, STRICTLY: a tie is
// never culled.  tr_near_box is, per axis, g_k = max(fl(lo_k - p_k), fl(p_k - hi_k), 0) in float64, and
// tr_near_len2(g) -- the same last step as a candidate's distance.  MARGIN: NONE IS NEEDED, by monotonicity of rounding:
//    every candidate q of a triangle in the box has q_k in [min vertex_k, max vertex_k] (the clamp), inside [lo_k, hi_k]
//    (a node's box contains its triangles' vertices; the leaf box in a parent is the PADDED triangle box tr_tri_box, a
//    superset).  So in real numbers |p_k - q_k| >= max(lo_k - p_k, p_k - hi_k, 0); rounding to nearest is monotone and
//    odd, so the same holds for the rounded differences: |fl(p_k - q_k)| >= g_k, exactly.  tr_near_len2 is a chain of
//    one rounded product and two rounded fma, each monotone in every (non-negative) argument, so
//    tr_near_len2(p - q) >= tr_near_len2(g) in the computed float64 values.  The bound is a lower bound OF THE COMPUTED
//    d2 of every triangle below, not merely of the exact one: culling on `>` can lose neither the winner nor a tie.
//    In float64 the bound cannot overflow (points at 3e38 included).
// The far-child stack keeps an entry's bound as a float32 rounded DOWN (tr_near_floor32: never above the float64
// value, the largest finite float where that overflows), still a lower bound; the entry is dropped at the pop, without
// loading its node, when that float32 is beyond the best.
//
// THE WALK.  First the seed descent (tr_near_seed): from the root to the nearer child at every level, down to one leaf,
// so that the best is finite before anything is pushed.  Then tr_near_visit, one node per call, from the root: both
// child boxes of the node are bounded; leaves among the children are evaluated at once, the nearer first; of the internal children that survive the (updated) best, the nearer is
// visited next and the farther is pushed on the per-lane stack as {node, bound}.  With no child left the stack is
// popped.  The stack holds `stack_entries` entries (1 .. TR_NEAR_STACK); a push that does not fit is dropped and sets
// the sticky `lost` bit of st.sp.  A walk that ends with `lost` set is followed by tr_rewalk on a tr_near_probe: the whole tree again
// without a stack, children in fixed order, up through the parent links (tr_link), culling against the best already
// found -- near-optimal, so this second walk is short.  The winner is a lexicographic minimum over candidates: the
// second walk yields the same bits.  Cold, correct, not fast.  The builder guarantees a depth of at most 64; nothing
// here depends on the depth.  Below two triangles there is no hierarchy: the one triangle is evaluated directly.
#pragma once
#include "tr_walk.h"

#define TR_NEAR_STACK 32      // entries of {node, bound} per lane: 32 x 8 B x 128 lanes = 32 KB of LDS per workgroup; no walk of a hierarchy of up to 32 levels overflows it (tr_near_seed)

struct tr_near_pt { double d2, x, y, z; };      // a candidate point and its squared distance
struct tr_near_best {
    double d2;
    int32_t face;    // original face index of the best triangle so far (0x7fffffff: none)
    int32_t slot;    // its slot in `tris` (-1: none)
};
struct tr_near_state {
    int32_t node;    // next internal node to visit, -1 = nothing left
    uint32_t sp;     // 2 * entries in use | lost
};

TR_HD double tr_near_dot(double ax, double ay, double az, double bx, double by, double bz) { return fma(az, bz, fma(ay, by, ax * bx)); }
// the one squared length of candidates AND box bounds: monotone in |x|, |y|, |z| (see THE BOUND)
TR_HD double tr_near_len2(double x, double y, double z) { return fma(z, z, fma(y, y, x * x)); }
TR_HD double tr_near_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// candidate q (already computed) of the triangle with coordinate range [lo, hi]: clamp, measure, keep if strictly nearer
TR_HD void tr_near_take(tr_near_pt& best, bool exists, double px, double py, double pz, double qx, double qy, double qz,
                        const double* lo, const double* hi) {
    qx = tr_near_clamp(qx, lo[0], hi[0]); qy = tr_near_clamp(qy, lo[1], hi[1]); qz = tr_near_clamp(qz, lo[2], hi[2]);
    const double d2 = tr_near_len2(px - qx, py - qy, pz - qz);
    const bool lt = exists && d2 < best.d2;
    best.d2 = lt ? d2 : best.d2; best.x = lt ? qx : best.x; best.y = lt ? qy : best.y; best.z = lt ? qz : best.z;
}
// the segment v + t e, t in [0, 1], w = p - v
TR_HD void tr_near_edge(tr_near_pt& best, double px, double py, double pz, double vx, double vy, double vz, double ex, double ey,
                        double ez, double wx, double wy, double wz, const double* lo, const double* hi) {
    const double ee = tr_near_len2(ex, ey, ez);
    const double we = tr_near_dot(wx, wy, wz, ex, ey, ez);
    double t = ee > 0.0 ? we / (ee > 0.0 ? ee : 1.0) : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    tr_near_take(best, true, px, py, pz, fma(t, ex, vx), fma(t, ey, vy), fma(t, ez, vz), lo, hi);
}
// d2(p, T) and the closest point of T (see THE CONTRACT)
TR_HD tr_near_pt tr_near_tri(float pxf, float pyf, float pzf, float axf, float ayf, float azf, float bxf, float byf, float bzf,
                             float cxf, float cyf, float czf) {
    const double px = pxf, py = pyf, pz = pzf;
    const double ax = axf, ay = ayf, az = azf, bx = bxf, by = byf, bz = bzf, cx = cxf, cy = cyf, cz = czf;
    const double lo[3] = {(double)fminf(fminf(axf, bxf), cxf), (double)fminf(fminf(ayf, byf), cyf), (double)fminf(fminf(azf, bzf), czf)};
    const double hi[3] = {(double)fmaxf(fmaxf(axf, bxf), cxf), (double)fmaxf(fmaxf(ayf, byf), cyf), (double)fmaxf(fmaxf(azf, bzf), czf)};
    const double e0x = bx - ax, e0y = by - ay, e0z = bz - az;
    const double e1x = cx - bx, e1y = cy - by, e1z = cz - bz;
    const double e2x = ax - cx, e2y = ay - cy, e2z = az - cz;
    const double wax = px - ax, way = py - ay, waz = pz - az;
    const double wbx = px - bx, wby = py - by, wbz = pz - bz;
    const double wcx = px - cx, wcy = py - cy, wcz = pz - cz;
    tr_near_pt best;
    best.d2 = INFINITY; best.x = ax; best.y = ay; best.z = az;
    {   // the in-plane projection, where it exists and falls inside
        const double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
        const double nn = tr_near_len2(nx, ny, nz);
        const double u = tr_near_dot(e0y * waz - e0z * way, e0z * wax - e0x * waz, e0x * way - e0y * wax, nx, ny, nz);
        const double v = tr_near_dot(e1y * wbz - e1z * wby, e1z * wbx - e1x * wbz, e1x * wby - e1y * wbx, nx, ny, nz);
        const double w = tr_near_dot(e2y * wcz - e2z * wcy, e2z * wcx - e2x * wcz, e2x * wcy - e2y * wcx, nx, ny, nz);
        const bool exists = nn > 0.0 && u >= 0.0 && v >= 0.0 && w >= 0.0;
        const double s = tr_near_dot(wax, way, waz, nx, ny, nz) / (nn > 0.0 ? nn : 1.0);
        tr_near_take(best, exists, px, py, pz, fma(-s, nx, px), fma(-s, ny, py), fma(-s, nz, pz), lo, hi);
    }
    tr_near_edge(best, px, py, pz, ax, ay, az, e0x, e0y, e0z, wax, way, waz, lo, hi);
    tr_near_edge(best, px, py, pz, bx, by, bz, e1x, e1y, e1z, wbx, wby, wbz, lo, hi);
    tr_near_edge(best, px, py, pz, cx, cy, cz, e2x, e2y, e2z, wcx, wcy, wcz, lo, hi);
    return best;
}

// lower bound of the COMPUTED d2 of every triangle whose vertices lie in the box (see THE BOUND; no margin needed)
TR_HD double tr_near_box(double px, double py, double pz, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    const double ax = (double)lox - px, bx = px - (double)hix;
    const double ay = (double)loy - py, by = py - (double)hiy;
    const double az = (double)loz - pz, bz = pz - (double)hiz;
    const double mx = ax > bx ? ax : bx, my = ay > by ? ay : by, mz = az > bz ? az : bz;
    return tr_near_len2(mx > 0.0 ? mx : 0.0, my > 0.0 ? my : 0.0, mz > 0.0 ? mz : 0.0);
}
// the largest float32 that is not above x (x >= 0, finite): the bound as the stack keeps it
TR_HD float tr_near_floor32(double x) {
    const float f = (float)x;
    return (double)f > x ? tr_u2f(tr_f2u(f) - 1u) : f;      // (f > x >= 0: f is positive, Inf included -> the largest finite float)
}
// (float)sqrt(d2), +Inf beyond the float range: 2^128 - 2^103 is the midpoint between FLT_MAX and 2^128, which rounds away
TR_HD float tr_near_distance(double d2) {
    const double s = sqrt(d2);
    return s >= 3.4028235677973366e38 ? INFINITY : (float)s;
}

TR_HD void tr_near_init(tr_near_best& best) { best.d2 = INFINITY; best.face = 0x7fffffff; best.slot = -1; }
TR_HD bool tr_near_lost(uint32_t sp) { return (sp & 1u) != 0; }

// all nine coordinates finite (see INACTIVE TRIANGLES)
TR_HD bool tr_near_active(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    return tr_finite(ax) && tr_finite(ay) && tr_finite(az) && tr_finite(bx) && tr_finite(by) && tr_finite(bz) && tr_finite(cx) &&
           tr_finite(cy) && tr_finite(cz);
}

// one triangle against the best so far: (d2, face) lexicographic; an inactive triangle changes nothing (a select, not a
// branch: the arithmetic on its NaN / Inf is harmless and the control flow stays that of the finite case)
TR_HD void tr_near_leaf(const tr_bvh_view& b, int32_t slot, float px, float py, float pz, tr_near_best& best) {
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    const tr_near_pt c = tr_near_tri(px, py, pz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
    const bool active = tr_near_active(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
    if (active && (c.d2 < best.d2 || (c.d2 == best.d2 && t.face < best.face))) { best.d2 = c.d2; best.face = t.face; best.slot = slot; }
}

// both child boxes and child ids of an internal node
struct tr_near_node { double lb0, lb1; int32_t c0, c1; };
TR_HD tr_near_node tr_near_load(const tr_bvh_view& b, int32_t node, float px, float py, float pz) {
    const tr_f4* q = reinterpret_cast<const tr_f4*>(b.nodes + node);
    const tr_f4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];      // lo.x lo.y lo.z hi.z | hi.x hi.y lo.x lo.y | lo.z hi.z hi.x hi.y | c0 c1 ..
    tr_near_node r;
    r.lb0 = tr_near_box(px, py, pz, n0.x, n0.y, n0.z, n1.x, n1.y, n0.w);
    r.lb1 = tr_near_box(px, py, pz, n1.z, n1.w, n2.x, n2.z, n2.w, n2.y);
    r.c0 = (int32_t)tr_f2u(n3.x); r.c1 = (int32_t)tr_f2u(n3.y);
    return r;
}

// Far-child stack: entry e of a lane is the words 2 e (node) and 2 e + 1 (bound, float32 bits) of its column of a tr_ring
// (LDS on the device: stride = block size, explicit address_space(3) accesses through tr_ring_get / tr_ring_put).
// cap2 = 2 * entries the walk may use.
TR_HD void tr_near_push(const tr_ring stack, uint32_t cap2, uint32_t& sp, int32_t node, double lb) {
    const uint32_t w = sp & ~1u;
    if (w < cap2) {
        tr_ring_put(stack, w, node);
        tr_ring_put(stack, w + 1u, (int32_t)tr_f2u(tr_near_floor32(lb)));
        sp += 2u;
    } else {
        sp |= 1u;
    }
}
// the next entry whose bound is not beyond the best; -1: the stack is empty
TR_HD int32_t tr_near_pop(const tr_ring stack, uint32_t& sp, double best_d2) {
    while (sp >= 2u) {
        sp -= 2u;
        const uint32_t w = sp & ~1u;
        const float lb = tr_u2f((uint32_t)tr_ring_get(stack, w + 1u));
        if (!((double)lb > best_d2)) return tr_ring_get(stack, w);
    }
    return -1;
}

// visit st.node (>= 0): see THE WALK
TR_HD void tr_near_visit(const tr_bvh_view& b, float px, float py, float pz, tr_near_state& st, tr_near_best& best,
                         const tr_ring stack, uint32_t cap2) {
    const tr_near_node n = tr_near_load(b, st.node, px, py, pz);
    const bool swap = n.lb1 < n.lb0;
    const int32_t cn = swap ? n.c1 : n.c0, cf = swap ? n.c0 : n.c1;
    const double ln = swap ? n.lb1 : n.lb0, lf = swap ? n.lb0 : n.lb1;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? cf : cn;
        const double lb = k ? lf : ln;
        if (c < 0 && !(lb > best.d2)) tr_near_leaf(b, ~c, px, py, pz, best);
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

// The seed descent, one node per call: from `node` to its nearer child, without a stack and without culling, down to one
// leaf, which is evaluated.  Returns the next node, -1 after the leaf.  It gives the walk a finite best before its first
// push (unless that leaf is inactive: the walk then starts as if there were no seed, correct and only slower): without it the first descent of the walk culls nothing and pushes a far child at EVERY level -- a stack as deep as
// the hierarchy.  Measured on the host (20 000 hash points in 1.2x the box of an 81 920-triangle displaced icosphere, 23
// levels): without the seed 68 % of the walks need more than 16 entries, with it 6 %; the median need is 11-12 entries, the
// largest 21 -- points deep inside a near-sphere are nearly equidistant from much of the surface and keep a far child
// at most levels.  Hence TR_NEAR_STACK = 32: a walk pushes at most one entry per level.  The leaf the seed finds is one more candidate of the lexicographic minimum (the walk
// meets it again): results do not change.
TR_HD int32_t tr_near_seed(const tr_bvh_view& b, int32_t node, float px, float py, float pz, tr_near_best& best) {
    const tr_near_node n = tr_near_load(b, node, px, py, pz);
    const int32_t c = n.lb1 < n.lb0 ? n.c1 : n.c0;
    if (c >= 0) return c;
    tr_near_leaf(b, ~c, px, py, pz, best);
    return -1;
}

// the whole tree again without a stack (after a lost push): tr_rewalk(b, tr_near_probe{b, px, py, pz, best}) -- never done
// early, a child is culled against the best so far
struct tr_near_probe {
    const tr_bvh_view& b;
    float px, py, pz;
    tr_near_best& best;
    TR_HDM bool done() const { return false; }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_near_node n = tr_near_load(b, node, px, py, pz);
        c = phase ? n.c1 : n.c0;
        return !((phase ? n.lb1 : n.lb0) > best.d2);
    }
    TR_HDM void leaf(int32_t slot) const { tr_near_leaf(b, slot, px, py, pz, best); }
};

// the three outputs of a point from the best triangle (valid = finite point; best.slot < 0: no triangle).  Any of the
// pointers may be null.
TR_HD void tr_near_outputs(const tr_bvh_view& b, float px, float py, float pz, bool valid, const tr_near_best& best,
                           float* closest3, float* distance, int32_t* tri) {
    float qx = tr_u2f(0x7fc00000u), qy = qx, qz = qx, d = INFINITY;
    int32_t face = -1;
    if (valid && best.slot >= 0) {
        tr_counters* nc = nullptr;
        const tr_tri t = tr_load_tri<false, false>(b, best.slot, nc);
        const tr_near_pt c = tr_near_tri(px, py, pz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
        qx = (float)c.x; qy = (float)c.y; qz = (float)c.z;
        d = tr_near_distance(c.d2);
        face = t.face;
    }
    if (closest3) { closest3[0] = qx; closest3[1] = qy; closest3[2] = qz; }
    if (distance) *distance = d;
    if (tri) *tri = face;
}

TR_HD bool tr_near_valid(float px, float py, float pz) { return tr_finite(px) && tr_finite(py) && tr_finite(pz); }

// one point, start to end, on one lane (the host simulation; the kernel runs the first walk as a wave loop).
// stack_entries: 1 .. TR_NEAR_STACK, 0 = all of them.
TR_HD void tr_near_query(const tr_bvh_view& b, float px, float py, float pz, const tr_ring stack, int stack_entries,
                         float* closest3, float* distance, int32_t* tri) {
    const bool valid = tr_near_valid(px, py, pz) && b.num_tris > 0;
    tr_near_best best;
    tr_near_init(best);
    if (valid && b.num_tris >= 2) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
        tr_near_state st;
        for (int32_t node = 0; node >= 0;) node = tr_near_seed(b, node, px, py, pz, best);
        st.node = 0; st.sp = 0;
        while (st.node >= 0) tr_near_visit(b, px, py, pz, st, best, stack, cap2);
        if (tr_near_lost(st.sp)) tr_rewalk(b, tr_near_probe{b, px, py, pz, best});
    } else if (valid) {
        tr_near_leaf(b, 0, px, py, pz, best);      // no hierarchy below two triangles
    }
    tr_near_outputs(b, px, py, pz, valid, best, closest3, distance, tri);
}
