// tr_planes.h -- plane queries (include/triro_planes.h): the faces of a mesh that a plane meets, and the segments in which it
// cuts them (the section of trimesh.intersections.mesh_plane / mesh_multiplane).  Host + device, as tr_boxes.h, whose row limit
// (tr_rows_limit) and activity rule (tr_near_active) it uses UNCHANGED: k_planes<>, k_planes_rows and k_planes_segments
// (planes.hip) run these functions per lane, tests/host_sim/planes_sim.cpp compiles the very same functions with g++ and drives
// them for a simulated wave of 64 lanes.  Not a CPU fallback: nothing in the C ABI reaches the host instantiation.
//
// THE CONTRACT.  Query: a plane through the origin o with the normal n, six float32; the mesh of the handle.  The normal is NOT
// normalised: only signs and ratios of s (below) are used.
//
//  * The query is VALID iff all six values are finite and n != (0, 0, 0) (-0 is 0).  Denormal normals are valid.
//  * A triangle with a non-finite coordinate is INACTIVE (tr_near_active, as everywhere) and is never met.
//  * THE SIGNED VALUE of a vertex v is ONE FIXED EXPRESSION in float64 from the float32 inputs (-ffp-contract=off holds, fma only
//    where written):   d_k = (double)v_k - (double)o_k,   s(v) = fma(n_z, d_z, fma(n_y, d_y, n_x * d_x))      (tr_plane_s).
//    With finite inputs |d| <= 6.9e38 and |s| <= about 1e78: nothing overflows and no NaN arises.
//  * With pos, neg, zero = the numbers of vertices of a face with s > 0, s < 0, s == 0:
//      a face MEETS the plane iff it is active and neither pos == 3 nor neg == 3 -- touching counts, a coplanar face meets;
//      a face is CUT iff it is active and pos >= 1 && (neg >= 1 || zero == 2) -- these faces own a row of the section.
//    The section of a plane is the boundary of the part of the surface STRICTLY on the positive side: a face that only touches
//    the plane from below owns nothing, a coplanar face owns nothing, a face that stands on the plane with one vertex owns
//    nothing, and an edge lying in the plane belongs to the face whose third vertex is positive.
//  * THE SEGMENT of a cut face.  Walk the vertices in winding order 0 -> 1 -> 2 -> 0; the positive vertices are one cyclic arc.
//    p0 is where the walk ENTERS the arc (from a vertex with s <= 0 to one with s > 0): that first vertex itself, its float32
//    coordinates exactly, when its s is 0, else the crossing point of that edge.  p1 is where the walk LEAVES the arc, by the
//    same rule on the leaving edge.  The direction p0 -> p1 of a row is (face normal) x (plane normal).
//    THE CROSSING POINT of an edge is ALWAYS computed from its negative vertex u to its positive vertex w, whichever face asks:
//        t = s(u) / (s(u) - s(w))  in float64,      p_k = (float)fma(t, (double)w_k - (double)u_k, (double)u_k)      (tr_plane_cross)
//    so both faces of a shared edge produce the same bits, and the p1 of one face IS the p0 of its neighbour: the rows of a
//    closed, consistently wound mesh close into loops bit for bit (the fill rule of the ray predicate carried over to sections).
//    0 <= t <= 1 UNDER ROUNDING: s(u) < 0 < s(w), so the exact difference s(u) - s(w) <= s(u) < 0, and rounding is monotone and
//    s(u) is representable: the computed denominator D satisfies D <= s(u) < 0 (and is finite, |D| <= 2e78).  The exact quotient
//    s(u) / D lies in (0, 1]; 0 and 1 are representable and rounding is monotone: 0 <= t <= 1 (t may underflow to 0).
//    p IS FINITE and lies in the closed interval of u_k and w_k: e = fl(w_k - u_k) is within 2^-53 relative of w_k - u_k, the exact
//    value u_k + t e lies between u_k and u_k + e, so the float64 result is within max(|u_k|, |w_k|) * 2^-51 of that interval; half a
//    float32 step at that magnitude is max(|u_k|, |w_k|) * 2^-25 or more, so the conversion lands on or between the two float32
//    numbers u_k and w_k -- never an overflow, +-FLT_MAX included.
//  * any = at least one face meets (is cut by) the plane (uint8); count = how many (int32); list = those faces by ORIGINAL FACE
//    INDEX, ASCENDING, at rows offsets[i] .. offsets[i] + count[i] (uncapped; int64 offsets from tr_hits_scan).  Each of the three
//    works for either predicate: the run-time argument `cut` (0 = MEET, 1 = CUT) selects it, wave-uniform.  With cut = 1 the fill
//    may also write segments float32 [rows, 2, 3] = (p0, p1) per row.  A row is a pure function of (plane, face).
//  * An invalid plane, a mesh of zero triangles or one without an active triangle: any = 0, count = 0, an empty list.  Every
//    element of every output is written.
//  * Results do not depend on walk order, frontier capacity or launch shape.
//
// CULLING.  s is MONOTONE in every vertex coordinate UNDER ITS OWN ROUNDING: fl is monotone, so d_k = fl(v_k - o_k) is
// non-decreasing in v_k; a rounded product n_k * d_k is monotone in d_k (non-decreasing for n_k >= 0, non-increasing otherwise); a
// rounded fma(n_k, d_k, acc) is non-decreasing in acc and monotone in d_k the same way.  s is a chain of these, so with the other
// two coordinates fixed s is non-decreasing in v_k where n_k >= 0 and non-increasing where n_k < 0.  For a node box [lo, hi] take
// the corner m_k = (n_k >= 0 ? lo_k : hi_k) and the opposite corner M: moving a vertex v of the box to m one coordinate at a time
// never raises s, moving it to M never lowers it: s(m) <= s(v) <= s(M) in COMPUTED values, with the same function.  Every vertex
// of every active triangle below a node lies in the node's box (the leaf box in a parent is the padded triangle box, a superset).
// A subtree is skipped iff s(m) > 0 || s(M) < 0, strictly (tr_plane_skip): then every vertex below has s > 0 (pos == 3 for every
// face) or s < 0 (neg == 3): no face below MEETS the plane, and a face that is CUT meets it.  No rounding margin is needed.  A box
// with an infinity keeps the inequalities (the chain is monotone on the extended reals) unless a NaN arises (0 * Inf, Inf - Inf,
// a NaN bound), and a NaN compares false and never culls.
//
// THE WALK (planes.hip: k_planes<>; planes_sim.cpp: the same loop for a simulated wave).  ONE WAVE PER PLANE: the typical call has
// few planes and large answers, one plane per lane would leave the GPU idle.  The wave owns a FRONTIER of node ids in LDS
// (TR_PLANES_FRONTIER entries), used from the top.  In a ROUND lane l takes entry top - 1 - l, for up to 64 entries
// (tr_planes_visit): it loads its 64-byte node and tests both child boxes.  A surviving leaf child is a CANDIDATE, a surviving
// internal child is PUSHED at top + its rank among the pushing lanes (a ballot prefix, tr_planes_rank): child 0 of every lane
// first, then child 1.  Candidates are evaluated in converged code (tr_planes_leaf) and recorded by ballot + lane rank at a
// wave-uniform cursor: one wave owns the plane, no atomic is needed, and FILL never writes at or beyond its limit.
// OVERFLOW.  A push whose position is at or beyond the capacity is not lost: its lane keeps the child as the root of a SUBTREE
// WALK (tr_planes_sub) and walks that subtree to the end without a stack, children in fixed order, up through the parent links,
// stopping when it is back at the subtree's root -- the tr_rewalk of tr_walk.h bounded to a subtree.  (Not folded into it: this
// one is RESUMABLE, one candidate per call with its state in the lane between calls, and stops at a root that is not the
// tree's; the shared loop would need a flag for each.)  A lane can overflow with both children
// of one round: the second waits in `next`.  The subtree walks run as a wave loop of their own (each lane advances to its next
// candidate, tr_planes_sub_next; the candidates are then recorded in converged code as above) and have priority: rounds resume
// when no lane has a subtree left, so a lane never holds more than the two roots of one round.  A node is entered from exactly
// one place -- the frontier or a subtree walk above it -- so nothing is visited twice, and nothing is discarded and redone.
// ANY ends the wave at the first hit, FILL when its rows are full.  Below two triangles there is no hierarchy: lane 0 takes the
// one triangle as its candidate.
//
// THE ORDERING (k_planes_rows, one workgroup per plane).  The rows of a plane leave the walk in walk order.  They are put into
// ascending face order in place by a sorting network whose compare-exchanges all point the same way: the bitonic form in which the
// first step of each merge of two runs of k pairs i with i ^ (2k - 1) (the mirror image in its block of 2k) and the later steps
// pair i with i ^ j, j = k/2 .. 1; the smaller key always goes to the smaller index.  On the array padded with +inf to a power of
// two a pair with an index >= m never exchanges (the larger index holds +inf and keeps it), so such pairs are simply SKIPPED: no
// scratch, no padding, and every index formed is below m whatever the rows hold (tr_planes_pair / tr_planes_cx).  The arena slot
// of a row rides beside its face through every exchange (in word 0 of the row's segment, which k_planes_segments overwrites).
// k_planes_segments then evaluates (p0, p1) per row, one lane per row, from (plane, slot): the plane of a row by binary search in
// offsets (tr_planes_owner), the slot clamped into the arena (rows the caller misdirected: wrong, never outside).
#pragma once
#include "tr_within.h"

#define TR_PLANES_FRONTIER 2048      // node ids per wave: 8 KB of LDS per wave
#define TR_PLANES_WAVE 64

enum tr_planes_mode { TR_PLANES_ANY = 0, TR_PLANES_COUNT = 1, TR_PLANES_FILL = 2 };

struct tr_plane { float ox, oy, oz, nx, ny, nz; };

TR_HD bool tr_plane_valid(const tr_plane& q) {
    return tr_finite(q.ox) && tr_finite(q.oy) && tr_finite(q.oz) && tr_finite(q.nx) && tr_finite(q.ny) && tr_finite(q.nz) &&
           !(q.nx == 0.0f && q.ny == 0.0f && q.nz == 0.0f);
}
// THE SIGNED VALUE of the point (x, y, z)
TR_HD double tr_plane_s(const tr_plane& q, float x, float y, float z) {
    const double dx = (double)x - (double)q.ox, dy = (double)y - (double)q.oy, dz = (double)z - (double)q.oz;
    return fma((double)q.nz, dz, fma((double)q.ny, dy, (double)q.nx * dx));
}
// CULLING: no vertex in the box [lo, hi] has s == 0 or a sign other than all the others (a NaN compares false: never skipped)
TR_HD bool tr_plane_skip(const tr_plane& q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    const bool px = q.nx >= 0.0f, py = q.ny >= 0.0f, pz = q.nz >= 0.0f;
    const double smin = tr_plane_s(q, px ? lox : hix, py ? loy : hiy, pz ? loz : hiz);
    const double smax = tr_plane_s(q, px ? hix : lox, py ? hiy : loy, pz ? hiz : loz);
    return smin > 0.0 || smax < 0.0;
}
// THE PREDICATES on the signed values of the three vertices (activity is the caller's)
TR_HD bool tr_plane_meets(double s0, double s1, double s2) {
    const int pos = (s0 > 0.0) + (s1 > 0.0) + (s2 > 0.0), neg = (s0 < 0.0) + (s1 < 0.0) + (s2 < 0.0);
    return !(pos == 3 || neg == 3);
}
TR_HD bool tr_plane_cut(double s0, double s1, double s2) {
    const int pos = (s0 > 0.0) + (s1 > 0.0) + (s2 > 0.0), neg = (s0 < 0.0) + (s1 < 0.0) + (s2 < 0.0);
    const int zero = (s0 == 0.0) + (s1 == 0.0) + (s2 == 0.0);
    return pos >= 1 && (neg >= 1 || zero == 2);
}
// THE CROSSING POINT of the edge from its negative vertex u (su < 0) to its positive vertex w (sw > 0)
TR_HD void tr_plane_cross(double su, double sw, float ux, float uy, float uz, float wx, float wy, float wz, float* p) {
    const double t = su / (su - sw);
    p[0] = (float)fma(t, (double)wx - (double)ux, (double)ux);
    p[1] = (float)fma(t, (double)wy - (double)uy, (double)uy);
    p[2] = (float)fma(t, (double)wz - (double)uz, (double)uz);
}
// one end of THE SEGMENT: the edge from the vertex a (sa <= 0) to the vertex b (sb > 0) of the positive arc, in either direction
// of the walk: a itself where sa == 0, else the crossing from a to b
TR_HD void tr_plane_end(double sa, double sb, float ax, float ay, float az, float bx, float by, float bz, float* p) {
    if (sa == 0.0) { p[0] = ax; p[1] = ay; p[2] = az; }
    else tr_plane_cross(sa, sb, ax, ay, az, bx, by, bz, p);
}
// THE SEGMENT of a cut face (p0, p1: three float32 each).  A face that is not cut (a row the caller misdirected) gets values,
// not a fault: the selects below always name vertices of the face.  (Selects, not indexed arrays: no scratch on the device.)
TR_HD void tr_plane_segment(const tr_plane& q, const tr_tri& t, float* p0, float* p1) {
    const double s0 = tr_plane_s(q, t.ax, t.ay, t.az), s1 = tr_plane_s(q, t.bx, t.by, t.bz), s2 = tr_plane_s(q, t.cx, t.cy, t.cz);
    // edge e runs from vertex e to vertex e + 1: the one on which the walk enters the positive arc, and the one on which it leaves
    const int in = (!(s0 > 0.0) && s1 > 0.0) ? 0 : ((!(s1 > 0.0) && s2 > 0.0) ? 1 : 2);
    const int out = (s0 > 0.0 && !(s1 > 0.0)) ? 0 : ((s1 > 0.0 && !(s2 > 0.0)) ? 1 : 2);
    {   // entering: a = vertex `in` (s <= 0), b = the next one (s > 0)
        const double sa = in == 0 ? s0 : (in == 1 ? s1 : s2), sb = in == 0 ? s1 : (in == 1 ? s2 : s0);
        const float ax = in == 0 ? t.ax : (in == 1 ? t.bx : t.cx), ay = in == 0 ? t.ay : (in == 1 ? t.by : t.cy);
        const float az = in == 0 ? t.az : (in == 1 ? t.bz : t.cz);
        const float bx = in == 0 ? t.bx : (in == 1 ? t.cx : t.ax), by = in == 0 ? t.by : (in == 1 ? t.cy : t.ay);
        const float bz = in == 0 ? t.bz : (in == 1 ? t.cz : t.az);
        tr_plane_end(sa, sb, ax, ay, az, bx, by, bz, p0);
    }
    {   // leaving: b = vertex `out` (s > 0), a = the next one (s <= 0)
        const double sb = out == 0 ? s0 : (out == 1 ? s1 : s2), sa = out == 0 ? s1 : (out == 1 ? s2 : s0);
        const float bx = out == 0 ? t.ax : (out == 1 ? t.bx : t.cx), by = out == 0 ? t.ay : (out == 1 ? t.by : t.cy);
        const float bz = out == 0 ? t.az : (out == 1 ? t.bz : t.cz);
        const float ax = out == 0 ? t.bx : (out == 1 ? t.cx : t.ax), ay = out == 0 ? t.by : (out == 1 ? t.cy : t.ay);
        const float az = out == 0 ? t.bz : (out == 1 ? t.cz : t.az);
        tr_plane_end(sa, sb, ax, ay, az, bx, by, bz, p1);
    }
}

// one triangle against the plane: true iff it is active and meets (cut == 0) / is cut by (cut != 0) the plane; face = its index
TR_HD bool tr_planes_leaf(const tr_bvh_view& b, int32_t slot, const tr_plane& q, int cut, int32_t& face) {
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    const double s0 = tr_plane_s(q, t.ax, t.ay, t.az), s1 = tr_plane_s(q, t.bx, t.by, t.bz), s2 = tr_plane_s(q, t.cx, t.cy, t.cz);
    face = t.face;
    return tr_near_active(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz) && (cut ? tr_plane_cut(s0, s1, s2) : tr_plane_meets(s0, s1, s2));
}

// both child ids of an internal node and whether each child box is skipped
struct tr_planes_node { int32_t c0, c1; bool skip0, skip1; };
TR_HD tr_planes_node tr_planes_load(const tr_bvh_view& b, int32_t node, const tr_plane& q) {
    const tr_f4* p = reinterpret_cast<const tr_f4*>(b.nodes + node);
    const tr_f4 n0 = p[0], n1 = p[1], n2 = p[2], n3 = p[3];      // lo.x lo.y lo.z hi.z | hi.x hi.y lo.x lo.y | lo.z hi.z hi.x hi.y | c0 c1 ..
    tr_planes_node r;
    r.skip0 = tr_plane_skip(q, n0.x, n0.y, n0.z, n1.x, n1.y, n0.w);
    r.skip1 = tr_plane_skip(q, n1.z, n1.w, n2.x, n2.z, n2.w, n2.y);
    r.c0 = (int32_t)tr_f2u(n3.x); r.c1 = (int32_t)tr_f2u(n3.y);
    return r;
}

// what a lane brings back from a ROUND: the arena slots of its candidates and the node ids it pushes (-1 = none)
struct tr_planes_found { int32_t leaf0, leaf1, push0, push1; };
TR_HD tr_planes_found tr_planes_visit(const tr_bvh_view& b, int32_t node, const tr_plane& q) {
    tr_planes_found f;
    f.leaf0 = -1; f.leaf1 = -1; f.push0 = -1; f.push1 = -1;
    if (node >= 0) {
        const tr_planes_node n = tr_planes_load(b, node, q);
        if (!n.skip0) { if (n.c0 < 0) f.leaf0 = ~n.c0; else f.push0 = n.c0; }
        if (!n.skip1) { if (n.c1 < 0) f.leaf1 = ~n.c1; else f.push1 = n.c1; }
    }
    return f;
}
// the rank of `lane` among the lanes of `mask`: the ballot prefix of pushes and of recorded rows
TR_HD int32_t tr_planes_rank(uint64_t mask, int lane) { return (int32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }
TR_HD int32_t tr_planes_popc(uint64_t mask) { return (int32_t)__builtin_popcountll(mask); }

// THE SUBTREE WALK of a lane (see OVERFLOW).  node < 0: nothing to walk.  phase 0: arriving from above (child 0 next), 1: child 0
// done (child 1 next), 2: both done (climb, or stop at the root)
struct tr_planes_sub { int32_t node, root, next, phase; };
TR_HD void tr_planes_sub_init(tr_planes_sub& w) { w.node = -1; w.root = -1; w.next = -1; w.phase = 0; }
TR_HD void tr_planes_sub_start(tr_planes_sub& w, int32_t root) {
    const bool idle = w.node < 0;      // (selects: a store through a selected address would put the state into scratch)
    w.next = idle ? w.next : root;
    w.root = idle ? root : w.root;
    w.phase = idle ? 0 : w.phase;
    w.node = idle ? root : w.node;
}
// advance to the next candidate: its arena slot, or -1 when the lane's subtrees are exhausted (then w.node < 0)
TR_HD int32_t tr_planes_sub_next(const tr_bvh_view& b, const tr_plane& q, tr_planes_sub& w) {
    while (w.node >= 0) {
        if (w.phase == 2) {
            if (w.node == w.root) {      // back at the root of the subtree: on to the one that waits, if any
                w.node = w.next; w.root = w.next; w.next = -1; w.phase = 0;
                continue;
            }
            const int32_t parent = b.links[w.node].parent;
            w.phase = b.nodes[parent].c0 == w.node ? 1 : 2;
            w.node = parent;
            continue;
        }
        const tr_planes_node n = tr_planes_load(b, w.node, q);
        const int32_t c = w.phase ? n.c1 : n.c0;
        const bool skip = w.phase ? n.skip1 : n.skip0;
        w.phase++;
        if (skip) continue;
        if (c < 0) return ~c;
        w.node = c;
        w.phase = 0;
    }
    return -1;
}

// the walk has what it came for: ANY a face, FILL all its rows (cursor = faces found so far)
template <int MODE>
TR_HD bool tr_planes_full(int32_t cursor, int32_t limit) {
    return MODE == TR_PLANES_ANY ? cursor > 0 : (MODE == TR_PLANES_FILL ? cursor >= limit : false);
}

// THE ORDERING.  Pair t = 0, 1, .. of the step (k, j) of the network: j == 0 is the first step of the merge of two runs of k (i
// against its mirror image i ^ (2k - 1)), j = k/2 .. 1 the later ones (i against i ^ j).  i < p always, and i grows with t.
TR_HD void tr_planes_pair(uint32_t t, uint32_t k, uint32_t j, uint32_t& i, uint32_t& p) {
    const uint32_t r = t & ((j ? j : k) - 1u);
    i = ((t - r) << 1) + r;
    p = j ? i + j : (i ^ (2u * k - 1u));
}
// one compare-exchange, the smaller key to the smaller index; s (may be null): a word per row that rides along, s_stride apart
TR_HD void tr_planes_cx(int32_t* f, int32_t* s, int64_t s_stride, uint32_t i, uint32_t p) {
    const int32_t a = f[i], c = f[p];
    if (a > c) {
        f[i] = c; f[p] = a;
        if (s) { const int32_t x = s[i * s_stride]; s[i * s_stride] = s[p * s_stride]; s[p * s_stride] = x; }
    }
}
// every pair of one step that lies below m, for the worker `first` of `workers` (the kernel: a thread of the workgroup, with a
// barrier between the steps; the host: one worker)
TR_HD void tr_planes_step(int32_t* f, int32_t* s, int64_t s_stride, uint32_t m, uint32_t k, uint32_t j, uint32_t first, uint32_t workers) {
    for (uint32_t t = first;; t += workers) {
        uint32_t i, p;
        tr_planes_pair(t, k, j, i, p);
        if (i >= m) break;
        if (p < m) tr_planes_cx(f, s, s_stride, i, p);
    }
}

// the plane that owns row r: the largest i in [0, n) with offsets[i] <= r (0 where there is none); the caller checks that r is
// one of its rows.  n >= 1.  Terminates and stays in [0, n) whatever offsets holds.
TR_HD int64_t tr_planes_owner(const int64_t* offsets, int64_t n, int64_t r) {
    int64_t a = 0, z = n - 1;
    while (a < z) {
        const int64_t mid = a + (z - a + 1) / 2;
        if (offsets[mid] <= r) a = mid; else z = mid - 1;
    }
    return a;
}
// the segment of row r of plane q from the slot that rode beside its face (clamped: wrong, never outside); num_tris >= 1
TR_HD void tr_planes_row(const tr_bvh_view& b, const tr_plane& q, int32_t slot, float* seg6) {
    slot = slot < 0 ? 0 : ((int64_t)slot < b.num_tris ? slot : (int32_t)(b.num_tris - 1));
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    float p0[3], p1[3];
    tr_plane_segment(q, t, p0, p1);
    seg6[0] = p0[0]; seg6[1] = p0[1]; seg6[2] = p0[2]; seg6[3] = p1[0]; seg6[4] = p1[1]; seg6[5] = p1[2];
}
