// tr_within.h -- radius queries (include/triro_within.h): the faces of a mesh within a distance r of a point.  Host + device,
// as tr_nearest.h, whose per-triangle function, box bound and activity rule it uses UNCHANGED and to which it adds nothing:
// k_within<> and k_within_closest (within.hip) instantiate the walks per lane, tests/host_sim/within_sim.cpp compiles the
// very same functions with g++.  Not a CPU fallback: nothing in the C ABI reaches the host instantiation.
//
// THE CONTRACT.  Query point p (three float32), radius r (float32, per point or one for all), the mesh of the handle.
//
//  * R2 = (double)r * (double)r.  The product of two float32 is exact in float64, so sqrt(R2) == r exactly; r = 3e38 gives a
//    finite R2 (9e76), r = +Inf gives +Inf.
//  * The query is VALID when p is finite and r >= 0: -0.0 and +Inf are valid radii, NaN and negative ones are not.
//  * Face T is WITHIN iff tr_near_active(T) and tr_near_tri(p, T).d2 <= R2 -- not strict: a face at exactly r is within.
//    r = 0 keeps the faces that contain p exactly (computed d2 == 0), r = +Inf keeps every active face.
//  * any = at least one face is within; count = how many are (int32); list = those faces by ORIGINAL FACE INDEX, ASCENDING,
//    at rows offsets[i] .. offsets[i] + count[i] (uncapped; int64 offsets).  Optional per row: distance =
//    tr_near_distance(d2) and closest = the float32-rounded candidate point, both as tr_near_outputs computes them for that
//    face.  A row is a pure function of (p, face).
//  * BOUNDED NEAREST = the lexicographic minimum of (d2, face) over the faces within, else the miss values.  It equals
//    tr_closest_point's winner, bit for bit, where that winner's float64 d2 <= R2.  (The float32 distance <= r does NOT
//    imply that: a d2 slightly above R2 can round to r.  The identity is one of d2.)
//  * An invalid query, a mesh of zero triangles or one without an active triangle: any = 0, count = 0, an empty list, and for
//    the bounded nearest (-1, +Inf, NaN) as tr_closest_point.  Every element of every output is written.
//  * Everything is a pure function of (p, r, the set of triangles): independent of traversal order, stack capacity and launch
//    shape.
//
// CULLING.  A subtree is skipped iff tr_near_box(p, its box) > R2, strictly.  tr_near_box is a lower bound of the COMPUTED d2
// of every triangle below the box (tr_nearest.h, THE BOUND: rounding is monotone, no margin needed), so a skipped subtree
// holds no face with d2 <= R2, a face at exactly r included.  Boxes with NaN or Inf behave as there: a NaN difference
// selects the bound 0, and nothing exceeds R2 = +Inf.
//
// THE WALK is THE SET WALK of tr_walk.h (the node-id stack, the re-walk of a lane that lost a push, tr_set_query) with this
// visit (tr_within_visit): both child boxes are bounded (tr_near_load); children that are leaves are evaluated where their
// bound does not exceed R2; of the internal children that survive, the nearer is visited next and the other is pushed.  The
// threshold never moves, so a pushed entry never dies: TR_WITHIN_STACK = 32 node ids per lane.
// FILL writes the faces of a point in walk order at its rows -- never more than `limit` = the rows the caller's count / offsets
// / total leave it, whatever the walk finds -- and ends once they are full; tr_within_rows then puts the segment into ascending
// face order (an in-place heapsort that carries the arena slot beside the face when rows are to be evaluated) and evaluates
// the optional outputs per (point, face).
//
// THE BOUNDED NEAREST is the walk of tr_nearest.h with one change: the best starts as {d2 = R2, face = INT_MAX, slot = -1}
// instead of tr_near_init.  tr_near_leaf's comparison then accepts a face at exactly R2 (its index is below INT_MAX) and
// rejects anything farther; tr_near_seed, tr_near_visit, tr_near_probe, tr_near_outputs and the 8-byte {node, bound} entries
// are reused unchanged.
#pragma once
#include "tr_nearest.h"

#define TR_WITHIN_STACK 32      // node ids per lane: 32 x 4 B x 128 lanes = 16 KB of LDS per workgroup

enum tr_within_mode { TR_WITHIN_ANY = TR_SET_ANY, TR_WITHIN_COUNT = TR_SET_COUNT, TR_WITHIN_FILL = TR_SET_FILL };

// what a lane has found: `count` faces, of which the first min(count, limit) were written (FILL)
struct tr_within_acc {
    int32_t count;
    int32_t limit;      // FILL: rows this point may write
    int32_t* face;      // FILL: its rows of the face list
    int32_t* slot;      // FILL: its rows of the slot scratch, or null
};

TR_HD bool tr_within_valid(float px, float py, float pz, float r) { return tr_near_valid(px, py, pz) && r >= 0.0f; }
TR_HD double tr_within_r2(float r) { return (double)r * (double)r; }

// one triangle against the radius (a select on activity, as tr_near_leaf: the arithmetic on NaN / Inf is harmless)
template <int MODE>
TR_HD void tr_within_leaf(const tr_bvh_view& b, int32_t slot, float px, float py, float pz, double R2, tr_within_acc& acc) {
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    const tr_near_pt c = tr_near_tri(px, py, pz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
    const bool active = tr_near_active(t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
    if (active && c.d2 <= R2) {
        if (MODE == TR_WITHIN_FILL && acc.count < acc.limit) {
            acc.face[acc.count] = t.face;
            if (acc.slot) acc.slot[acc.count] = slot;
        }
        acc.count++;
    }
}

// visit st.node (>= 0): see THE WALK
template <int MODE>
TR_HD void tr_within_visit(const tr_bvh_view& b, float px, float py, float pz, double R2, tr_walk_state& st, tr_within_acc& acc,
                           const tr_ring stack, uint32_t cap2) {
    const tr_near_node n = tr_near_load(b, st.node, px, py, pz);
    const bool swap = n.lb1 < n.lb0;
    const int32_t cn = swap ? n.c1 : n.c0, cf = swap ? n.c0 : n.c1;
    const double ln = swap ? n.lb1 : n.lb0, lf = swap ? n.lb0 : n.lb1;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? cf : cn;
        const double lb = k ? lf : ln;
        if (c < 0 && !(lb > R2) && !tr_set_full<MODE>(acc)) tr_within_leaf<MODE>(b, ~c, px, py, pz, R2, acc);
    }
    if (tr_set_full<MODE>(acc)) { st.node = -1; return; }
    const bool go_n = cn >= 0 && !(ln > R2), go_f = cf >= 0 && !(lf > R2);
    if (go_n) {
        if (go_f) tr_walk_push(stack, cap2, st.sp, cf);
        st.node = cn;
    } else if (go_f) {
        st.node = cf;
    } else {
        st.node = tr_walk_pop(stack, st.sp);
    }
}

// the query as tr_walk.h sees it (tr_rewalk, tr_set_query, tr_set_kernel)
template <int MODE>
struct tr_within_probe {
    const tr_bvh_view& b;
    float px, py, pz;
    double R2;
    tr_within_acc& acc;
    TR_HDM bool done() const { return tr_set_full<MODE>(acc); }
    TR_HDM void leaf(int32_t slot) const { tr_within_leaf<MODE>(b, slot, px, py, pz, R2, acc); }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_near_node n = tr_near_load(b, node, px, py, pz);
        c = phase ? n.c1 : n.c0;
        return !((phase ? n.lb1 : n.lb0) > R2);
    }
    TR_HDM void visit(tr_walk_state& st, const tr_ring stack, uint32_t cap2) const {
        tr_within_visit<MODE>(b, px, py, pz, R2, st, acc, stack, cap2);
    }
};

// the rows a point may write: tr_rows_limit under the name the host simulations of within, boxes, tris and planes call
TR_HD int32_t tr_within_limit(int32_t count, int64_t off, int64_t total) { return tr_rows_limit(count, off, total); }

// m rows into ascending face order, in place (tr_rows_sort); s (the slots beside the faces) may be null
struct tr_within_sorted {
    int32_t* f;
    int32_t* s;
    TR_HDM bool before(int32_t i, int32_t j) const { return f[i] < f[j]; }
    TR_HDM void swap(int32_t i, int32_t j) const {
        const int32_t a = f[i]; f[i] = f[j]; f[j] = a;
        if (s) { const int32_t c = s[i]; s[i] = s[j]; s[j] = c; }
    }
};
TR_HD void tr_within_sort(int32_t* f, int32_t* s, int32_t m) { tr_rows_sort(tr_within_sorted{f, s}, m); }

// order the m rows of a point and evaluate the optional outputs of each (slot is required for them): as tr_near_outputs
TR_HD void tr_within_rows(const tr_bvh_view& b, float px, float py, float pz, int32_t* face, int32_t* slot, int32_t m, float* distance,
                          float* closest3) {
    tr_within_sort(face, slot, m);
    if (!slot || (!distance && !closest3) || b.num_tris <= 0) return;
    for (int32_t k = 0; k < m; k++) {
        int32_t s = slot[k];
        s = s < 0 ? 0 : ((int64_t)s < b.num_tris ? s : (int32_t)(b.num_tris - 1));      // (rows the caller misdirected: wrong, never outside)
        tr_counters* nc = nullptr;
        const tr_tri t = tr_load_tri<false, false>(b, s, nc);
        const tr_near_pt c = tr_near_tri(px, py, pz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
        if (distance) distance[k] = tr_near_distance(c.d2);
        if (closest3) { closest3[3 * k] = (float)c.x; closest3[3 * k + 1] = (float)c.y; closest3[3 * k + 2] = (float)c.z; }
    }
}

// one point, start to end, on one lane (the host simulation: tr_set_query); stack_entries: 1 .. TR_WITHIN_STACK, 0 = all of them
template <int MODE>
TR_HD int32_t tr_within_query(const tr_bvh_view& b, float px, float py, float pz, float r, const tr_ring stack, int stack_entries,
                              tr_within_acc& acc, bool* lost) {
    const tr_within_probe<MODE> probe = {b, px, py, pz, tr_within_r2(r), acc};
    return tr_set_query(b, probe, tr_within_valid(px, py, pz, r), stack, stack_entries, TR_WITHIN_STACK, lost);
}

// the bounded nearest: where the best starts (see THE BOUNDED NEAREST)
TR_HD void tr_within_closest_init(tr_near_best& best, double R2) { best.d2 = R2; best.face = 0x7fffffff; best.slot = -1; }

// one point, start to end, on one lane; stack_entries: 1 .. TR_NEAR_STACK, 0 = all of them
TR_HD void tr_within_closest_query(const tr_bvh_view& b, float px, float py, float pz, float r, const tr_ring stack, int stack_entries,
                                   float* closest3, float* distance, int32_t* tri) {
    const bool valid = tr_within_valid(px, py, pz, r) && b.num_tris > 0;
    tr_near_best best;
    tr_within_closest_init(best, tr_within_r2(r));
    if (valid && b.num_tris >= 2) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
        tr_near_state st;
        for (int32_t node = 0; node >= 0;) node = tr_near_seed(b, node, px, py, pz, best);
        st.node = 0; st.sp = 0;
        while (st.node >= 0) tr_near_visit(b, px, py, pz, st, best, stack, cap2);
        if (tr_near_lost(st.sp)) tr_rewalk(b, tr_near_probe{b, px, py, pz, best});
    } else if (valid) {
        tr_near_leaf(b, 0, px, py, pz, best);
    }
    tr_near_outputs(b, px, py, pz, valid, best, closest3, distance, tri);
}
