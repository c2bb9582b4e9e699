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
// THE SET WALK (tr_within_visit, one node per call, from the root).  Both child boxes are bounded (tr_near_load); children that
// are leaves are evaluated where their bound does not exceed R2 and recorded (FILL), counted (COUNT) or end the walk (ANY);
// of the internal children that survive, the nearer is visited next and the other is pushed.  The threshold never moves, so
// a pushed entry never dies: stack entries are NODE IDS ONLY, 4 bytes, TR_WITHIN_STACK = 32 of them per lane.  A push that
// does not fit sets the sticky lost bit of st.sp; a lane that ends with it set DISCARDS its partial count / write cursor and
// repeats the whole walk without a stack, through the parent links (tr_within_rewalk, as tr_near_rewalk): nothing is counted
// twice.  Each walk visits a node at most once, so the faces one walk records are distinct.  Below two triangles there is no
// hierarchy: the one triangle is tested directly.
// FILL writes the faces of a point in walk order at its rows -- never more than `limit` = the rows the caller's count / offsets
// / total leave it, whatever the walk finds -- and ends once they are full; tr_within_rows then puts the segment into ascending
// face order (an in-place heapsort that carries the arena slot beside the face when rows are to be evaluated) and evaluates
// the optional outputs per (point, face).
//
// THE BOUNDED NEAREST is the walk of tr_nearest.h with one change: the best starts as {d2 = R2, face = INT_MAX, slot = -1}
// instead of tr_near_init.  tr_near_leaf's comparison then accepts a face at exactly R2 (its index is below INT_MAX) and
// rejects anything farther; tr_near_seed, tr_near_visit, tr_near_rewalk, tr_near_outputs and the 8-byte {node, bound} entries
// are reused unchanged.
#pragma once
#include "tr_nearest.h"

#define TR_WITHIN_STACK 32      // node ids per lane: 32 x 4 B x 128 lanes = 16 KB of LDS per workgroup

enum tr_within_mode { TR_WITHIN_ANY = 0, TR_WITHIN_COUNT = 1, TR_WITHIN_FILL = 2 };

// what a lane has found: `count` faces, of which the first min(count, limit) were written (FILL)
struct tr_within_acc {
    int32_t count;
    int32_t limit;      // FILL: rows this point may write
    int32_t* face;      // FILL: its rows of the face list
    int32_t* slot;      // FILL: its rows of the slot scratch, or null
};
struct tr_within_state {
    int32_t node;    // next internal node to visit, -1 = nothing left
    uint32_t sp;     // 2 * entries in use | lost
};

TR_HD bool tr_within_valid(float px, float py, float pz, float r) { return tr_near_valid(px, py, pz) && r >= 0.0f; }
TR_HD double tr_within_r2(float r) { return (double)r * (double)r; }
TR_HD bool tr_within_lost(uint32_t sp) { return (sp & 1u) != 0; }
// the walk has what it came for: ANY a face, FILL all its rows
template <int MODE>
TR_HD bool tr_within_full(const tr_within_acc& acc) {
    return MODE == TR_WITHIN_ANY ? acc.count > 0 : (MODE == TR_WITHIN_FILL ? acc.count >= acc.limit : false);
}

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

// Stack: entry e of a lane is word e of its column of a tr_ring.  cap2 = 2 * entries the walk may use.
TR_HD void tr_within_push(const tr_ring stack, uint32_t cap2, uint32_t& sp, int32_t node) {
    const uint32_t w = sp & ~1u;
    if (w < cap2) {
        tr_ring_put(stack, w >> 1, node);
        sp += 2u;
    } else {
        sp |= 1u;
    }
}
TR_HD int32_t tr_within_pop(const tr_ring stack, uint32_t& sp) {
    if (sp < 2u) return -1;
    sp -= 2u;
    return tr_ring_get(stack, sp >> 1);
}

// visit st.node (>= 0): see THE SET WALK
template <int MODE>
TR_HD void tr_within_visit(const tr_bvh_view& b, float px, float py, float pz, double R2, tr_within_state& st, tr_within_acc& acc,
                           const tr_ring stack, uint32_t cap2) {
    const tr_near_node n = tr_near_load(b, st.node, px, py, pz);
    const bool swap = n.lb1 < n.lb0;
    const int32_t cn = swap ? n.c1 : n.c0, cf = swap ? n.c0 : n.c1;
    const double ln = swap ? n.lb1 : n.lb0, lf = swap ? n.lb0 : n.lb1;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? cf : cn;
        const double lb = k ? lf : ln;
        if (c < 0 && !(lb > R2) && !tr_within_full<MODE>(acc)) tr_within_leaf<MODE>(b, ~c, px, py, pz, R2, acc);
    }
    if (tr_within_full<MODE>(acc)) { st.node = -1; return; }
    const bool go_n = cn >= 0 && !(ln > R2), go_f = cf >= 0 && !(lf > R2);
    if (go_n) {
        if (go_f) tr_within_push(stack, cap2, st.sp, cf);
        st.node = cn;
    } else if (go_f) {
        st.node = cf;
    } else {
        st.node = tr_within_pop(stack, st.sp);
    }
}

// the whole tree again without a stack (after a lost push; the caller has reset acc.count): children in fixed order, up
// through the parent links.  phase 0: arriving from above (child 0 next), 1: child 0 done (child 1 next), 2: both done (climb)
template <int MODE>
TR_HD void tr_within_rewalk(const tr_bvh_view& b, float px, float py, float pz, double R2, tr_within_acc& acc) {
    int32_t node = 0;
    int phase = 0;
    for (;;) {
        if (tr_within_full<MODE>(acc)) break;
        if (phase == 2) {
            const int32_t parent = b.links[node].parent;
            if (parent < 0) break;
            phase = b.nodes[parent].c0 == node ? 1 : 2;
            node = parent;
            continue;
        }
        const tr_near_node n = tr_near_load(b, node, px, py, pz);
        const int32_t c = phase ? n.c1 : n.c0;
        const double lb = phase ? n.lb1 : n.lb0;
        phase++;
        if (lb > R2) continue;
        if (c < 0) {
            tr_within_leaf<MODE>(b, ~c, px, py, pz, R2, acc);
        } else {
            node = c;
            phase = 0;
        }
    }
}

// the rows a point may write: [off, off + count) cut to [0, total); nothing for a negative count or an offset outside
TR_HD int32_t tr_within_limit(int32_t count, int64_t off, int64_t total) {
    if (count <= 0 || off < 0 || off >= total) return 0;
    const int64_t room = total - off;
    return (int64_t)count < room ? count : (int32_t)room;
}

// m rows into ascending face order, in place; s (the slots beside the faces) may be null.  A heapsort: no scratch, and every
// index it forms is below m whatever the rows hold.
TR_HD void tr_within_swap(int32_t* f, int32_t* s, int32_t i, int32_t j) {
    const int32_t a = f[i]; f[i] = f[j]; f[j] = a;
    if (s) { const int32_t c = s[i]; s[i] = s[j]; s[j] = c; }
}
TR_HD void tr_within_sift(int32_t* f, int32_t* s, int32_t root, int32_t end) {
    for (;;) {
        int32_t child = 2 * root + 1;
        if (child >= end) break;
        if (child + 1 < end && f[child] < f[child + 1]) child++;
        if (!(f[root] < f[child])) break;
        tr_within_swap(f, s, root, child);
        root = child;
    }
}
TR_HD void tr_within_sort(int32_t* f, int32_t* s, int32_t m) {
    for (int32_t i = m / 2 - 1; i >= 0; i--) tr_within_sift(f, s, i, m);
    for (int32_t end = m - 1; end > 0; end--) {
        tr_within_swap(f, s, 0, end);
        tr_within_sift(f, s, 0, end);
    }
}

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

// one point, start to end, on one lane (the host simulation; the kernel runs the first walk as a wave loop).
// stack_entries: 1 .. TR_WITHIN_STACK, 0 = all of them.  Returns the number of faces within (FILL: min(it, acc.limit) rows are
// written and still in walk order); *lost (may be null): the first walk overflowed its stack.
template <int MODE>
TR_HD int32_t tr_within_query(const tr_bvh_view& b, float px, float py, float pz, float r, const tr_ring stack, int stack_entries,
                              tr_within_acc& acc, bool* lost) {
    const bool valid = tr_within_valid(px, py, pz, r) && b.num_tris > 0;
    const double R2 = tr_within_r2(r);
    acc.count = 0;
    if (lost) *lost = false;
    if (valid && b.num_tris >= 2 && !tr_within_full<MODE>(acc)) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_WITHIN_STACK);
        tr_within_state st;
        st.node = 0; st.sp = 0;
        while (st.node >= 0) tr_within_visit<MODE>(b, px, py, pz, R2, st, acc, stack, cap2);
        if (lost) *lost = tr_within_lost(st.sp);
        if (tr_within_lost(st.sp) && !tr_within_full<MODE>(acc)) {
            acc.count = 0;
            tr_within_rewalk<MODE>(b, px, py, pz, R2, acc);
        }
    } else if (valid && !tr_within_full<MODE>(acc)) {
        tr_within_leaf<MODE>(b, 0, px, py, pz, R2, acc);      // no hierarchy below two triangles
    }
    return acc.count;
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
        if (tr_near_lost(st.sp)) tr_near_rewalk(b, px, py, pz, best);
    } else if (valid) {
        tr_near_leaf(b, 0, px, py, pz, best);
    }
    tr_near_outputs(b, px, py, pz, valid, best, closest3, distance, tri);
}
