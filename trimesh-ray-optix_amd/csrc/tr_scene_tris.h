// tr_scene_tris.h -- triangle queries over INSTANCES (include/triro_scene_tris.h): the (instance, face) pairs of a scene
// (tr_scene.h: placed copies of several meshes) that meet a world triangle, the narrow phase of a mesh against placed copies.
// Host + device.  It includes tr_scene_nearest.h -- the placement as a walk holds it (tr_scene_near_map), the placed box
// (tr_scene_near_place) and the proof that it holds what lies below -- and tr_tris.h -- the predicate, the degenerate rule, the
// box of the query -- and CHANGES NEITHER: what is added here is their composition, the instance loop around the set walk of
// tr_walk.h, the overflow rule of a set walk inside that loop and the row order across instances.  k_scene_tris<> and
// k_scene_tris_rows (scene_tris.hip) run these functions with each member walk as a wave loop,
// tests/host_sim/scene_tris_sim.cpp compiles the very same functions with g++.  Not a CPU fallback: nothing in the C ABI
// reaches the host instantiation.
//
// THE CONTRACT.  Query: a world triangle Q = (p, q, r) of nine float32; the committed scene.
//  1. PLACED TRIANGLES: exactly rule 1 of tr_scene_nearest.h.  For a valid instance k (TR_SCENE_VALID of the committed table)
//     the placed vertices of a member face are tr_scene_point(rec.M, v) of its three float32 vertices: float32 values, three
//     fmaf each.  The placed triangle is ACTIVE iff its nine placed coordinates are finite (tr_near_active on the placed values):
//     a member vertex that is not finite places to a non-finite one, and a finite one whose placed coordinates overflow is
//     inactive just the same.  Invalid instances and members without triangles offer nothing.
//  2. MEETS.  The pair (k, f) meets Q iff Q is live (tr_tris_live: nine finite values and a float64 normal that is not exactly
//     0), the placed triangle is active and tr_tris_meets(Q, tr_tris_box(Q), placed a, placed b, placed c) is true.  The
//     degenerate rule of tr_tris.h is evaluated on the PLACED float32 coordinates: a face that has area in its member and none
//     once placed (a nearly singular placement that still has a finite inverse, an underflow) is never met, and one whose
//     collinear vertices place, through rounding, to a triangle with area can be: only the placed coordinates decide, as on
//     the baked mesh.  Nothing new is evaluated per pair.
//  3. OUTPUTS.  any (uint8) = some pair meets Q; count (int32) = the number of meeting (instance, face) pairs over all
//     instances -- more than 2^31 - 1 pairs for one query are OUTSIDE THE CONTRACT, as in tr_scene_cross.h; list = the pairs
//     ascending by (instance, face index in the member mesh), at rows offsets[i] .. offsets[i] + count[i] (int64 offsets from
//     tr_hits_scan).  Every element of every output given is written, for invalid and degenerate queries as well (0 / 0 / no
//     rows).  An empty scene gives 0 / 0 / no rows.
//  4. PURITY.  A pure function of (Q, instances, member triangles): independent of the order in which instances or nodes are
//     visited, of stack capacity and of launch shape.
//
// TWO IDENTITIES.
//  * BAKED MESH.  Let the baked mesh concatenate, in instance order, the faces of every valid instance with vertices placed by
//    the same chain in float32 (tests/host_sim/scene_nearest_sim.bake).  The scene's any, count and rows equal tr_tris_any /
//    _count / _fill on the baked mesh, (instance, face) mapping to the baked index through the instance offsets: both evaluate
//    tr_near_active and tr_tris_meets on the same float32 triangles, and ascending (instance, face) IS ascending baked index.
//    This is the oracle.
//  * IDENTITY PLACEMENT.  One instance at the identity gives tr_tris_any / _count / _fill of that mesh, WITHOUT the
//    negative-zero caveat of the ray and nearest scenes.  fmaf(1, x, +0) turns a -0 coordinate into +0 (tr_scene.h, NEGATIVE
//    ZEROS), and that is all the identity changes.  No output here carries the sign of a zero: step 1 of the predicate
//    compares (-0 == +0 either way), every float64 difference with a zero operand x - (+-0) or (+-0) - x of a non-zero x is
//    the same number, a difference of two zeros is +0 or -0 and enters only products, sums and comparisons whose results feed
//    comparisons again (a -0 product or axis component compares as 0), and tr_tris_zero tests == 0.  any, count and rows are
//    integers decided by comparisons alone.  tests/test_scene_tris_cpu.py holds a member with negative-zero coordinates to it.
//
// CULLING.  A child box [lo, hi] of a member's hierarchy is placed by tr_scene_near_place -> [LO, HI].  The subtree is skipped
// iff all six placed values are not NaN AND tr_box_apart holds for Q's box against [LO, HI] (tr_scene_tris_apart).  PROOF:
// (c) - (e) of tr_scene_nearest.h give LO_i <= placed coordinate <= HI_i, exactly, for every vertex of every ACTIVE placed
// triangle below the box, whenever no NaN arose on the way (an infinite LO_i or HI_i is an ordinary member of the extended
// reals there); so max(a_i, b_i, c_i) <= HI_i < min(p_i, q_i, r_i) or the mirror image, and step 1 of tr_tris_meets separates
// that triangle with the same exact comparisons.  What is new is only this: the comparison that culls is the comparison of
// step 1 with a bound on its left side, so a skipped subtree holds no pair that meets Q.  A bound that is not proven never
// culls: a NaN among the six values (rule (d) there) keeps the subtree.  (tr_box_apart alone would not do: a NaN on one axis
// compares false, but the bound of ANOTHER axis of the same box rests on the same corners and is proven only with them; the
// rule is the one of tr_scene_near_bound, all six or nothing.)  No margin and no rounding argument of its own.
// The first visit's test of the root's two children is the cull of an instance; the loop over instances is linear: there is no
// structure over them.
//
// THE WALK.  Instances are visited one after the other (any order: `order` of the host query; ascending in the kernel).  The
// tr_boxes_acc is that OF THE WHOLE QUERY, as in tr_scene_cross.h: count accumulates across instances, limit is the query's
// rows.  Per instance the walk is THE SET WALK of tr_walk.h through tr_scene_tris_probe, shaped like tr_set_probe (visit /
// child / leaf / done): the placed box test in visit and child, the leaf loads the member triangle, places it and calls the
// predicate.  TR_TRIS_STACK = 32 node ids per lane; below two triangles the one triangle is tested directly.
// OVERFLOW.  A lane remembers c0 = acc.count before an instance.  If the stack lost a push IN THAT INSTANCE and the query is
// not done(), it sets acc.count = c0 -- dropping what it found in this instance, and nothing else -- and runs tr_rewalk on that
// instance only, before the next instance is begun.  Pairs of earlier instances are never dropped or recounted; within the
// instance each walk visits a node at most once, so nothing is counted twice.  (The set walk of one mesh resets count to 0:
// inside the loop that would drop the earlier instances.)  ANY ends at the first pair, FILL once its rows are full.
// FILL.  After each instance the lane writes instance[c0 .. min(acc.count, acc.limit)) = k beside the faces the leaf wrote
// there (tr_scene_tris_mark, the pattern of tr_scene_cross_mark): never beyond the rows tr_rows_limit(count[i], offsets[i],
// total) names, whatever the walk finds.  tr_scene_tris_rows then orders the m rows of a query in place by (instance, face)
// with tr_rows_sort: no scratch, and every index it forms is below m whatever the rows hold.  Misdirected counts or offsets
// give wrong rows, never a write outside the arrays.
//
// REGISTERS.  The placed vertices stay nine float32 and become float64 inside tr_tris_sat, as on one mesh: the one-axis-at-a-
// time shape of tr_tris.h is kept.  What the compiler would otherwise carry across the walk -- the float64 edges and normal of
// Q -- is derived per leaf, where it is written: tr_scene_tris_leaf passes Q through tr_tn_fresh's empty statement (the
// device of tr_tri_nearest.h, restated here as TR_SCENE_TRIS_FRESH so that this header does not pull in that walk).
#pragma once
#include "tr_scene_nearest.h"
#include "tr_tris.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TR_SCENE_TRIS_FRESH(x) asm volatile("" : "+v"(x))
#else
#define TR_SCENE_TRIS_FRESH(x) ((void)0)
#endif
// REGISTERS: Q as it is, but derived values start from here (the values do not change; on the host it is nothing)
TR_HD void tr_scene_tris_fresh(tr_tris_q& q) {
    TR_SCENE_TRIS_FRESH(q.px); TR_SCENE_TRIS_FRESH(q.py); TR_SCENE_TRIS_FRESH(q.pz);
    TR_SCENE_TRIS_FRESH(q.qx); TR_SCENE_TRIS_FRESH(q.qy); TR_SCENE_TRIS_FRESH(q.qz);
    TR_SCENE_TRIS_FRESH(q.rx); TR_SCENE_TRIS_FRESH(q.ry); TR_SCENE_TRIS_FRESH(q.rz);
}

// CULLING: the object-space box [lo, hi] placed by A is proven apart from the box of the query
TR_HD bool tr_scene_tris_apart(const tr_scene_near_map& A, const tr_box& qb, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    float LO[3], HI[3];
    tr_scene_near_place(A, lox, loy, loz, hix, hiy, hiz, LO, HI);
    const bool proven = LO[0] == LO[0] && LO[1] == LO[1] && LO[2] == LO[2] && HI[0] == HI[0] && HI[1] == HI[1] && HI[2] == HI[2];
    return proven && tr_box_apart(qb, LO[0], LO[1], LO[2], HI[0], HI[1], HI[2]);
}

// both child ids of an internal node and whether the query is proven apart from each placed child box (tr_boxes_load)
TR_HD tr_boxes_node tr_scene_tris_load(const tr_bvh_view& b, const tr_scene_near_map& A, int32_t node, const tr_box& qb) {
    const tr_f4* p = reinterpret_cast<const tr_f4*>(b.nodes + node);
    const tr_f4 n0 = p[0], n1 = p[1], n2 = p[2], n3 = p[3];      // lo.x lo.y lo.z hi.z | hi.x hi.y lo.x lo.y | lo.z hi.z hi.x hi.y | c0 c1 ..
    tr_boxes_node r;
    r.apart0 = tr_scene_tris_apart(A, qb, n0.x, n0.y, n0.z, n1.x, n1.y, n0.w);
    r.apart1 = tr_scene_tris_apart(A, qb, n1.z, n1.w, n2.x, n2.z, n2.w, n2.y);
    r.c0 = (int32_t)tr_f2u(n3.x); r.c1 = (int32_t)tr_f2u(n3.y);
    return r;
}

// one member face, placed, against the query (contract 1 and 2); FILL: its face index into the next row
template <int MODE>
TR_HD void tr_scene_tris_leaf(const tr_bvh_view& b, const tr_scene_near_map& A, int32_t slot, tr_tris_q q, const tr_box& qb, tr_boxes_acc& acc) {
    const tr_scene_near_tri w = tr_scene_near_load_tri(b, A.M, slot);
    tr_scene_tris_fresh(q);
    if (tr_near_active(w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz) &&
        tr_tris_meets(q, qb, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz)) {
        if (MODE == TR_TRIS_FILL && acc.count < acc.limit) acc.key[acc.count] = w.face;
        acc.count++;
    }
}

// the query as tr_walk.h sees it within ONE instance (tr_rewalk and the wave loop of the kernel): tr_set_probe with the placed
// box test and the placed leaf.  acc is the accumulator of the whole query
template <int MODE>
struct tr_scene_tris_probe {
    const tr_bvh_view& b;
    const tr_scene_near_map& A;
    const tr_tris_q& q;
    const tr_box& qb;
    tr_boxes_acc& acc;
    TR_HDM bool done() const { return tr_set_full<MODE>(acc); }
    TR_HDM void leaf(int32_t slot) const { tr_scene_tris_leaf<MODE>(b, A, slot, q, qb, acc); }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_boxes_node n = tr_scene_tris_load(b, A, node, qb);
        c = phase ? n.c1 : n.c0;
        return !(phase ? n.apart1 : n.apart0);
    }
    // visit st.node (>= 0): tr_set_visit with the placed box test
    TR_HDM void visit(tr_walk_state& st, const tr_ring stack, uint32_t cap2) const {
        const tr_boxes_node n = tr_scene_tris_load(b, A, st.node, qb);
#pragma unroll 1
        for (int k = 0; k < 2; k++) {
            const int32_t c = k ? n.c1 : n.c0;
            const bool apart = k ? n.apart1 : n.apart0;
            if (c < 0 && !apart && !done()) leaf(~c);
        }
        if (done()) { st.node = -1; return; }
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
};

// FILL: the instance of the rows an instance's walk wrote: [c0, min(acc.count, acc.limit))
TR_HD void tr_scene_tris_mark(const tr_boxes_acc& acc, int32_t* inst, int32_t c0, int32_t k) {
    const int32_t end = acc.count < acc.limit ? acc.count : acc.limit;
    for (int32_t j = c0; j < end; j++) inst[j] = k;
}

// m rows into ascending (instance, face) order, in place (tr_rows_sort)
struct tr_scene_tris_sorted {
    int32_t* in;
    int32_t* f;
    TR_HDM bool before(int32_t i, int32_t j) const { return in[i] < in[j] || (in[i] == in[j] && f[i] < f[j]); }
    TR_HDM void swap(int32_t i, int32_t j) const {
        const int32_t a = in[i]; in[i] = in[j]; in[j] = a;
        const int32_t c = f[i]; f[i] = f[j]; f[j] = c;
    }
};
TR_HD void tr_scene_tris_rows(int32_t* inst, int32_t* face, int32_t m) { tr_rows_sort(tr_scene_tris_sorted{inst, face}, m); }

// one instance on one lane after its first walk ended with sp (the kernel runs that walk as a wave loop): OVERFLOW
template <int MODE>
TR_HD void tr_scene_tris_again(const tr_bvh_view& b, const tr_scene_tris_probe<MODE>& probe, uint32_t sp, int32_t c0) {
    if (tr_walk_lost(sp) && !probe.done()) {      // cold: this instance's part is dropped, not added to
        probe.acc.count = c0;
        tr_rewalk(b, probe);
    }
}

// one world triangle, start to end, on one lane (the host simulation; the kernel runs each instance's first walk as a wave
// loop).  order (may be null): the order in which the instances are visited, a permutation of 0 .. ninst - 1 (null:
// ascending).  stack_entries: 1 .. TR_TRIS_STACK, 0 = all of them.  inst (FILL): the query's rows of the instance list,
// beside acc.key.  Returns the number of pairs (FILL: min(it, acc.limit) rows are written, in walk order); *lost (may be
// null): some instance's first walk overflowed its stack.
template <int MODE>
TR_HD int32_t tr_scene_tris_query(const tr_scene_member* members, const tr_scene_inst* insts, int32_t ninst, const int32_t* order,
                                  const tr_tris_q& q, const tr_ring stack, int stack_entries, tr_boxes_acc& acc, int32_t* inst, uint8_t* lost) {
    const bool live = tr_tris_live(q);
    const tr_box qb = tr_tris_box(q);
    acc.count = 0;
    if (lost) *lost = 0;
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_TRIS_STACK);
    for (int32_t j = 0; live && j < ninst; j++) {
        if (tr_set_full<MODE>(acc)) break;
        const int32_t k = order ? order[j] : j;
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        tr_scene_near_map A;
        tr_scene_near_map_make(rec.M, A);
        const tr_scene_tris_probe<MODE> probe = {b, A, q, qb, acc};
        const int32_t c0 = acc.count;
        if (b.num_tris >= 2) {
            tr_walk_state st;
            st.node = 0; st.sp = 0;
            while (st.node >= 0) probe.visit(st, stack, cap2);
            if (lost && tr_walk_lost(st.sp)) *lost = 1;
            tr_scene_tris_again<MODE>(b, probe, st.sp, c0);
        } else {
            probe.leaf(0);      // no hierarchy below two triangles (a valid instance has one: contract 2 of tr_scene.h)
        }
        if (MODE == TR_TRIS_FILL && inst) tr_scene_tris_mark(acc, inst, c0, k);
    }
    return acc.count;
}
