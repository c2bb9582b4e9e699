// tr_scene_points.h -- which INSTANCES of a scene hold a point (include/triro_scene_points.h): contains_points over placed
// copies of several meshes -- is the point inside any, inside how many, and the ascending list of the instances it is
// inside.  Host + device.  It includes tr_scene_cross.h -- the instance record, the ray in an instance's frame, validity, the
// crossing predicate, the stack walk without a best hit, the rewalk -- and tr_points.h -- the parity rule of the reference --
// and RESTATES NEITHER: what is added here is two passes per instance, a counter per instance and pass, and a decision
// instead of rows.  k_scene_points<> (scene_points.hip) runs these functions with each pass as a wave loop,
// tests/host_sim/scene_points_sim.cpp compiles the very same functions with g++.  Not a CPU fallback: nothing in the C ABI
// reaches the host instantiation.
//
// THE CONTRACT.
//  * QUERY.  A world point p (three float32); the call carries ONE world direction d (three float32), the d_dir3 of
//    tr_contains_points.
//  * PER VALID INSTANCE k:
//      c+_k = the number of faces of the member for which tr_range_tri accepts the ray tr_scene_ray(rec_k, p, d) under the
//             default bounds tr_range_bounds(0, TR_TMAX): no band, so the predicate is tr_tri_test (tr_range.h, DEFAULTS);
//      c-_k = the same for (p, -d), where -d is the exact negation of each component of the WORLD direction, taken before
//             the transform (tr_scene_points_ray).
//    In words: c+-_k is tr_scene_cross_count of a scene that holds instance k alone.
//    p is INSIDE instance k iff c+_k and c-_k are both odd: tr_point_decide with in_box = true (tr_scene_points_inside).
//    Containment is invariant under an invertible affine map, and an affine map preserves the ray parameter (tr_scene.h):
//    the answer is a composition of contracts that exist and needs no new rounding argument.
//  * WHAT COUNTS AS OUTSIDE.  There is no box test: a point outside a member's root boxes has c+ = 0 or c- = 0 by the walk's
//    own culling.  There is no `broken` output and no retry direction: an OPEN member contains nothing on the side where
//    one of the two rays escapes.
//  * VALIDITY is contract 4 of tr_scene.h.  tr_ray_setup on the world rays (p, +-d) runs once (tr_scene_points_valid); a
//    point that fails is inside nothing, and every output is still written.  A transformed ray that fails tr_ray_setup
//    means "not inside THAT instance" only.  Invalid instances (contract 2) and members without triangles contain nothing.
//  * THE THREE RESULTS.
//      any   = uint8: the point is inside some instance.
//      count = int32: the number of instances it is inside.
//      list  = the indices of those instances, ascending, uncapped, at rows offsets[i] .. offsets[i] + count[i] (int64
//              offsets: tr_hits_scan); the rows a point may write are tr_rows_limit(count[i], offsets[i], total).
//    Every element of every output is written.  Everything is a pure function of (p, d, instances, member triangles): it
//    depends neither on the order in which instances or nodes are visited, nor on stack capacity, nor on launch shape, and
//    is bit-comparable with cross_sim.brute per instance on the rays of scene_sim.transform and a parity in numpy.
//  * A PERMITTED SHORTCUT.  A lane whose c+_k is even need not walk (p, -d) in instance k: the decision does not depend on
//    it (tr_scene_points_second).  It halves the work for points outside an instance.  The host query can be told to walk
//    the second pass regardless (`both`): same bits.
//  * IDENTITIES.  any == (count > 0).  The list of a point is the set of instances k for which the rows of
//    tr_scene_cross_fill on (p, +d) and on (p, -d) each hold an odd number of rows with instance == k.  For ONE instance at
//    the identity, and points and a direction WITHOUT A NEGATIVE-ZERO COMPONENT (the caveat of tr_scene.h, point 3),
//    inside equals the parity of tr_cross_count on (p, +-d) of that mesh.
//
// THE WALK.  Instances are visited one after the other (any order: `order` of the host query; ascending in the kernel).  Per
// instance there are two passes, +d then -d; each is tr_cross_visit<TR_CROSS_COUNT> from the member's root with the stack of
// tr_cross.h (node ids only, TR_CROSS_STACK of them per lane) and a tr_cross_acc OF ITS OWN: the counter is per instance and
// per pass, not the ray-wide accumulator of tr_scene_cross_query.  Below two triangles the one triangle is tested directly
// (tr_scene_cross_single).
// OVERFLOW.  A lane whose stack lost a push in a pass drops THAT PASS'S count -- nothing else -- and runs tr_rewalk (tr_cross_probe) for
// that pass only, before the next pass or instance is begun: the c0 rule of tr_scene_cross.h with c0 = 0.
// MODES.  ANY: a point that has found an instance is finished.  FILL: a containing instance is written into the point's
// rows as it is found, never beyond the rows tr_rows_limit names; the point is finished once they are full.  The kernel
// visits instances in ascending order, so its rows are ascending as written; the host query, which may visit in any
// `order`, sorts its rows afterwards (tr_scene_points_sort).  Misdirected counts or offsets give wrong rows, never a write
// outside the arrays.
#pragma once
#include "tr_scene_cross.h"
#include "tr_points.h"

enum tr_scene_points_mode { TR_SCENE_POINTS_ANY = 0, TR_SCENE_POINTS_COUNT = 1, TR_SCENE_POINTS_FILL = 2 };

// what a point has found: `count` containing instances, of which the first min(count, limit) were written (FILL)
struct tr_scene_points_acc {
    int32_t count;
    int32_t limit;      // FILL: rows this point may write
    int32_t* inst;      // FILL: its rows of the instance list
};

// the point has what it came for: ANY one instance, FILL all its rows
template <int MODE>
TR_HD bool tr_scene_points_done(const tr_scene_points_acc& acc) {
    return MODE == TR_SCENE_POINTS_ANY ? acc.count > 0 : (MODE == TR_SCENE_POINTS_FILL ? acc.count >= acc.limit : false);
}
// one containing instance: counted, and (FILL) written while the point has rows left
template <int MODE>
TR_HD void tr_scene_points_record(tr_scene_points_acc& acc, int32_t k) {
    if (MODE == TR_SCENE_POINTS_FILL && acc.count < acc.limit) acc.inst[acc.count] = k;
    acc.count++;
}

// validity of the world rays (p, +d) and (p, -d), once per point
TR_HD bool tr_scene_points_valid(float px, float py, float pz, float dx, float dy, float dz) {
    tr_ray rw;
    const bool plus = tr_ray_setup(rw, px, py, pz, dx, dy, dz);
    return tr_ray_setup(rw, px, py, pz, -dx, -dy, -dz) && plus;
}
// the ray of a pass (0: +d, 1: -d) in the frame of `rec`: -d is negated in world space, then transformed
TR_HD bool tr_scene_points_ray(const tr_scene_inst& rec, float px, float py, float pz, float dx, float dy, float dz, int pass, tr_ray& r) {
    return tr_scene_ray(rec, px, py, pz, pass ? -dx : dx, pass ? -dy : dy, pass ? -dz : dz, r);
}
// THE SHORTCUT: does the decision depend on the second pass?
TR_HD bool tr_scene_points_second(int32_t cp) { return (cp & 1) != 0; }
// the decision from the two counts of an instance: tr_point_decide without a box and without `broken`
TR_HD bool tr_scene_points_inside(int32_t cp, int32_t cm) {
    bool inside, broken;
    tr_point_decide(true, cp, cm, inside, broken);
    return inside;
}

// m rows into ascending order, in place (the host query after a visit in another order: at most one row per instance)
TR_HD void tr_scene_points_sort(int32_t* inst, int32_t m) {
    for (int32_t i = 1; i < m; i++) {
        const int32_t x = inst[i];
        int32_t j = i;
        for (; j > 0 && inst[j - 1] > x; j--) inst[j] = inst[j - 1];
        inst[j] = x;
    }
}

// one pass of one instance on one lane: the count of the member's faces that the ray crosses under the default bounds.
// *lost (may be null) is set when the walk overflowed its stack.
TR_HD int32_t tr_scene_points_pass(const tr_bvh_view& b, const tr_ray& r, const tr_ring stack, uint32_t cap2, uint8_t* lost) {
    float lo, hi;
    (void)tr_range_bounds(0.0f, TR_TMAX, lo, hi);
    tr_cross_acc ca;
    ca.count = 0; ca.limit = 0; ca.face = nullptr; ca.t = nullptr; ca.slot = nullptr;
    if (b.num_tris >= 2) {
        tr_cross_state st;
        st.node = 0; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
        while (st.node >= 0) tr_cross_visit<TR_CROSS_COUNT>(b, r, lo, hi, st, ca, stack, cap2);
        if (tr_walk_lost(st.sp)) {
            if (lost) *lost = 1;
            ca.count = 0;
            tr_rewalk(b, tr_cross_probe<TR_CROSS_COUNT>{b, r, lo, hi, ca});
        }
    } else {
        tr_scene_cross_single<TR_CROSS_COUNT>(b, r, lo, hi, ca);
    }
    return ca.count;
}

// one world point, start to end, on one lane (the host simulation; the kernel runs each pass as a wave loop).
// order (may be null): the order in which the instances are visited, a permutation of 0 .. ninst - 1 (null: ascending).
// stack_entries: 1 .. TR_CROSS_STACK, 0 = all of them.  both: walk (p, -d) even where c+ is even.  acc.limit / acc.inst
// (FILL): the point's rows.  Returns the number of containing instances found (FILL: min(it, acc.limit) rows are written,
// ascending).  *lost_inst (may be null): the last instance visited in which a pass overflowed its stack, -1: none.
template <int MODE>
TR_HD int32_t tr_scene_points_query(const tr_scene_member* members, const tr_scene_inst* insts, int32_t ninst, const int32_t* order,
                                    float px, float py, float pz, float dx, float dy, float dz, const tr_ring stack, int stack_entries,
                                    bool both, tr_scene_points_acc& acc, int32_t* lost_inst) {
    const bool valid = tr_scene_points_valid(px, py, pz, dx, dy, dz);
    acc.count = 0;
    if (lost_inst) *lost_inst = -1;
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_CROSS_STACK);
    for (int32_t j = 0; valid && j < ninst; j++) {
        if (tr_scene_points_done<MODE>(acc)) break;
        const int32_t k = order ? order[j] : j;
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        int32_t c[2] = {0, 0};
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1 && !both && !tr_scene_points_second(c[0])) break;
            tr_ray r;
            if (!tr_scene_points_ray(rec, px, py, pz, dx, dy, dz, pass, r)) break;      // (both passes fail together: -d is as finite as d)
            uint8_t lost = 0;
            c[pass] = tr_scene_points_pass(b, r, stack, cap2, &lost);
            if (lost && lost_inst) *lost_inst = k;
        }
        if (tr_scene_points_inside(c[0], c[1])) tr_scene_points_record<MODE>(acc, k);
    }
    if (MODE == TR_SCENE_POINTS_FILL && order) tr_scene_points_sort(acc.inst, acc.count < acc.limit ? acc.count : acc.limit);
    return acc.count;
}
