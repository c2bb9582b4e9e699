// tr_scene_cross.h -- every crossing of a world ray over INSTANCES on a per-ray interval [tmin, tmax]
// (include/triro_scene_cross.h): how many (instance, triangle) pairs the ray crosses within the interval, and the uncapped,
// ordered list of them.  Host + device.  It includes tr_scene.h -- the instance record, the transform of a ray into an
// instance's frame, validity -- and tr_cross.h -- the crossing predicate, the box tests, the stack walk, the rewalk and the
// accumulator -- and CHANGES NEITHER: what is added here is the instance loop around the crossing walk and the row order
// across instances.  k_scene_cross<> and k_scene_cross_rows (scene_cross.hip) run these functions with each member walk as
// a wave loop, tests/host_sim/scene_cross_sim.cpp compiles the very same functions with g++.  Not a CPU fallback: nothing in
// the C ABI reaches the host instantiation.
//
// THE CONTRACT.
//  * WORLD RAY, BOUNDS, VALIDITY: exactly contract 4 of tr_scene.h.  tr_ray_setup and tr_range_bounds run ONCE on the world
//    ray (o, d) and its bounds lo = tmin[i] (0 where NULL), hi = tmax[i] (TR_TMAX where NULL); a ray that fails either crosses
//    nothing: count 0, no rows.  The ray in an instance's frame is tr_scene_ray (contract 3); a transformed ray that fails
//    tr_ray_setup crosses nothing IN THAT INSTANCE only.  The bounds are not transformed: lo' and hi' of the world ray are
//    those of every instance.  Invalid instances (contract 2) and members without triangles are crossed by nothing.
//  * A CROSSING is a pair (instance k, face f of its member) for which tr_range_tri accepts the transformed ray on that
//    triangle with the world ray's lo', hi'.  Its distance is the t that predicate returns, UNCHANGED: an affine map
//    preserves the ray parameter (tr_scene.h, WHY IT CAN BE EXACT).  Nothing is carried between instances: there is no best
//    hit, so neither tr_scene_seed nor any argument about G is needed.
//  * count = the number of crossings over all instances, int32.  A ray with more than 2^31 - 1 crossings is OUTSIDE THE
//    CONTRACT (the counter wraps; tr_hits_scan refuses a negative count).
//  * list  = the crossings ordered by (t, instance index, face index) ascending; -0.0 == +0.0 is a tie in t.  The list of
//    ray i occupies the rows offsets[i] .. offsets[i] + count[i] (int64 offsets: tr_hits_scan with the cap INT32_MAX).
//  * row   = instance, face (the index IN THE MEMBER MESH) and t; optionally, as tr_scene_outputs computes them for that
//    (instance, triangle): front (the object-space front, inverted under TR_SCENE_FLIP), loc3 (M applied to the object-space
//    location by tr_scene_point), uv2 (object space); and ray = i + ray_base.
//    A row is a pure function of (ray, bounds, instance record, triangle); the row set is a pure function of (ray, bounds,
//    instances, member triangles).  Neither depends on the order in which instances or nodes are visited, on stack capacity or
//    on launch shape: both are bit-comparable with a brute force -- tr_range_tri on every triangle of every instance on the
//    rays of tr_scene_ray -- followed by any correct sort on (t, instance, face).
//  * IDENTITIES.  count > 0 equals tr_scene_any.  The first row of a ray is tr_scene_closest's (instance, tri, t, front,
//    loc, uv): both minimise (t, instance, face) over the same accepted set.  ONE instance at the identity gives
//    tr_cross_count / tr_cross_fill's count, faces, t, front, uv and loc for rays WITHOUT A NEGATIVE-ZERO COMPONENT (the
//    caveat of tr_scene.h, point 3: the transform turns -0 into +0).
//
// WHY NO NEW PROOF.  Per instance the walk is tr_cross.h's on (o', d', lo', hi'): the two box tests of tr_range.h with no
// best distance, under which no accepted hit is lost (tr_cross.h, CULLING), and the predicate itself.  The instance loop adds
// no cull -- an instance is skipped only by the flag computed at commit (contract 2) -- and no margin: the first visit's
// test of the root's two child boxes against the object-space ray is the cull of an instance, as in tr_scene.h.
//
// THE WALK.  Instances are visited one after the other (any order: `order` of the host query; ascending in the kernel).  The
// tr_cross_acc is that OF THE WHOLE RAY: count accumulates across instances, limit is the ray's rows.  Per instance the
// walk is tr_cross_visit from the member's root with the stack of tr_cross.h (node ids only, TR_CROSS_STACK of them per
// lane); below two triangles the one triangle is tested directly.
// OVERFLOW.  A lane remembers c0 = acc.count before an instance.  If the stack lost a push IN THAT INSTANCE and the rows are
// not yet full, it sets acc.count = c0 -- dropping what it found in this instance, and nothing else -- and runs
// tr_rewalk (tr_cross_probe) on that instance only, before the next instance is begun.  Crossings of earlier instances are never
// dropped or recounted; within the instance each walk visits a node at most once, so nothing is counted twice.
// FILL.  After each instance the lane writes instance[c0 .. min(acc.count, acc.limit)) = k beside the (face, t, slot) that
// tr_cross_record wrote there: never beyond the rows tr_rows_limit(count[i], offsets[i], total) names, whatever the walk
// finds, and the ray is finished once they are full.
// ROWS (tr_scene_cross_rows) then orders the m rows of a ray in place -- a heapsort on (t, instance, face) that carries t,
// instance, face and slot together; no scratch, and every index it forms is below m whatever the rows hold, NaN keys
// included, as tr_cross_sort -- evaluates front / loc / uv per row from (instance, slot) with the instance clamped into
// 0 .. ninst - 1 and the slot clamped into that member's arena, and writes ray.  Misdirected counts or offsets give wrong
// rows, never a write or a read outside the arrays.
#pragma once
#include "tr_scene.h"
#include "tr_cross.h"

// FILL: the instance of the rows an instance's walk wrote: [c0, min(acc.count, acc.limit))
TR_HD void tr_scene_cross_mark(const tr_cross_acc& acc, int32_t* inst, int32_t c0, int32_t k) {
    const int32_t end = acc.count < acc.limit ? acc.count : acc.limit;
    for (int32_t j = c0; j < end; j++) inst[j] = k;
}

// the one triangle of a member without a hierarchy
template <int MODE>
TR_HD void tr_scene_cross_single(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, tr_cross_acc& acc) {
    tr_counters* nc = nullptr;
    const tr_tri w = tr_load_tri<false, false>(b, 0, nc);
    float tt;
    if (tr_range_tri(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, lo, hi, tt)) tr_cross_record<MODE>(acc, w.face, tt, 0);
}

// m rows into ascending (t, instance, face) order, in place (tr_rows_sort); s (the slots beside them) may be null
struct tr_scene_cross_sorted {
    int32_t* in;
    tr_cross_sorted r;
    TR_HDM bool before(int32_t i, int32_t j) const {
        return r.t[i] < r.t[j] || (r.t[i] == r.t[j] && (in[i] < in[j] || (in[i] == in[j] && r.f[i] < r.f[j])));
    }
    TR_HDM void swap(int32_t i, int32_t j) const {
        const int32_t a = in[i]; in[i] = in[j]; in[j] = a;
        r.swap(i, j);
    }
};
TR_HD void tr_scene_cross_sort(float* t, int32_t* in, int32_t* f, int32_t* s, int32_t m) {
    tr_rows_sort(tr_scene_cross_sorted{in, {t, f, s}}, m);
}

// order the m rows of a world ray and evaluate the optional outputs of each (slot is required for front / loc3 / uv2) as
// tr_scene_outputs evaluates its winner.  ray (may be null) gets ray_id in every row.
TR_HD void tr_scene_cross_rows(const tr_scene_member* members, const tr_scene_inst* insts, int32_t ninst, float ox, float oy, float oz,
                               float dx, float dy, float dz, int32_t* inst, int32_t* face, float* t, int32_t* slot, int32_t m,
                               uint8_t* front, float* loc3, float* uv2, int64_t* ray, int64_t ray_id) {
    tr_scene_cross_sort(t, inst, face, slot, m);
    if (ray) for (int32_t k = 0; k < m; k++) ray[k] = ray_id;
    if (!slot || (!front && !loc3 && !uv2) || ninst <= 0) return;
    for (int32_t k = 0; k < m; k++) {
        tr_scene_best g;
        g.t = t[k]; g.face = face[k];
        g.inst = inst[k] < 0 ? 0 : (inst[k] < ninst ? inst[k] : ninst - 1);      // (rows the caller misdirected: wrong, never outside)
        const int64_t nt = members[insts[g.inst].mesh].num_tris;
        g.slot = slot[k] < 0 ? 0 : ((int64_t)slot[k] < nt ? slot[k] : (int32_t)(nt - 1));
        // (a member without triangles has no row of its own: only a misdirected one lands here, and reads nothing)
        tr_scene_outputs(members, insts, ox, oy, oz, dx, dy, dz, nt > 0, g, nullptr, front ? front + k : nullptr, nullptr, nullptr, nullptr,
                         loc3 ? loc3 + 3 * k : nullptr, uv2 ? uv2 + 2 * k : nullptr);
    }
}

// one world ray, start to end, on one lane (the host simulation; the kernel runs each instance's first walk as a wave loop).
// order (may be null): the order in which the instances are visited, a permutation of 0 .. ninst - 1 (null: ascending).
// stack_entries: 1 .. TR_CROSS_STACK, 0 = all of them.  inst (FILL): the ray's rows of the instance list, beside acc.face.
// Returns the number of crossings (FILL: min(it, acc.limit) rows are written, in walk order); *lost (may be null): some
// instance's first walk overflowed its stack.
template <int MODE>
TR_HD int32_t tr_scene_cross_query(const tr_scene_member* members, const tr_scene_inst* insts, int32_t ninst, const int32_t* order,
                                   float ox, float oy, float oz, float dx, float dy, float dz, float tmin, float tmax,
                                   const tr_ring stack, int stack_entries, tr_cross_acc& acc, int32_t* inst, uint8_t* lost) {
    tr_ray rw;
    float lo, hi;
    bool valid = tr_ray_setup(rw, ox, oy, oz, dx, dy, dz);
    valid = tr_range_bounds(tmin, tmax, lo, hi) && valid;
    acc.count = 0;
    if (lost) *lost = 0;
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_CROSS_STACK);
    for (int32_t j = 0; valid && j < ninst; j++) {
        if (tr_cross_full<MODE>(acc)) break;
        const int32_t k = order ? order[j] : j;
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        tr_ray r;
        if (!tr_scene_ray(rec, ox, oy, oz, dx, dy, dz, r)) continue;
        const int32_t c0 = acc.count;
        if (b.num_tris >= 2) {
            tr_cross_state st;
            st.node = 0; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
            while (st.node >= 0) tr_cross_visit<MODE>(b, r, lo, hi, st, acc, stack, cap2);
            if (tr_walk_lost(st.sp)) {
                if (lost) *lost = 1;
                if (!tr_cross_full<MODE>(acc)) {
                    acc.count = c0;
                    tr_rewalk(b, tr_cross_probe<MODE>{b, r, lo, hi, acc});
                }
            }
        } else {
            tr_scene_cross_single<MODE>(b, r, lo, hi, acc);
        }
        if (MODE == TR_CROSS_FILL) tr_scene_cross_mark(acc, inst, c0, k);
    }
    return acc.count;
}
