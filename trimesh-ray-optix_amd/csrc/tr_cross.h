// tr_cross.h -- every crossing of a ray on a per-ray interval [tmin, tmax] (include/triro_cross.h): how many triangles the
// ray crosses within the interval, and the uncapped, ordered list of them.  Host + device, as tr_range.h, whose ray set-up,
// bounds, per-triangle predicate and box tests it uses UNCHANGED and to which it adds nothing: k_cross<> and k_cross_rows
// (cross.hip) instantiate the walk and the ordering per lane, tests/host_sim/cross_sim.cpp compiles the very same functions
// with g++.  Not a CPU fallback: nothing in the C ABI reaches the host instantiation.
//
// THE CONTRACT.  A ray is (o, d), six float32; its bounds are lo = tmin[i] (0 where the array is NULL) and hi = tmax[i]
// (TR_TMAX where NULL).  Ray, validity and bounds are EXACTLY those of tr_range.h:
//
//  * The ray is set up with tr_ray_setup and is NEVER ANCHORED: distances are measured from the origin given.
//  * lo' = max(lo, 0) and hi' = min(hi, TR_TMAX) (tr_range_bounds); the interval is closed.
//  * A NaN bound, an empty interval (lo' > hi') or a non-finite ray component gives NO CROSSING: count 0, no rows.
//
//  * WHAT A CROSSING IS.  Triangle T is a crossing of ray i iff tr_range_tri(ray, T, lo', hi', t) accepts it, and its distance
//    is the t that predicate returns: the float32 t_f, or the float64-derived t_e where a band or an undecided float32 test
//    sent it there (tr_range.h, THE PER-TRIANGLE PREDICATE, with the proof of the band).  The predicate is neither restated
//    nor changed here.  A ray through a shared edge or vertex crosses exactly one owner (tr_tie_own), as everywhere.
//
//  * THE THREE RESULTS.
//      count = the number of crossings, int32, uncapped.
//      list  = the crossings ordered by (t, original face index) ascending, as tr_closer orders them: -0.0 == +0.0 is a tie,
//              broken by the face.  The list of ray i is the rows offsets[i] .. offsets[i] + count[i] (int64 offsets).
//      row   = face and t; optionally front, loc3 and uv2 -- tr_hit_outputs on that triangle -- and ray (int64, = i + ray_base).
//    A row is a pure function of (ray, bounds, face); the row set is a pure function of (ray, bounds, the set of triangles).
//    Neither depends on traversal order, stack capacity or launch shape: both are bit-comparable with a brute force over
//    tr_range_tri followed by any correct sort on (t, face).  The first row is tr_range_closest's answer.
//
// CULLING.  The two tests of tr_range.h with best_t = +Inf: a box with slab interval (tn, tf) is skipped only when
//      (a) tr_slab_hit(tn, tf, hi' * TR_CULL_SLACK) fails, or
//      (b) tf < lo' * TR_RANGE_LO_CUT                                           (tr_range_box, both).
// NO ACCEPTED HIT IS LOST: the argument is that header's with best_t removed.  In (a) the clause "a hit that could still win
// has a distance <= best_t" is not needed, because nothing is ever discarded for a nearer hit: what remains is "an accepted
// hit has a distance <= hi', a float32 one at most 2^-11 beyond the exact one, a box's entry at most 3 u beyond the exact
// entry".  (b) never mentioned best_t.  No new margin.
//
// THE WALK (tr_cross_visit, one node per call, from the root) reads the exact 64-byte node and tests both child boxes
// (tr_node_slabs).  Leaf children that pass are tested at once, the nearer first; of the internal children that pass, the nearer
// is visited next and the farther is pushed.  The threshold never moves, so a pushed entry never dies: stack entries are
// NODE IDS ONLY, 4 bytes, TR_CROSS_STACK = 32 of them per lane (16 KB of LDS per workgroup of 128 lanes), as tr_within.h.
// REGISTERS.  The float64 half stays out of the leaf test: a test that tr_range_fast returns as TR_UNDECIDED parks its slot
// (st.pe0 / st.pe1, one per child) and tr_cross_drain decides it at the END of the visit -- tr_range_drain's sequence: a
// wave-uniform cold skip, the triangle fetched again for the tie question -- and counts or records the hit where
// tr_range_drain folds a best.
// The node-id stack, the lost bit and the re-walk of a lane that lost a push (tr_rewalk on a tr_cross_probe; the partial count
// / write cursor is DISCARDED first, so nothing is counted twice) are THE SET WALK of tr_walk.h.  Below two triangles there
// is no hierarchy: the one triangle is tested directly (tr_range_tri).
//
// FILL writes (face, t, slot) of a ray's crossings in walk order at its rows -- never more than `limit`, the rows the caller's
// count[i], offsets[i] and total leave the ray (tr_rows_limit: [off, off + count) cut to [0, total); nothing for a
// negative count or an offset outside), whatever the walk finds -- and ends once they are full.
// ROWS (tr_cross_rows) then orders the m rows of a ray in place -- a heapsort on (t, face) that carries t, face and slot
// together; no scratch, and every index it forms is below m whatever the rows hold, NaN keys included (a NaN compares false
// both ways: the order of such rows is unspecified, the rows stay a permutation) -- evaluates front / loc / uv per row from
// the slot (clamped into the arena), and writes ray.
#pragma once
#include "tr_range.h"

#define TR_CROSS_STACK 32      // node ids per lane: 32 x 4 B x 128 lanes = 16 KB of LDS per workgroup

enum tr_cross_mode { TR_CROSS_COUNT = 0, TR_CROSS_FILL = 1 };

// what a lane has found: `count` crossings, of which the first min(count, limit) were written (FILL)
struct tr_cross_acc {
    int32_t count;
    int32_t limit;      // FILL: rows this ray may write
    int32_t* face;      // FILL: its rows of the face list
    float* t;           // FILL: its rows of the distances
    int32_t* slot;      // FILL: its rows of the slot scratch, or null
};
struct tr_cross_state {
    int32_t node;       // next internal node to visit, -1 = nothing left
    uint32_t sp;        // 2 * entries in use | lost
    int32_t pe0, pe1;   // leaf tests waiting for the float64 part (tri slots, -1 = none): nearer / farther child
};

// the walk has what it came for: FILL all its rows
template <int MODE>
TR_HD bool tr_cross_full(const tr_cross_acc& acc) { return MODE == TR_CROSS_FILL ? acc.count >= acc.limit : false; }

// one crossing: counted, and (FILL) written while the ray has rows left
template <int MODE>
TR_HD void tr_cross_record(tr_cross_acc& acc, int32_t face, float t, int32_t slot) {
    if (MODE == TR_CROSS_FILL && acc.count < acc.limit) {
        acc.face[acc.count] = face;
        acc.t[acc.count] = t;
        if (acc.slot) acc.slot[acc.count] = slot;
    }
    acc.count++;
}

// the leaf test of the walk: the float32 half here; a test it leaves to the float64 half is parked in `pe`
template <int MODE>
TR_HD void tr_cross_leaf(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, int32_t slot, tr_cross_acc& acc, int32_t& pe) {
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    float tt;
    const int c = tr_range_fast(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, t.esum, lo, hi, tt);
    if (c == TR_UNDECIDED) pe = slot;
    if (c == TR_HIT) tr_cross_record<MODE>(acc, t.face, tt, slot);
}
// decide a parked test (tr_range_exact's sequence, laid out as tr_range_drain: cold, wave-uniform skip when no lane has one,
// the triangle fetched again for the tie question instead of living through the call)
template <int MODE>
TR_HD void tr_cross_drain(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, int32_t& pe, tr_cross_acc& acc) {
    const bool any_parked = TR_WAVE_ANY(pe >= 0);
    if (__builtin_expect(any_parked, 0)) {
        if (pe >= 0) {
            tr_counters* nc = nullptr;
            const tr_tri t = tr_load_tri<false, false>(b, pe, nc);
            const tr_exact_res e = tr_tri_exact_t(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
            float tt = e.t;
            if (__builtin_expect(e.tie != 0, 0)) {
#if defined(__HIP_DEVICE_COMPILE__)
                __asm__ volatile("" ::: "memory");
#endif
                const tr_tri u = tr_load_tri<false, false>(b, pe, nc);
                if (!tr_tie_own(r.dx, r.dy, r.dz, u.ax, u.ay, u.az, u.bx, u.by, u.bz, u.cx, u.cy, u.cz, e.tie)) tt = -1.0f;
            }
            if (tt >= lo && tt <= hi) tr_cross_record<MODE>(acc, t.face, tt, pe);
            pe = -1;
        }
    }
}

// visit st.node (>= 0): see THE WALK
template <int MODE>
TR_HD void tr_cross_visit(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, tr_cross_state& st, tr_cross_acc& acc,
                          const tr_ring stack, uint32_t cap2) {
    const tr_f4* q = reinterpret_cast<const tr_f4*>(b.nodes + st.node);
    const tr_f4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];
    float tn0, tf0, tn1, tf1;
    tr_node_slabs(r, n0, n1, n2, tn0, tf0, tn1, tf1);
    const int32_t c0 = (int32_t)tr_f2u(n3.x), c1 = (int32_t)tr_f2u(n3.y);
    const float lim = hi * TR_CULL_SLACK, cut = lo * TR_RANGE_LO_CUT;
    const bool swap = tn1 < tn0;
    const int32_t cn = swap ? c1 : c0, cf = swap ? c0 : c1;
    const float tnn = swap ? tn1 : tn0, tfn = swap ? tf1 : tf0;
    const float tnf = swap ? tn0 : tn1, tff = swap ? tf0 : tf1;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? cf : cn;
        const float tn = k ? tnf : tnn, tf = k ? tff : tfn;
        if (c < 0 && !tr_cross_full<MODE>(acc) && tr_range_box(tn, tf, lim, cut)) {
            int32_t pe = -1;
            tr_cross_leaf<MODE>(b, r, lo, hi, ~c, acc, pe);
            if (k) st.pe1 = pe; else st.pe0 = pe;
        }
    }
    const bool go_n = cn >= 0 && tr_range_box(tnn, tfn, lim, cut), go_f = cf >= 0 && tr_range_box(tnf, tff, lim, cut);
    if (go_n) {
        if (go_f) tr_walk_push(stack, cap2, st.sp, cf);
        st.node = cn;
    } else if (go_f) {
        st.node = cf;
    } else {
        st.node = tr_walk_pop(stack, st.sp);
    }
    // the end of the visit: the float64 half of what the leaf tests parked
    tr_cross_drain<MODE>(b, r, lo, hi, st.pe0, acc);
    tr_cross_drain<MODE>(b, r, lo, hi, st.pe1, acc);
    if (tr_cross_full<MODE>(acc)) st.node = -1;
}

// the whole tree again without a stack (after a lost push; the caller has reset acc.count):
// tr_rewalk(b, tr_cross_probe<MODE>{b, r, lo, hi, acc}) -- a child is culled as in the walk, a leaf is tested and what it
// parked decided at once
template <int MODE>
struct tr_cross_probe {
    const tr_bvh_view& b;
    const tr_ray& r;
    float lo, hi;
    tr_cross_acc& acc;
    TR_HDM bool done() const { return tr_cross_full<MODE>(acc); }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_f4* q = reinterpret_cast<const tr_f4*>(b.nodes + node);
        const tr_f4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];
        float tn0, tf0, tn1, tf1;
        tr_node_slabs(r, n0, n1, n2, tn0, tf0, tn1, tf1);
        c = (int32_t)tr_f2u(phase ? n3.y : n3.x);
        return tr_range_box(phase ? tn1 : tn0, phase ? tf1 : tf0, hi * TR_CULL_SLACK, lo * TR_RANGE_LO_CUT);
    }
    TR_HDM void leaf(int32_t slot) const {
        int32_t pe = -1;
        tr_cross_leaf<MODE>(b, r, lo, hi, slot, acc, pe);
        tr_cross_drain<MODE>(b, r, lo, hi, pe, acc);
    }
};

// the rows a ray may write: tr_rows_limit under the name the host simulations of cross, scene_cross and scene_points call
TR_HD int32_t tr_cross_limit(int32_t count, int64_t off, int64_t total) { return tr_rows_limit(count, off, total); }

// m rows into ascending (t, face) order, in place (tr_rows_sort); s (the slots beside them) may be null
struct tr_cross_sorted {
    float* t;
    int32_t* f;
    int32_t* s;
    TR_HDM bool before(int32_t i, int32_t j) const { return tr_closer(t[i], f[i], t[j], f[j]); }
    TR_HDM void swap(int32_t i, int32_t j) const {
        const float x = t[i]; t[i] = t[j]; t[j] = x;
        const int32_t a = f[i]; f[i] = f[j]; f[j] = a;
        if (s) { const int32_t c = s[i]; s[i] = s[j]; s[j] = c; }
    }
};
TR_HD void tr_cross_sort(float* t, int32_t* f, int32_t* s, int32_t m) { tr_rows_sort(tr_cross_sorted{t, f, s}, m); }

// order the m rows of a ray and evaluate the optional outputs of each (slot is required for front / loc3 / uv2): as
// tr_range_outputs evaluates its winner.  ray (may be null) gets ray_id in every row.
TR_HD void tr_cross_rows(const tr_bvh_view& b, const tr_ray& r, int32_t* face, float* t, int32_t* slot, int32_t m, uint8_t* front,
                         float* loc3, float* uv2, int64_t* ray, int64_t ray_id) {
    tr_cross_sort(t, face, slot, m);
    if (ray) for (int32_t k = 0; k < m; k++) ray[k] = ray_id;
    if (!slot || (!front && !loc3 && !uv2) || b.num_tris <= 0) return;
    for (int32_t k = 0; k < m; k++) {
        int32_t s = slot[k];
        s = s < 0 ? 0 : ((int64_t)s < b.num_tris ? s : (int32_t)(b.num_tris - 1));      // (rows the caller misdirected: wrong, never outside)
        tr_counters* nc = nullptr;
        const tr_tri w = tr_load_tri<false, false>(b, s, nc);
        float loc[3], uv[2];
        const bool fr = tr_hit_outputs(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, loc, uv);
        if (front) front[k] = fr ? 1 : 0;
        if (loc3) { loc3[3 * k] = loc[0]; loc3[3 * k + 1] = loc[1]; loc3[3 * k + 2] = loc[2]; }
        if (uv2) { uv2[2 * k] = uv[0]; uv2[2 * k + 1] = uv[1]; }
    }
}

// one ray, start to end, on one lane (the host simulation; the kernel runs the first walk as a wave loop).
// stack_entries: 1 .. TR_CROSS_STACK, 0 = all of them.  Returns the number of crossings (FILL: min(it, acc.limit) rows are
// written and still in walk order); *lost (may be null): the first walk overflowed its stack.
template <int MODE>
TR_HD int32_t tr_cross_query(const tr_bvh_view& b, float ox, float oy, float oz, float dx, float dy, float dz, float tmin, float tmax,
                             const tr_ring stack, int stack_entries, tr_cross_acc& acc, uint8_t* lost) {
    tr_ray r;
    float lo, hi;
    bool valid = tr_ray_setup(r, ox, oy, oz, dx, dy, dz);
    valid = tr_range_bounds(tmin, tmax, lo, hi) && valid && b.num_tris > 0;
    acc.count = 0;
    if (lost) *lost = 0;
    if (valid && b.num_tris >= 2 && !tr_cross_full<MODE>(acc)) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_CROSS_STACK);
        tr_cross_state st;
        st.node = 0; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
        while (st.node >= 0) tr_cross_visit<MODE>(b, r, lo, hi, st, acc, stack, cap2);
        if (lost) *lost = tr_walk_lost(st.sp) ? 1 : 0;
        if (tr_walk_lost(st.sp) && !tr_cross_full<MODE>(acc)) {
            acc.count = 0;
            tr_rewalk(b, tr_cross_probe<MODE>{b, r, lo, hi, acc});
        }
    } else if (valid && !tr_cross_full<MODE>(acc)) {
        tr_counters* nc = nullptr;
        const tr_tri w = tr_load_tri<false, false>(b, 0, nc);      // no hierarchy below two triangles
        float tt;
        if (tr_range_tri(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, lo, hi, tt)) tr_cross_record<MODE>(acc, w.face, tt, 0);
    }
    return acc.count;
}
