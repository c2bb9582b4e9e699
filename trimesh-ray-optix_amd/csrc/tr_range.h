// tr_range.h -- ray queries on a per-ray interval [tmin, tmax] (include/triro_range.h): is anything hit within the
// interval (any), and what is the first hit within it (closest).  Host + device, as tr_nearest.h: k_range_query
// (range.hip) runs these functions as wave loops, tests/host_sim/range_sim.cpp compiles the very same functions with g++.
// Not a CPU fallback: nothing in the C ABI reaches the host instantiation.
//
// THE CONTRACT.  A ray is (o, d), six float32; its bounds are lo = tmin[i] (0 where the array is NULL) and hi = tmax[i]
// (TR_TMAX where NULL).  Distances are parametric (P = o + t d), as everywhere in tr_math.h.
//
//  * The ray is set up with tr_ray_setup and is NEVER ANCHORED (tr_ray_anchor): a user's bounds are measured from the
//    user's origin, and an anchored ray measures from the anchor.
//  * INVALID rays miss everything and still get every output written: tr_ray_setup returns false (a non-finite component),
//    or lo or hi is NaN.
//  * Otherwise lo' = max(lo, 0) and hi' = min(hi, TR_TMAX) (tr_range_bounds); lo' > hi' is an EMPTY range: a miss.
//    A negative tmin is 0, tmax = +Inf is TR_TMAX; the interval is CLOSED: a hit at exactly lo' or hi' counts.
//
//  * THE PER-TRIANGLE PREDICATE (tr_range_tri; the walk runs its two halves apart: tr_range_fast, tr_range_drain) is a pure
//    function of (ray, triangle, lo', hi'):
//      c = tr_tri_fast(ray, triangle): TR_MISS is a miss.
//      A bound b has a BAND only when it is a real restriction: lo' when lo' > 0, hi' when hi' < TR_TMAX.  t_f is in the
//      band of b when fabsf(t_f - b) <= b * 2^-10, evaluated in float32 (tr_range_in_band).
//      TR_HIT with t_f in no band: accepted iff lo' <= t_f <= hi'; its distance is t_f.
//      TR_UNDECIDED, or TR_HIT with t_f in a band: the float64 part decides -- tr_tri_exact_t, and tr_tie_own on a tie,
//      exactly as tr_tri_exact / tr_drain_exact do it: accepted iff inside and lo' <= t_e <= hi'; its distance is t_e.
//    WHY 2^-10.  tr_tri_fast only returns a distance t_f whose relative error against the exact distance t is proven
//    below 2^-11 (tr_math.h, "the distance of a proven hit": |T| and |det| exceed 2^12 x their error bounds):
//    |t_f - t| <= 2^-11 t.  t_e is the float32 rounding of a float64 quotient of float64 edge functions: within 2^-24 t
//    (and a few 2^-53).  Take t_f outside the band of b, above it: the float32 difference t_f - b is within (1 +- 2^-24) of
//    the real one and b * 2^-10 is exact (a power of two; b >= 2^-116 or the band is empty anyway), so
//    t_f > b (1 + 2^-10 (1 - 2^-24)), hence t >= t_f / (1 + 2^-11) > b (1 + 2^-12) and t_e >= t (1 - 2^-24) > b.  Below it:
//    t_f < b (1 - 2^-10 (1 - 2^-24)), t <= t_f / (1 - 2^-11) < b (1 - 2^-12), t_e < b.  So outside the bands t_f, t_e and
//    the exact t lie on the same side of every restricting bound: WHETHER A HIT LIES IN THE RANGE IS ALWAYS DECIDED AS
//    THE CORRECTLY ROUNDED DISTANCE t_e WOULD DECIDE IT.  The bound of tr_math.h carries the claim with a factor of two to
//    spare; the band is not widened.  (The two ends that are NOT restrictions, 0 and TR_TMAX, are decided as the old
//    contract decides them: by t_f inside tr_tri_fast, by t_e in the float64 part.)
//  * DEFAULTS.  With both bounds at their defaults there is no band, lo' = 0 = TR_TMIN and hi' = TR_TMAX, and on a ray
//    that the old contract does not anchor the predicate IS tr_tri_test: same hits, same distances.
//
//  * RESULTS.  any: some triangle is accepted.  closest: the accepted triangle that minimises (t, original face index)
//    lexicographically (tr_closer); front, uv and loc come from tr_hit_outputs on the winner, t is its distance.  A miss
//    gives what tr_intersects_closest writes (hit 0, front 0, tri -1, loc 0, uv 0) and t = +Inf.  Both are pure functions
//    of (ray, bounds, the set of triangles): independent of traversal order, launch shape and stack capacity, and
//    bit-comparable with a brute force over tr_range_tri.
//
// CULLING.  A box with slab interval (tn, tf) -- tr_node_slabs: tn the entry, tf the exit padded by TR_SLAB_PAD -- is skipped
// only when
//      (a) tr_slab_hit(tn, tf, min(hi', best_t) * TR_CULL_SLACK) fails   (best_t = +Inf before a hit and for any), or
//      (b) tf < lo' * (1 - 2^-9)                                          (tr_range_box).
// Nothing else culls.  NO ACCEPTED HIT IS LOST:
//   (a) is the old contract's test with min(hi', best_t) in place of best_t: an accepted hit has a distance <= hi', a float32
//       one at most 2^-11 beyond the exact one, a box's entry at most 3 u beyond the exact entry (tr_math.h, TR_CULL_SLACK),
//       and a hit that could still win has a distance <= best_t.
//   (b) the exact hit point lies in the triangle (or within float64 rounding of its edge), the triangle inside its padded
//       leaf box (tr_tri_box) and that inside every ancestor's box, so the ray is still inside the box at the exact distance t:
//       exact exit >= t.  The padded exit is >= the exact exit whatever the roundings (TR_SLAB_PAD: tf >= exact exit).  An
//       accepted hit has t_f >= lo' with t >= t_f (1 - 2^-11), or t_e >= lo' with t >= t_e (1 - 2^-24): t >= lo' (1 - 2^-11).
//       Together tf >= lo' (1 - 2^-11), and lo' * (1 - 2^-9) as computed (one rounding) is below that: (b) never fires
//       for the box of an accepted hit.  A NaN in tn or tf (a box with non-finite planes) fails no comparison: kept.
//
// THE WALK is the ordered per-lane-stack walk of tr_nearest.h, turned to rays.  tr_range_visit, one node per call, from
// the root: it reads the exact 64-byte node and tests both child boxes (tr_node_slabs).  Leaf children are tested at once,
// the nearer first (by tn).  Of the internal children that survive the (updated) limit the nearer is visited next and
// the farther is pushed as {node, tn}.  With no child left the stack is popped; a pop drops an entry whose tn is beyond the
// current limit without loading its node.  The stack holds `stack_entries` entries (1 .. TR_RANGE_STACK) in LDS: 8 B x 32 x
// 128 lanes = 32 KB per workgroup.  A push that does not fit is dropped and sets the sticky `lost` bit of st.sp; a lane that
// ends with it walks the whole tree again without a stack (tr_rewalk on a tr_range_probe: children in fixed order, up through the
// parent links, tr_link), culling against what it has.  Same bits: the minimum is lexicographic and any is a
// disjunction.  An any-ray stops at its first accepted hit.  Below two triangles there is no hierarchy: the one triangle
// is tested directly.
// REGISTERS.  The float64 part stays out of the leaf test: a test that needs it parks its slot (st.pe0 / st.pe1, one per
// child) and tr_range_drain decides it at the END of the visit, through the real calls tr_tri_exact_t / tr_tie_own, where
// the node record and the triangle are dead -- as tr_fold_leaf / tr_drain_exact do, and for the reason given there.
// Until then the candidate culls nothing, which changes no result.
#pragma once
#include "tr_walk.h"

#define TR_RANGE_STACK 32                    // entries of {node, tn} per lane
#define TR_RANGE_BAND 9.765625e-4f           // 2^-10: half-width of a bound's band, relative
#define TR_RANGE_LO_CUT 0.998046875f         // 1 - 2^-9: a box is skipped when it ends before lo' times this

struct tr_range_best {
    float t;         // distance of the best accepted hit so far (+Inf: none)
    int32_t face;    // its original face index (0x7fffffff: none)
    int32_t slot;    // its slot in `tris` (-1: none)
};
struct tr_range_state {
    int32_t node;    // next internal node to visit, -1 = nothing left
    uint32_t sp;     // 2 * entries in use | lost
    int32_t pe0, pe1;   // leaf tests waiting for the float64 part (tri slots, -1 = none): nearer / farther child
};

TR_HD void tr_range_init(tr_range_best& best) { best.t = INFINITY; best.face = 0x7fffffff; best.slot = -1; }
TR_HD bool tr_range_lost(uint32_t sp) { return (sp & 1u) != 0; }

// (lo, hi) as given -> (lo', hi'); false: a NaN bound or an empty range (the ray misses everything)
TR_HD bool tr_range_bounds(float lo, float hi, float& lo2, float& hi2) {
    const bool nan = (lo != lo) | (hi != hi);
    lo2 = lo > 0.0f ? lo : 0.0f;
    hi2 = hi < TR_TMAX ? hi : TR_TMAX;
    return !nan && lo2 <= hi2;
}
// is t within the band of a bound that is a real restriction?
TR_HD bool tr_range_in_band(float t, float lo, float hi) {
    const bool bl = lo > 0.0f && fabsf(t - lo) <= lo * TR_RANGE_BAND;
    const bool bh = hi < TR_TMAX && fabsf(t - hi) <= hi * TR_RANGE_BAND;
    return bl | bh;
}

// the float32 half of the predicate: TR_MISS, TR_HIT (accepted, distance t) or TR_UNDECIDED (the float64 half decides).
// E = tr_tri_scale of the triangle.
TR_HD int tr_range_fast(const tr_ray& r, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                        float E, float lo, float hi, float& t) {
    tr_hit h;
    h.t = 0.f;
    int c = tr_tri_fast(r, ax, ay, az, bx, by, bz, cx, cy, cz, E, h);
    if (c == TR_HIT) {
        if (tr_range_in_band(h.t, lo, hi)) c = TR_UNDECIDED;
        else if (!(lo <= h.t && h.t <= hi)) c = TR_MISS;
    }
    t = h.t;
    return c;
}
// the float64 half: tr_tri_exact with [lo, hi] in place of [TR_TMIN, TR_TMAX]
TR_HD bool tr_range_exact(const tr_ray& r, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                          float lo, float hi, float& t) {
    const tr_exact_res e = tr_tri_exact_t(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, ax, ay, az, bx, by, bz, cx, cy, cz);
    float tt = e.t;
    if (__builtin_expect(e.tie != 0, 0)) {
        if (!tr_tie_own(r.dx, r.dy, r.dz, ax, ay, az, bx, by, bz, cx, cy, cz, e.tie)) tt = -1.0f;
    }
    t = tt;
    return tt >= lo && tt <= hi;      // (lo >= 0: the -1 of "outside" is never accepted)
}
// the whole predicate in one call (brute force, meshes without a hierarchy)
TR_HD bool tr_range_tri(const tr_ray& r, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                        float lo, float hi, float& t) {
    const int c = tr_range_fast(r, ax, ay, az, bx, by, bz, cx, cy, cz, tr_tri_scale(ax, ay, az, bx, by, bz, cx, cy, cz), lo, hi, t);
    if (c != TR_UNDECIDED) return c == TR_HIT;
    return tr_range_exact(r, ax, ay, az, bx, by, bz, cx, cy, cz, lo, hi, t);
}

// one accepted hit against the best so far: (t, face) lexicographic
TR_HD void tr_range_fold(float t, int32_t face, int32_t slot, tr_range_best& best) {
    if (tr_closer(t, face, best.t, best.face)) { best.t = t; best.face = face; best.slot = slot; }
}

// the limit a box's entry distance is culled against, and the box test (see CULLING)
TR_HD float tr_range_limit(float hi, const tr_range_best& best) { return fminf(hi, best.t) * TR_CULL_SLACK; }
TR_HD bool tr_range_box(float tn, float tf, float lim, float cut) { return tr_slab_hit(tn, tf, lim) && !(tf < cut); }

// the leaf test of the walk: the float32 half here; a test it leaves to the float64 half is parked in `pe`
TR_HD void tr_range_leaf(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, int32_t slot, tr_range_best& best, int32_t& pe) {
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    float tt;
    const int c = tr_range_fast(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, t.esum, lo, hi, tt);
    if (c == TR_UNDECIDED) pe = slot;
    if (c == TR_HIT) tr_range_fold(tt, t.face, slot, best);
}
// decide a parked test (tr_range_exact's sequence; cold: wave-uniform skip when no lane has one, and the triangle is fetched
// again for the tie question instead of living through the call: tr_drain_exact has the measurements)
TR_HD void tr_range_drain(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, int32_t& pe, tr_range_best& best) {
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
            if (tt >= lo && tt <= hi) tr_range_fold(tt, t.face, pe, best);
            pe = -1;
        }
    }
}

// Far-child stack: entry e of a lane is the words 2 e (node) and 2 e + 1 (tn, float32 bits) of its column of a tr_ring
// (tr_nearest.h has the same layout).  cap2 = 2 * entries the walk may use.
TR_HD void tr_range_push(const tr_ring stack, uint32_t cap2, uint32_t& sp, int32_t node, float tn) {
    const uint32_t w = sp & ~1u;
    if (w < cap2) {
        tr_ring_put(stack, w, node);
        tr_ring_put(stack, w + 1u, (int32_t)tr_f2u(tn));
        sp += 2u;
    } else {
        sp |= 1u;
    }
}
// the next entry whose entry distance is not beyond the limit; -1: the stack is empty
TR_HD int32_t tr_range_pop(const tr_ring stack, uint32_t& sp, float lim) {
    while (sp >= 2u) {
        sp -= 2u;
        const uint32_t w = sp & ~1u;
        const float tn = tr_u2f((uint32_t)tr_ring_get(stack, w + 1u));
        if (!(tn > lim)) return tr_ring_get(stack, w);
    }
    return -1;
}

// visit st.node (>= 0): see THE WALK.  Q: TR_Q_ANY or TR_Q_CLOSEST.
template <int Q>
TR_HD void tr_range_visit(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, tr_range_state& st, tr_range_best& best,
                          const tr_ring stack, uint32_t cap2) {
    const tr_f4* q = reinterpret_cast<const tr_f4*>(b.nodes + st.node);
    const tr_f4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];
    float tn0, tf0, tn1, tf1;
    tr_node_slabs(r, n0, n1, n2, tn0, tf0, tn1, tf1);
    const int32_t c0 = (int32_t)tr_f2u(n3.x), c1 = (int32_t)tr_f2u(n3.y);
    const float cut = lo * TR_RANGE_LO_CUT;
    const bool swap = tn1 < tn0;
    const int32_t cn = swap ? c1 : c0, cf = swap ? c0 : c1;
    const float tnn = swap ? tn1 : tn0, tfn = swap ? tf1 : tf0;
    const float tnf = swap ? tn0 : tn1, tff = swap ? tf0 : tf1;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? cf : cn;
        const float tn = k ? tnf : tnn, tf = k ? tff : tfn;
        const bool done = Q == TR_Q_ANY && best.slot >= 0;
        if (c < 0 && !done && tr_range_box(tn, tf, tr_range_limit(hi, best), cut)) {
            int32_t pe = -1;
            tr_range_leaf(b, r, lo, hi, ~c, best, pe);
            if (k) st.pe1 = pe; else st.pe0 = pe;
        }
    }
    const float lim = tr_range_limit(hi, best);
    const bool go_n = cn >= 0 && tr_range_box(tnn, tfn, lim, cut), go_f = cf >= 0 && tr_range_box(tnf, tff, lim, cut);
    if (go_n) {
        if (go_f) tr_range_push(stack, cap2, st.sp, cf, tnf);
        st.node = cn;
    } else if (go_f) {
        st.node = cf;
    } else {
        st.node = tr_range_pop(stack, st.sp, lim);
    }
    // the end of the visit: the float64 half of what the leaf tests parked
    tr_range_drain(b, r, lo, hi, st.pe0, best);
    tr_range_drain(b, r, lo, hi, st.pe1, best);
    if (Q == TR_Q_ANY && best.slot >= 0) st.node = -1;
}

// the whole tree again without a stack (after a lost push): tr_rewalk(b, tr_range_probe<Q>{b, r, lo, hi, best}) -- a child is
// culled as in the walk, a leaf is tested and what it parked decided at once
template <int Q>
struct tr_range_probe {
    const tr_bvh_view& b;
    const tr_ray& r;
    float lo, hi;
    tr_range_best& best;
    TR_HDM bool done() const { return Q == TR_Q_ANY && best.slot >= 0; }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_f4* q = reinterpret_cast<const tr_f4*>(b.nodes + node);
        const tr_f4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];
        float tn0, tf0, tn1, tf1;
        tr_node_slabs(r, n0, n1, n2, tn0, tf0, tn1, tf1);
        c = (int32_t)tr_f2u(phase ? n3.y : n3.x);
        return tr_range_box(phase ? tn1 : tn0, phase ? tf1 : tf0, tr_range_limit(hi, best), lo * TR_RANGE_LO_CUT);
    }
    TR_HDM void leaf(int32_t slot) const {
        int32_t pe = -1;
        tr_range_leaf(b, r, lo, hi, slot, best, pe);
        tr_range_drain(b, r, lo, hi, pe, best);
    }
};

// the outputs of a ray from its best hit (valid = a ray that can hit; best.slot < 0: a miss).  Any pointer may be null.
TR_HD void tr_range_outputs(const tr_bvh_view& b, const tr_ray& r, bool valid, const tr_range_best& best, uint8_t* hit,
                            uint8_t* front, int32_t* tri, float* t, float* loc3, float* uv2) {
    float loc[3] = {0.f, 0.f, 0.f}, uv[2] = {0.f, 0.f}, tt = INFINITY;
    uint8_t h = 0, fr = 0;
    int32_t face = -1;
    if (valid && best.slot >= 0) {
        h = 1; face = best.face; tt = best.t;
        if (front || loc3 || uv2) {
            tr_counters* nc = nullptr;
            const tr_tri w = tr_load_tri<false, false>(b, best.slot, nc);
            fr = tr_hit_outputs(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, loc, uv) ? 1 : 0;
        }
    }
    if (hit) *hit = h;
    if (front) *front = fr;
    if (tri) *tri = face;
    if (t) *t = tt;
    if (loc3) { loc3[0] = loc[0]; loc3[1] = loc[1]; loc3[2] = loc[2]; }
    if (uv2) { uv2[0] = uv[0]; uv2[1] = uv[1]; }
}

// one ray, start to end, on one lane (the host simulation; the kernel runs the first walk as a wave loop).
// stack_entries: 1 .. TR_RANGE_STACK, 0 = all of them.  lost (may be null): the first walk overflowed its stack.
template <int Q>
TR_HD void tr_range_query(const tr_bvh_view& b, float ox, float oy, float oz, float dx, float dy, float dz, float tmin, float tmax,
                          const tr_ring stack, int stack_entries, uint8_t* hit, uint8_t* front, int32_t* tri, float* t,
                          float* loc3, float* uv2, uint8_t* lost) {
    tr_ray r;
    float lo, hi;
    bool valid = tr_ray_setup(r, ox, oy, oz, dx, dy, dz);
    valid = tr_range_bounds(tmin, tmax, lo, hi) && valid && b.num_tris > 0;
    tr_range_best best;
    tr_range_init(best);
    if (lost) *lost = 0;
    if (valid && b.num_tris >= 2) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_RANGE_STACK);
        tr_range_state st;
        st.node = 0; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
        while (st.node >= 0) tr_range_visit<Q>(b, r, lo, hi, st, best, stack, cap2);
        if (lost) *lost = tr_range_lost(st.sp) ? 1 : 0;
        if (tr_range_lost(st.sp)) tr_rewalk(b, tr_range_probe<Q>{b, r, lo, hi, best});
    } else if (valid) {
        tr_counters* nc = nullptr;
        const tr_tri w = tr_load_tri<false, false>(b, 0, nc);      // no hierarchy below two triangles
        float tt;
        if (tr_range_tri(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, lo, hi, tt)) tr_range_fold(tt, w.face, 0, best);
    }
    tr_range_outputs(b, r, valid, best, hit, front, tri, t, loc3, uv2);
}
