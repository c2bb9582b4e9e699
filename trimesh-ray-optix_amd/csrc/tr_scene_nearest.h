// tr_scene_nearest.h -- closest_point over INSTANCES (include/triro_scene_nearest.h): the nearest placed triangle of a scene
// (tr_scene.h: placed copies of several meshes) to a world point, and which copy it belongs to.  Host + device, as tr_scene.h
// and tr_nearest.h: k_scene_closest_point (scene_nearest.hip) runs these functions with each instance's walk as a wave loop,
// tests/host_sim/scene_nearest_sim.cpp compiles the very same functions with g++.  Not a CPU fallback: nothing in the C ABI
// reaches the host instantiation.
//
// WHY THE RAY TRICK DOES NOT CARRY OVER, AND WHAT DOES.  A ray query transforms the QUERY into the member's frame and compares
// ray parameters there (tr_scene.h): an affine map preserves them.  It does not preserve distances, so a point query cannot do
// that.  This one walks the member's hierarchy in OBJECT space and places what it meets -- child boxes and triangles -- into
// WORLD space with the one chain the scene already has (tr_scene_point with rec.M, the chain that produces `loc`), and measures
// there with the per-triangle function, the box bound and the activity rule of tr_nearest.h, UNCHANGED.
//
// THE CONTRACT.  World point p (three float32), max_distance (float32, per point or one for all), the committed scene.
//  1. PLACED TRIANGLES.  For a valid instance k (TR_SCENE_VALID of the committed table, as tr_scene.h defines it) the placed
//     vertices of a member triangle are tr_scene_point(rec.M, v) of its three float32 vertices: float32 values, three fmaf
//     each, in the order written there.  A placed triangle is ACTIVE iff all nine placed coordinates are finite
//     (tr_near_active on the placed values).  A member triangle with a non-finite coordinate places to a non-finite one (an
//     fmaf passes NaN on, and Inf times a finite entry is Inf or NaN), and a finite one whose placed coordinates overflow is
//     inactive just the same: neither offers a candidate.  An invalid instance and a member without triangles offer none.
//  2. DISTANCE.  d2(p, k, f) = tr_near_tri(p, placed a, placed b, placed c).d2: the float64 sequence of tr_nearest.h on the
//     float32 placed vertices.  Nothing new is evaluated.
//  3. WINNER.  The lexicographic minimum of (d2, instance, face) over the active placed triangles with d2 <= R2, where
//     R2 = tr_within_r2(max_distance).  +Inf: unbounded.  A NaN or negative max_distance accepts nothing (tr_within_valid, as
//     tr_within_closest).  A triangle at exactly max_distance is within.
//  4. OUTPUTS.  instance and tri name the winner, tri being the face index in the member mesh; closest = the float64 closest
//     point on the placed triangle, each component rounded to float32 (world space); distance = tr_near_distance(d2).  A point
//     with a non-finite component, an empty scene, or no accepted candidate: instance -1, tri -1, distance +Inf, closest NaN.
//     Every element of every output given is written.
//  5. PURITY.  A pure function of (p, max_distance, instances, member triangles): independent of the order in which nodes or
//     instances are visited, of stack capacity and of launch shape.
//
// TWO IDENTITIES.
//  * BAKED MESH.  Let the baked mesh concatenate, in instance order, the faces of every valid instance with vertices placed by
//    the same chain in float32.  The scene's answer equals tr_closest_point on the baked mesh, bit for bit in closest, distance
//    and triangle, (instance, tri) mapping to the baked face index by the instance offsets: both are the minimum of
//    (tr_near_tri.d2, index) over the same float32 triangles, and (instance, face) orders as the baked index does.  With a
//    bounded max_distance the same holds against tr_within_closest.  This is the oracle (tests/host_sim/scene_nearest_sim.py
//    bakes and calls nearest_sim's brute force).
//  * IDENTITY PLACEMENT.  One instance at the identity is tr_closest_point of that mesh, for meshes without a negative-zero
//    coordinate: fmaf(1, x, +0) turns -0 into +0 (tr_scene.h, NEGATIVE ZEROS), which can change the sign of a zero in `closest`.
//
// THE BOUND (culling), AND WHY IT NEEDS NO MARGIN.  Write chain_i(x, y, z) = fmaf(M[i][0], x, fmaf(M[i][1], y, fmaf(M[i][2], z,
// M[i][3]))), the placed coordinate i of tr_scene_point.
//  (a) Rounding to nearest is monotone (non-decreasing) on the extended reals.  So fl(a x + c), one fmaf, is non-decreasing in
//      c, and in x it is non-decreasing for a >= 0 (-0 included: the product is a zero) and non-increasing for a < 0.
//  (b) chain_i is a composition of three such steps, the inner result entering the next as c: it is monotone in each of x, y,
//      z separately, with the direction given by the sign of M[i][j].
//  (c) For a child box [lo, hi] of the member's hierarchy let LO_i = chain_i at the corner that takes lo_j where M[i][j] >= 0
//      and hi_j otherwise, and HI_i = chain_i at the opposite corner (tr_scene_near_place; the choice is kept per entry as a
//      bit mask, tr_scene_near_map).  Moving a vertex v with lo_j <= v_j <= hi_j one coordinate at a time to those corners
//      never increases, respectively never decreases, the result, by (b): LO_i <= chain_i(v) <= HI_i for the ROUNDED placed
//      coordinates, exactly, with no pad.
//  (d) NaN.  With finite M and finite corners the chain cannot produce NaN: the product inside an fmaf is exact, so the only
//      sum is (finite real) + (finite or infinite c), and Inf - Inf does not arise; an overflow gives +-Inf, which (a) covers.
//      A corner that is itself non-finite can: the builder boxes a leaf by tr_tri_box, whose fminf / fmaxf skip a NaN
//      coordinate and whose pad turns an infinite minimum into Inf - Inf = NaN, and a parent's box is the fminf / fmaxf union of
//      its children's, so boxes above inactive triangles hold NaN, -Inf or +Inf.  An infinite corner against a zero entry of M
//      is 0 x Inf = NaN, against a c that is infinite with the other sign Inf - Inf = NaN.  An fmaf passes a NaN on, so any NaN met on the
//      way is still there in LO_i or HI_i.  THE RULE: a bound that is not proven never culls -- a NaN among the six values gives
//      the bound 0 (tr_scene_near_bound), the smallest there is.  (tr_near_box alone would not do: of `lo - p` and `p - hi` it
//      keeps the one that is not NaN, which is no bound of anything when the other corner was not proven.)  Infinite values
//      without a NaN are ordinary members of the extended reals: (c) holds for them.
//  (e) What (c) is needed for: every ACTIVE placed triangle below the box has its placed vertices -- finite, so images of
//      finite member vertices, which the box contains (a node's box contains its triangles' vertices; the leaf box in a
//      parent is the padded tr_tri_box, a superset) -- in [LO, HI] per axis.  Inactive triangles below offer no candidate
//      and need no bound.
//  (f) From here THE BOUND of tr_nearest.h carries over word for word: every candidate q of a placed triangle is clamped, per
//      axis, into the coordinate range of its three placed vertices, inside [LO_i, HI_i]; so |fl(p_i - q_i)| >= g_i =
//      max(fl(LO_i - p_i), fl(p_i - HI_i), 0) exactly, and tr_near_len2 is monotone in every argument:
//      tr_near_box(p, LO, HI) <= the COMPUTED d2 of every active placed triangle below.  A subtree is skipped only on
//      bound > best, STRICTLY: culling can lose neither the winner nor a tie.
//  Cost per child box: 18 float32 fmaf and 18 bit selects; the masks depend on the instance alone (wave-uniform).
//
// CARRYING THE BEST BETWEEN INSTANCES (the pattern of tr_scene_seed / tr_scene_take).  G = (d2, instance, face) is the best of
// the instances visited so far, seeded with (R2, INT_MAX, INT_MAX) and no slot.  Instance k is walked with the per-instance
// state B = {d2 = G.d2, face = k < G.instance ? INT_MAX : -1, slot = -1} (tr_scene_near_seed_best) and the comparison of
// tr_near_leaf, (d2, face) lexicographic: with face = -1 a triangle at exactly G.d2 never enters -- instance k > G.instance
// loses that tie by rule 3 -- and with face = INT_MAX (the first instance, and an earlier instance visited later) it does, as
// rule 3 wants; the strict culling keeps it.  After the instance, B.slot >= 0 means B holds the instance's best among those
// that could beat G, and tr_scene_near_take compares (B.d2, k, B.face) with G EXPLICITLY, lexicographically.  Nothing depends on
// the visiting order: G after all instances is the minimum of rule 3.
//
// THE WALK of an instance is tr_nearest.h's with the placed bound and placed leaves: the seed descent (tr_scene_near_seed) only
// while the lane's best is still +Inf -- after the first instance, or under a bounded max_distance, the best is finite and the
// walk culls from its first node -- then tr_scene_near_visit from the member's root, whose first visit tests the placed boxes
// of the root's children against G: that is the cull of an instance.  The {node, float32 bound rounded down} entries, the push
// and the pop are tr_near_push / tr_near_pop as they are.  A lane whose stack overflowed IN THAT INSTANCE walks it again without
// a stack (tr_rewalk on a tr_scene_near_probe) before the next instance is begun.  Below two triangles the one triangle is tested directly.
// The loop over instances is linear: there is no structure over them.
#pragma once
#include "tr_scene.h"
#include "tr_within.h"

// G: the best of the instances visited so far
struct tr_scene_near_best {
    double d2;        // R2 until something is accepted
    int32_t inst;     // 0x7fffffff: none
    int32_t face;
    int32_t slot;     // slot in the member's `tris` (-1: none)
};

TR_HD void tr_scene_near_init(tr_scene_near_best& g, double R2) { g.d2 = R2; g.inst = 0x7fffffff; g.face = 0x7fffffff; g.slot = -1; }

// the query can accept something: a finite point and a max_distance that is not NaN and not negative
TR_HD bool tr_scene_near_valid(float px, float py, float pz, float max_distance) { return tr_within_valid(px, py, pz, max_distance); }

// the per-instance state of instance k, seeded from the best so far (see CARRYING THE BEST)
TR_HD void tr_scene_near_seed_best(const tr_scene_near_best& g, int32_t k, tr_near_best& b) {
    b.d2 = g.d2;
    b.face = k < g.inst ? 0x7fffffff : -1;
    b.slot = -1;
}
// what instance k found against the best so far: (d2, instance, face) lexicographic, explicitly
TR_HD void tr_scene_near_take(const tr_near_best& b, int32_t k, tr_scene_near_best& g) {
    if (b.slot < 0) return;
    const bool closer = b.d2 < g.d2 || (b.d2 == g.d2 && (k < g.inst || (k == g.inst && b.face < g.face)));
    if (closer) { g.d2 = b.d2; g.inst = k; g.face = b.face; g.slot = b.slot; }
}

// a placement as the walk holds it: M (3 x 4 row-major, object -> world) and, per entry of its linear part, the corner choice of
// THE BOUND (c) as a bit mask: hi[3 i + j] = 0 where M[i][j] >= 0 (LO_i takes lo_j), all ones otherwise (LO_i takes hi_j).
// Masks, not conditions: on the device the twenty-one words are wave-uniform and live in SGPRs, one each.
struct tr_scene_near_map {
    float M[12];
    uint32_t hi[9];
};
TR_HD void tr_scene_near_map_make(const float* M, tr_scene_near_map& A) {
    for (int k = 0; k < 12; k++) A.M[k] = M[k];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) A.hi[3 * i + j] = M[4 * i + j] >= 0.0f ? 0u : 0xffffffffu;
}
// b where the mask is set, a where it is clear (bit for bit: a NaN or an infinity passes through unchanged)
TR_HD float tr_scene_near_pick(uint32_t mask, float a, float b) { return tr_u2f((tr_f2u(a) & ~mask) | (tr_f2u(b) & mask)); }

// THE BOUND (c): the object-space box [lo, hi] placed by A -> LO[3], HI[3]
TR_HD void tr_scene_near_place(const tr_scene_near_map& A, float lox, float loy, float loz, float hix, float hiy, float hiz, float* LO,
                               float* HI) {
    for (int i = 0; i < 3; i++) {
        const float* r = A.M + 4 * i;
        const uint32_t* m = A.hi + 3 * i;
        LO[i] = fmaf(r[0], tr_scene_near_pick(m[0], lox, hix),
                     fmaf(r[1], tr_scene_near_pick(m[1], loy, hiy), fmaf(r[2], tr_scene_near_pick(m[2], loz, hiz), r[3])));
        HI[i] = fmaf(r[0], tr_scene_near_pick(m[0], hix, lox),
                     fmaf(r[1], tr_scene_near_pick(m[1], hiy, loy), fmaf(r[2], tr_scene_near_pick(m[2], hiz, loz), r[3])));
    }
}
// lower bound of the COMPUTED d2 of every active placed triangle whose member vertices lie in the box; 0 where not proven (d)
TR_HD double tr_scene_near_bound(const tr_scene_near_map& A, float px, float py, float pz, float lox, float loy, float loz, float hix, float hiy,
                                 float hiz) {
    float LO[3], HI[3];
    tr_scene_near_place(A, lox, loy, loz, hix, hiy, hiz, LO, HI);
    const bool proven = LO[0] == LO[0] && LO[1] == LO[1] && LO[2] == LO[2] && HI[0] == HI[0] && HI[1] == HI[1] && HI[2] == HI[2];
    const double lb = tr_near_box(px, py, pz, LO[0], LO[1], LO[2], HI[0], HI[1], HI[2]);
    return proven ? lb : 0.0;
}

// the placed vertices of the triangle in `slot` (contract 1)
struct tr_scene_near_tri { float ax, ay, az, bx, by, bz, cx, cy, cz; int32_t face; };
TR_HD tr_scene_near_tri tr_scene_near_load_tri(const tr_bvh_view& b, const float* M, int32_t slot) {
    tr_counters* nc = nullptr;
    const tr_tri t = tr_load_tri<false, false>(b, slot, nc);
    tr_scene_near_tri w;
    tr_scene_point(M, t.ax, t.ay, t.az, w.ax, w.ay, w.az);
    tr_scene_point(M, t.bx, t.by, t.bz, w.bx, w.by, w.bz);
    tr_scene_point(M, t.cx, t.cy, t.cz, w.cx, w.cy, w.cz);
    w.face = t.face;
    return w;
}
// one placed triangle against the instance's best: (d2, face) lexicographic, an inactive one changes nothing (tr_near_leaf)
TR_HD void tr_scene_near_leaf(const tr_bvh_view& b, const tr_scene_near_map& A, int32_t slot, float px, float py, float pz, tr_near_best& best) {
    const tr_scene_near_tri w = tr_scene_near_load_tri(b, A.M, slot);
    const tr_near_pt c = tr_near_tri(px, py, pz, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz);
    const bool active = tr_near_active(w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz);
    if (active && (c.d2 < best.d2 || (c.d2 == best.d2 && w.face < best.face))) { best.d2 = c.d2; best.face = w.face; best.slot = slot; }
}

// both placed child bounds and child ids of an internal node (tr_near_load)
TR_HD tr_near_node tr_scene_near_load(const tr_bvh_view& b, const tr_scene_near_map& A, int32_t node, float px, float py, float pz) {
    const tr_f4* q = reinterpret_cast<const tr_f4*>(b.nodes + node);
    const tr_f4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];      // lo.x lo.y lo.z hi.z | hi.x hi.y lo.x lo.y | lo.z hi.z hi.x hi.y | c0 c1 ..
    tr_near_node r;
    r.lb0 = tr_scene_near_bound(A, px, py, pz, n0.x, n0.y, n0.z, n1.x, n1.y, n0.w);
    r.lb1 = tr_scene_near_bound(A, px, py, pz, n1.z, n1.w, n2.x, n2.z, n2.w, n2.y);
    r.c0 = (int32_t)tr_f2u(n3.x); r.c1 = (int32_t)tr_f2u(n3.y);
    return r;
}

// visit st.node (>= 0): tr_near_visit with the placed bound and placed leaves
TR_HD void tr_scene_near_visit(const tr_bvh_view& b, const tr_scene_near_map& A, float px, float py, float pz, tr_near_state& st, tr_near_best& best,
                               const tr_ring stack, uint32_t cap2) {
    const tr_near_node n = tr_scene_near_load(b, A, st.node, px, py, pz);
    const bool swap = n.lb1 < n.lb0;
    const int32_t cn = swap ? n.c1 : n.c0, cf = swap ? n.c0 : n.c1;
    const double ln = swap ? n.lb1 : n.lb0, lf = swap ? n.lb0 : n.lb1;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int32_t c = k ? cf : cn;
        const double lb = k ? lf : ln;
        if (c < 0 && !(lb > best.d2)) tr_scene_near_leaf(b, A, ~c, px, py, pz, best);
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

// the seed descent, one node per call (tr_near_seed): to the child with the smaller placed bound, down to one leaf
TR_HD int32_t tr_scene_near_seed(const tr_bvh_view& b, const tr_scene_near_map& A, int32_t node, float px, float py, float pz, tr_near_best& best) {
    const tr_near_node n = tr_scene_near_load(b, A, node, px, py, pz);
    const int32_t c = n.lb1 < n.lb0 ? n.c1 : n.c0;
    if (c >= 0) return c;
    tr_scene_near_leaf(b, A, ~c, px, py, pz, best);
    return -1;
}

// the whole member again without a stack (after a lost push): tr_near_probe with the placed bound and placed leaves
struct tr_scene_near_probe {
    const tr_bvh_view& b;
    const tr_scene_near_map& A;
    float px, py, pz;
    tr_near_best& best;
    TR_HDM bool done() const { return false; }
    TR_HDM bool child(int32_t node, int phase, int32_t& c) const {
        const tr_near_node n = tr_scene_near_load(b, A, node, px, py, pz);
        c = phase ? n.c1 : n.c0;
        return !((phase ? n.lb1 : n.lb0) > best.d2);
    }
    TR_HDM void leaf(int32_t slot) const { tr_scene_near_leaf(b, A, slot, px, py, pz, best); }
};

// the four outputs of a point from the best placed triangle (valid: the query can accept something; g.slot < 0: nothing was
// accepted).  Any of the pointers may be null.
TR_HD void tr_scene_near_outputs(const tr_scene_member* members, const tr_scene_inst* insts, float px, float py, float pz, bool valid,
                                 const tr_scene_near_best& g, float* closest3, float* distance, int32_t* inst, int32_t* tri) {
    float qx = tr_u2f(0x7fc00000u), qy = qx, qz = qx, d = INFINITY;
    int32_t face = -1, in = -1;
    if (valid && g.slot >= 0) {
        const tr_scene_inst& rec = insts[g.inst];
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        const tr_scene_near_tri w = tr_scene_near_load_tri(b, rec.M, g.slot);
        const tr_near_pt c = tr_near_tri(px, py, pz, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz);
        qx = (float)c.x; qy = (float)c.y; qz = (float)c.z;
        d = tr_near_distance(c.d2);
        face = w.face; in = g.inst;
    }
    if (closest3) { closest3[0] = qx; closest3[1] = qy; closest3[2] = qz; }
    if (distance) *distance = d;
    if (inst) *inst = in;
    if (tri) *tri = face;
}

// one instance on one lane (the host simulation; the kernel runs the seed descent and the first walk as wave loops).
// *lost (may be null) is set when the first walk overflowed its stack.
TR_HD void tr_scene_near_instance(const tr_bvh_view& b, const tr_scene_near_map& A, float px, float py, float pz, const tr_ring stack, uint32_t cap2,
                                  tr_near_best& best, uint8_t* lost) {
    if (b.num_tris >= 2) {
        if (best.d2 == INFINITY)
            for (int32_t node = 0; node >= 0;) node = tr_scene_near_seed(b, A, node, px, py, pz, best);
        tr_near_state st;
        st.node = 0; st.sp = 0;
        while (st.node >= 0) tr_scene_near_visit(b, A, px, py, pz, st, best, stack, cap2);
        if (tr_near_lost(st.sp)) {
            if (lost) *lost = 1;
            tr_rewalk(b, tr_scene_near_probe{b, A, px, py, pz, best});
        }
    } else {
        tr_scene_near_leaf(b, A, 0, px, py, pz, best);      // no hierarchy below two triangles
    }
}

// one world point, start to end, on one lane.  order (may be null): the order in which the instances are visited, a
// permutation of 0 .. ninst - 1 (null: ascending).  stack_entries: 1 .. TR_NEAR_STACK, 0 = all of them.  lost (may be null):
// some instance's first walk overflowed its stack.
TR_HD void tr_scene_near_query(const tr_scene_member* members, const tr_scene_inst* insts, int32_t ninst, const int32_t* order, float px,
                               float py, float pz, float max_distance, const tr_ring stack, int stack_entries, float* closest3,
                               float* distance, int32_t* inst, int32_t* tri, uint8_t* lost) {
    const bool valid = tr_scene_near_valid(px, py, pz, max_distance);
    tr_scene_near_best g;
    tr_scene_near_init(g, tr_within_r2(max_distance));
    if (lost) *lost = 0;
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
    for (int32_t j = 0; valid && j < ninst; j++) {
        const int32_t k = order ? order[j] : j;
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        tr_near_best best;
        tr_scene_near_seed_best(g, k, best);
        tr_scene_near_map A;
        tr_scene_near_map_make(rec.M, A);
        tr_scene_near_instance(b, A, px, py, pz, stack, cap2, best, lost);
        tr_scene_near_take(best, k, g);
    }
    tr_scene_near_outputs(members, insts, px, py, pz, valid, g, closest3, distance, inst, tri);
}
