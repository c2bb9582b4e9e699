// tr_scene.h -- ray queries over INSTANCES: placed copies of several meshes (include/triro_scene.h).  A scene refers to
// `nmesh` member hierarchies and holds `ninst` instances, each a member index and a placement M (object -> world, 3 x 4
// row-major float32, any invertible affine map: scales and mirrors included).  Host + device, as tr_range.h: k_scene_query
// (scene.hip) runs these functions with the member walk as a wave loop, tests/host_sim/scene_sim.cpp compiles the very same
// functions with g++.  Not a CPU fallback: nothing in the C ABI reaches the host instantiation of the walk (the host
// instantiation of tr_scene_record IS what tr_scene_commit runs: the records are computed on the host).
//
// WHY IT CAN BE EXACT.  An affine map preserves the ray parameter: P = o + t d  =>  W P = (W o) + t (W_lin d).  The hit of a
// world ray on a placed mesh is the hit of the transformed ray on the mesh in its own frame AT THE SAME t, so distances of
// different instances compare without a change of units, and a scene is a minimum over range queries (tr_range.h).
//
// THE CONTRACT.
//  1. THE INVERSE.  W = M^-1 is computed once, at commit, in float64 from the float32 entries of M by the adjugate formula
//     in the order written in tr_scene_record: the nine cofactors c_ij (each  p q - r s, two products and a difference),
//     det = (m00 c00 + m01 c10) + m02 c20, W_lin[i][j] = c_ij / det, W[i][3] = -((w_i0 tx + w_i1 ty) + w_i2 tz) from the
//     float64 quotients; each of the twelve entries is then rounded once to float32.  flip = det < 0 in that arithmetic.
//     (-ffp-contract=off: nothing is fused.)  A signed axis permutation with power-of-two scales and a translation that is
//     representable after scaling has an EXACT inverse: every product and quotient above is exact.
//  2. INVALID INSTANCES are hit by nothing: an entry of M is non-finite, det is zero or non-finite, or an entry of the
//     float32 W is non-finite.  A member without triangles is likewise hit by nothing.
//  3. THE RAY IN AN INSTANCE'S FRAME, the innermost operation last (tr_scene_point / tr_scene_vector; the only fusions):
//        o'x = fmaf(W00, ox, fmaf(W01, oy, fmaf(W02, oz, W03)))        d'x = fmaf(W00, dx, fmaf(W01, dy, W02 * dz))
//     and alike for the rows y and z.
//     NEGATIVE ZEROS.  With M = I this is o' = o and d' = d for every component EXCEPT a negative zero: -0 + +0 = +0, so
//     a -0 component of an origin always comes out as +0, one of a direction does unless every term of its row is -0.  The
//     sign of a zero direction component picks the sign of its clamped reciprocal (tr_inv); no case where that changes an
//     answer is known, but the identity "one instance at I == the range query" is stated and tested for rays without a
//     negative-zero component only.
//  4. VALIDITY.  The world ray is checked with tr_ray_setup and its bounds with tr_range_bounds, ONCE: a ray that fails
//     either misses everything, and every output is still written.  The transformed ray is checked with tr_ray_setup
//     again (a finite ray can leave the float32 range under a large W): one that fails misses THAT INSTANCE only.
//     The bounds are not transformed: lo' and hi' of the world ray are those of every instance.
//  5. THE PER-INSTANCE ANSWER is the range contract -- tr_range_tri and its closest rule (t, original face index) -- for
//     (o', d', lo', hi') on the member's triangles.  The distance of a hit is the distance that contract gives, unchanged.
//  6. THE SCENE'S ANSWER.  any: some instance has an accepted hit.  closest: the accepted hit that minimises
//     (t, instance index, original face index) lexicographically.  instance = its index, tri = its face index IN THE MEMBER
//     MESH, uv as in object space (tr_hit_outputs on (o', d')).  front = the object-space front, inverted where flip: what
//     the placed triangle, in its vertex order, looks like from the ray.  loc = M applied to the object-space loc by the
//     fmaf order of 3.  A miss: hit 0, front 0, instance -1, tri -1, loc 0, uv 0, t = +Inf.
//  7. PURITY.  The answer is a pure function of (ray, bounds, instances, member triangles): independent of traversal
//     order, of the order in which instances are visited, of stack capacity and of launch shape, and bit-comparable with
//     a brute force over tr_range_tri (scene_sim.brute).
//
// CARRYING THE BEST HIT BETWEEN INSTANCES.  G = (t, instance, face) is the best accepted hit of the instances visited so
// far.  Instance k is walked with the per-instance state  B = {t = G.t, face = k < G.instance ? INT_MAX : -1, slot = -1}
// (tr_scene_seed) and THE USER'S lo', hi':
//   * The predicate (tr_range_fast / tr_range_exact inside tr_range_visit) sees the user's hi' only.  Whether a triangle is
//     accepted, and which arithmetic -- float32 or float64 -- produces its distance, is exactly what point 5 says: G.t never
//     becomes a bound with a band of its own.  (Passing min(hi', G.t) as the bound would move a later instance's candidate
//     within 2^-10 of G.t to the float64 distance: other bits than the contract's.  Not done.)
//   * Boxes are culled against min(hi', B.t) * TR_CULL_SLACK = min(hi', G.t) * TR_CULL_SLACK (tr_range_limit).  By (a) of
//     tr_range.h's culling proof no accepted hit with a distance <= G.t is lost: every hit STRICTLY nearer than G.t is found.
//   * An accepted hit enters B through tr_range_fold: it replaces B when t < B.t, or t == B.t and face < B.face.  With the
//     seed's face = -1 (k > G.instance) a hit at exactly G.t never enters: it loses by rule 6, nothing is lost.  With
//     face = INT_MAX (k < G.instance: only when instances are not visited in ascending order) a hit at exactly G.t enters,
//     as rule 6 wants, and culling keeps it: the limit is G.t * (1 + 2^-10), not G.t.  Within the instance B then orders by
//     (t, face) as tr_range.h does.
//   * After the instance, B.slot >= 0 means B holds the instance's best hit among those that could beat G, and
//     tr_scene_take compares (B.t, k, B.face) with G EXPLICITLY, lexicographically.  An earlier instance's hit is never
//     displaced by an equal distance in a later one; nothing depends on the visiting order.
//   So G after all instances is the lexicographic minimum of rule 6, whatever the order and whatever was culled.
//   any: B starts empty for every instance (G is +Inf until the ray's first hit, and the ray is finished by it).
//
// THE WALK of an instance is tr_range.h's: tr_range_visit from the member's root, tr_rewalk (tr_range_probe) for a lane whose stack
// overflowed IN THAT INSTANCE (before the next instance is begun), the one triangle directly below two.  The first visit
// tests the root's two child boxes against the object-space ray with the proven slab test: that is the cull of an instance.
// There is no world-space box and no top-level hierarchy: see DESIGN.md 4.6 for what that would have to prove.
#pragma once
#include "tr_range.h"

#define TR_SCENE_VALID 1      // tr_scene_inst::flags: the instance can be hit (contract 2; the member has triangles)
#define TR_SCENE_FLIP 2       // ... det(M_lin) < 0: front is inverted

// one member of the committed table: the device arrays of a tr_bvh as they were at commit
struct tr_scene_member {
    const tr_node* nodes;
    const tr_link* links;
    const tr_tri* tris;
    int64_t num_tris;
};
// one instance of the committed table
struct alignas(16) tr_scene_inst {
    float W[12];      // world -> object, 3 x 4 row-major
    float M[12];      // object -> world
    int32_t mesh;     // index into the members
    int32_t flags;    // TR_SCENE_VALID | TR_SCENE_FLIP
    int32_t pad[2];
};
static_assert(sizeof(tr_scene_member) == 32 && sizeof(tr_scene_inst) == 112, "layout of the committed table");

struct tr_scene_best {
    float t;          // +Inf: none
    int32_t inst;     // 0x7fffffff: none
    int32_t face;
    int32_t slot;     // slot in the member's `tris` (-1: none)
};

TR_HD void tr_scene_init(tr_scene_best& g) { g.t = INFINITY; g.inst = 0x7fffffff; g.face = 0x7fffffff; g.slot = -1; }

// contract 1 and 2: M (as given) -> the record's W, M and flags (without the member's share of TR_SCENE_VALID)
TR_HD void tr_scene_record(const float* M, tr_scene_inst& rec) {
    const double m00 = M[0], m01 = M[1], m02 = M[2], tx = M[3];
    const double m10 = M[4], m11 = M[5], m12 = M[6], ty = M[7];
    const double m20 = M[8], m21 = M[9], m22 = M[10], tz = M[11];
    const double c00 = m11 * m22 - m12 * m21, c01 = m02 * m21 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c10 = m12 * m20 - m10 * m22, c11 = m00 * m22 - m02 * m20, c12 = m02 * m10 - m00 * m12;
    const double c20 = m10 * m21 - m11 * m20, c21 = m01 * m20 - m00 * m21, c22 = m00 * m11 - m01 * m10;
    const double det = (m00 * c00 + m01 * c10) + m02 * c20;
    const double w00 = c00 / det, w01 = c01 / det, w02 = c02 / det;
    const double w10 = c10 / det, w11 = c11 / det, w12 = c12 / det;
    const double w20 = c20 / det, w21 = c21 / det, w22 = c22 / det;
    const double w03 = -((w00 * tx + w01 * ty) + w02 * tz);
    const double w13 = -((w10 * tx + w11 * ty) + w12 * tz);
    const double w23 = -((w20 * tx + w21 * ty) + w22 * tz);
    const double w[12] = {w00, w01, w02, w03, w10, w11, w12, w13, w20, w21, w22, w23};
    bool ok = det != 0.0 && det - det == 0.0;      // (NaN and +-Inf fail the second)
    for (int k = 0; k < 12; k++) {
        rec.M[k] = M[k];
        rec.W[k] = (float)w[k];
        ok = ok && tr_finite(M[k]) && tr_finite(rec.W[k]);
    }
    rec.flags = (ok ? TR_SCENE_VALID : 0) | (det < 0.0 ? TR_SCENE_FLIP : 0);
    rec.mesh = 0; rec.pad[0] = 0; rec.pad[1] = 0;
}

// contract 3: a point and a vector through a 3 x 4 map
TR_HD void tr_scene_point(const float* A, float x, float y, float z, float& px, float& py, float& pz) {
    px = fmaf(A[0], x, fmaf(A[1], y, fmaf(A[2], z, A[3])));
    py = fmaf(A[4], x, fmaf(A[5], y, fmaf(A[6], z, A[7])));
    pz = fmaf(A[8], x, fmaf(A[9], y, fmaf(A[10], z, A[11])));
}
TR_HD void tr_scene_vector(const float* A, float x, float y, float z, float& vx, float& vy, float& vz) {
    vx = fmaf(A[0], x, fmaf(A[1], y, A[2] * z));
    vy = fmaf(A[4], x, fmaf(A[5], y, A[6] * z));
    vz = fmaf(A[8], x, fmaf(A[9], y, A[10] * z));
}
// the world ray (o, d) in the frame of `rec`; false: the transformed ray has a non-finite component (contract 4)
TR_HD bool tr_scene_ray(const tr_scene_inst& rec, float ox, float oy, float oz, float dx, float dy, float dz, tr_ray& r) {
    float px, py, pz, vx, vy, vz;
    tr_scene_point(rec.W, ox, oy, oz, px, py, pz);
    tr_scene_vector(rec.W, dx, dy, dz, vx, vy, vz);
    return tr_ray_setup(r, px, py, pz, vx, vy, vz);
}

TR_HD tr_bvh_view tr_scene_view(const tr_scene_member& m) {
    tr_bvh_view v;
    v.nodes = m.nodes; v.links = m.links; v.tris = m.tris; v.num_tris = m.num_tris;
    v.qnodes = nullptr; v.frame_dev = nullptr;
    v.frame.base[0] = v.frame.base[1] = v.frame.base[2] = 0.f;
    v.frame.scale[0] = v.frame.scale[1] = v.frame.scale[2] = 1.f;
    return v;
}

// the per-instance state of instance k, seeded from the best so far (see CARRYING THE BEST HIT)
template <int Q>
TR_HD void tr_scene_seed(const tr_scene_best& g, int32_t k, tr_range_best& b) {
    b.t = Q == TR_Q_ANY ? INFINITY : g.t;
    b.face = (Q == TR_Q_ANY || k < g.inst) ? 0x7fffffff : -1;
    b.slot = -1;
}
// what instance k found against the best so far: (t, instance, face) lexicographic, explicitly
TR_HD void tr_scene_take(const tr_range_best& b, int32_t k, tr_scene_best& g) {
    if (b.slot < 0) return;
    const bool closer = b.t < g.t || (b.t == g.t && (k < g.inst || (k == g.inst && b.face < g.face)));
    if (closer) { g.t = b.t; g.inst = k; g.face = b.face; g.slot = b.slot; }
}

// the one triangle of a member without a hierarchy
TR_HD void tr_scene_single(const tr_bvh_view& b, const tr_ray& r, float lo, float hi, tr_range_best& best) {
    tr_counters* nc = nullptr;
    const tr_tri w = tr_load_tri<false, false>(b, 0, nc);
    float tt;
    if (tr_range_tri(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, lo, hi, tt)) tr_range_fold(tt, w.face, 0, best);
}

// the outputs of a world ray from its best hit (valid = a ray that can hit; g.slot < 0: a miss).  Any pointer may be null.
TR_HD void tr_scene_outputs(const tr_scene_member* members, const tr_scene_inst* insts, float ox, float oy, float oz, float dx,
                            float dy, float dz, bool valid, const tr_scene_best& g, uint8_t* hit, uint8_t* front, int32_t* inst,
                            int32_t* tri, float* t, float* loc3, float* uv2) {
    float loc[3] = {0.f, 0.f, 0.f}, uv[2] = {0.f, 0.f}, tt = INFINITY;
    uint8_t h = 0, fr = 0;
    int32_t face = -1, in = -1;
    if (valid && g.slot >= 0) {
        h = 1; face = g.face; in = g.inst; tt = g.t;
        if (front || loc3 || uv2) {
            const tr_scene_inst& rec = insts[g.inst];
            const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
            tr_ray r;
            (void)tr_scene_ray(rec, ox, oy, oz, dx, dy, dz, r);
            tr_counters* nc = nullptr;
            const tr_tri w = tr_load_tri<false, false>(b, g.slot, nc);
            float ol[3];
            const bool f = tr_hit_outputs(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, ol, uv);
            fr = (f != ((rec.flags & TR_SCENE_FLIP) != 0)) ? 1 : 0;
            tr_scene_point(rec.M, ol[0], ol[1], ol[2], loc[0], loc[1], loc[2]);
        }
    }
    if (hit) *hit = h;
    if (front) *front = fr;
    if (inst) *inst = in;
    if (tri) *tri = face;
    if (t) *t = tt;
    if (loc3) { loc3[0] = loc[0]; loc3[1] = loc[1]; loc3[2] = loc[2]; }
    if (uv2) { uv2[0] = uv[0]; uv2[1] = uv[1]; }
}

// one ray, start to end, on one lane (the host simulation; the kernel runs each instance's first walk as a wave loop).
// order (may be null): the order in which the instances are visited, a permutation of 0 .. ninst - 1 (null: ascending).
// stack_entries: 1 .. TR_RANGE_STACK, 0 = all of them.  lost (may be null): some instance's first walk overflowed its stack.
template <int Q>
TR_HD void tr_scene_query(const tr_scene_member* members, const tr_scene_inst* insts, int32_t ninst, const int32_t* order, float ox,
                          float oy, float oz, float dx, float dy, float dz, float tmin, float tmax, const tr_ring stack,
                          int stack_entries, uint8_t* hit, uint8_t* front, int32_t* inst, int32_t* tri, float* t, float* loc3,
                          float* uv2, uint8_t* lost) {
    tr_ray rw;
    float lo, hi;
    bool valid = tr_ray_setup(rw, ox, oy, oz, dx, dy, dz);
    valid = tr_range_bounds(tmin, tmax, lo, hi) && valid;
    tr_scene_best g;
    tr_scene_init(g);
    if (lost) *lost = 0;
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_RANGE_STACK);
    for (int32_t j = 0; valid && j < ninst; j++) {
        if (Q == TR_Q_ANY && g.slot >= 0) break;
        const int32_t k = order ? order[j] : j;
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        tr_ray r;
        if (!tr_scene_ray(rec, ox, oy, oz, dx, dy, dz, r)) continue;
        tr_range_best best;
        tr_scene_seed<Q>(g, k, best);
        if (b.num_tris >= 2) {
            tr_range_state st;
            st.node = 0; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
            while (st.node >= 0) tr_range_visit<Q>(b, r, lo, hi, st, best, stack, cap2);
            if (tr_range_lost(st.sp)) {
                if (lost) *lost = 1;
                tr_rewalk(b, tr_range_probe<Q>{b, r, lo, hi, best});
            }
        } else {
            tr_scene_single(b, r, lo, hi, best);
        }
        tr_scene_take(best, k, g);
    }
    tr_scene_outputs(members, insts, ox, oy, oz, dx, dy, dz, valid, g, hit, front, inst, tri, t, loc3, uv2);
}
