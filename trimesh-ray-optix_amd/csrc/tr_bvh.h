// tr_bvh.h -- traversal-side data layout of the LBVH and the per-ray traversal core.
//
// The core is host+device code on purpose: the HIP kernels (traverse.hip) instantiate it
// per lane, and tests/host_sim compiles the very same functions with g++ to check the
// trail/parent-link state machine against the oracle without a GPU.  It is not a CPU
// fallback: nothing in the C ABI can reach the host instantiation.
//
// Layout in HBM (one arena per mesh, see DESIGN.md "Data layout"):
//   nodes : (F-1) x 64 B   tr_node   both children's boxes + child ids + parent + sibling
//   qnodes: (F-1) x 32 B   tr_qnode  the same boxes on a 16-bit grid + child ids (unordered schedule)
//   links : (F-1) x  8 B   tr_link   {parent, sibling} again, packed 8 per 64-B line, read
//                                    only while backtracking (keeps the climb off the
//                                    64-B node lines)
//   tris  :  F    x 48 B   tr_tri    Morton-ordered copy of the triangle (v0,v1,v2) + the
//                                    original face index
// Child ids: c >= 0 internal node index, c < 0 leaf, slot = ~c into `tris`.
// One triangle per leaf; the leaf box stored in the parent is the triangle's padded box (tr_tri_box).
//
// Traversal is stackless: a 64-bit trail (bit k set = the node at depth k on the current
// path still owes its far child) plus parent/sibling links (Hapala 2011 / Afra &
// Szirmay-Kalos 2014 style backtracking).  The builder guarantees depth <= 64.
#pragma once
#include <type_traits>
#include "tr_math.h"
#include "../../include/triro_hip.h"   // tr_hit_entry

struct alignas(16) tr_f4 {
    float x, y, z, w;
};
struct alignas(16) tr_i4 {
    int32_t x, y, z, w;
};

// Child boxes are stored as {lo.x, lo.y | lo.z, hi.z | hi.x, hi.y}: every aligned pair of
// floats meets the SAME pair of ray constants ((ox,oy) or (oz,oz)), so the slab planes of a
// node are 6 packed subtracts + 6 packed multiplies on the register pairs the 16-byte loads
// produce (tr_node_slabs).
struct alignas(64) tr_node {
    float box0[6];  // child 0: lo.x lo.y lo.z hi.z hi.x hi.y
    float box1[6];  // child 1
    int32_t c0, c1;
    int32_t parent;   // -1 at the root
    int32_t sibling;  // other child of parent (same encoding as c0/c1); root: 0
};
static_assert(sizeof(tr_node) == 64, "node must be 64 B");
TR_HD void tr_node_set_box(float* box, const float* lo, const float* hi) {
    box[0] = lo[0]; box[1] = lo[1]; box[2] = lo[2]; box[3] = hi[2]; box[4] = hi[0]; box[5] = hi[1];
}

struct alignas(8) tr_link {
    int32_t parent, sibling;
};

// ---- second node array for the UNORDERED schedule (count / location): 32-byte nodes -------------
// Both child boxes on a 16-bit grid over the mesh bounds + child ids: two 16-byte loads per visit
// instead of four.  The unordered leaf phase evaluates the full predicate from the triangle's
// vertices anyway (tr_tri_hit), so the grid boxes only have to be SUPERSETS of the exact ones: the
// builder searches, with the very decode the traversal uses, the largest grid plane <= lo and the
// smallest >= hi, and the slab arithmetic on the decoded planes is the contract's -- monotone under
// box inclusion, so nothing the exact tree would visit is culled.  Measured: C4 count 0.93 -> 0.80
// ms, location 1.18 -> 1.0 ms.  The ordered (closest / first / any) trip keeps the exact 64-byte
// nodes: it needs the leaf's exact slab interval from its parent, and the decode (12 cvt + 6 packed
// fma per visit) made every ordered configuration slower (experiments/q32_nodes.patch).
// Grid plane q of axis k lies at fma(q, scale[k], base[k]), q = 0 .. 65535; base = the mesh bounds'
// minimum, scale = a power of two with decode(65535) >= the bounds' maximum: a pure function of
// the bounds (tr_qframe_make), so host and device derive identical frames.
struct tr_qframe {
    float base[3];
    float scale[3];
};
TR_HD float tr_qdecode(uint32_t q, float scale, float base) { return fmaf((float)q, scale, base); }
TR_HD void tr_qframe_make(const float* mn, const float* mx, tr_qframe* f) {
    for (int k = 0; k < 3; k++) {
        const float ext = mx[k] - mn[k];
        int e = 0;
        float s = 1.0f;
        if (ext > 0.f && ext <= 3.0e38f) {
            (void)frexpf(ext / 65535.0f, &e);      // ext/65535 = m * 2^e, m in [0.5, 1)
            s = ldexpf(1.0f, e < -126 ? -126 : e);
        }
        // rounding in the two lines above can leave the last plane just short of the maximum
        for (int it = 0; it < 300 && !(tr_qdecode(65535u, s, mn[k]) >= mx[k]); it++) s *= 2.0f;
        f->base[k] = mn[k];
        f->scale[k] = s;
    }
}
// ---- fused conservative box test (round 5) --------------------------------------------------------------------
// The grid nodes (and the 8-wide nodes, tr_wide.h) only have to be tested CONSERVATIVELY: the leaves are decided by
// the full predicate (tr_tri_hit), whose own slab interval lies inside every ancestor's (monotone under box
// inclusion).  The contract's form of a plane's distance is three roundings deep -- p = fma(q, scale, base),
// (p - o), (..) * inv: a packed fma, a packed add and a packed multiply per pair of planes, 18 of the ~44 VALU
// instructions of a node's box test.  Here the ray carries, per axis, A = scale * k and B = (base - o) * k -+ e, and a
// plane costs ONE fma: t' = fma(q, A, B).  What makes that safe:
//   * k = the contract's reciprocal, its magnitude clamped to kmax = the power of two with kmax * M <= 2^100, M = the
//     position scale of the axis (|base|, |top|, |base - o|, twice the extent): every product stays finite, no
//     inf - inf, no 0 * inf.  Only rays (numerically) parallel to a coordinate plane are clamped.
//   * e >= the largest possible difference between t' and the contract's value for any plane of the mesh's box.
//     With u = 2^-24, T = (p - o) inv exact, P = max |plane|, E = 65536 scale (>= the extent):
//       contract:  p^ = fl(q s + b), d^ = fl(p^ - o), t^ = fl(d^ inv):   |t^ - T|        <= u |inv| (|p| + 2 |p - o|)
//       fused:     bo = fl(b - o), b0 = fl(bo k), B = fl(b0 -+ e), t' = fl(q A + B):
//                                                                        |t' - (T -+ e)| <= u |k| (|p - o| + 3 |b - o|) + 2 u e
//       exit pad:  t^ * (1 + 2^-21), rounded (TR_SLAB_PAD, round 6):     + 9 u |inv| |p - o|
//     and |p - o| <= |b - o| + E:  e >= u |inv| (P + 15 |b - o| + 12 E) for the grid nodes; the 8-wide nodes decode in
//     their own frame (planes up to one extent outside the mesh's box, base_n - o rounded per node):
//     e >= u |inv| (P + 14 |b - o| + 27 E).  e = 1.25 u |k| (P + 15 |b - o| + 27 E) covers both.  Entry planes get
//     -e, exit planes +e (sel_n / sel_f already separate them): t'_entry <= t_entry, t'_exit >= t_exit * TR_SLAB_PAD.
//   * a clamped axis additionally gets -+ 1.1e7 (> TR_TLIM, the largest limit of a box test): with |k| < |inv| the fused
//     distance has the sign of the contract's and a smaller magnitude, so an exit plane behind the origin stays behind,
//     one in front is pushed beyond every limit (it cannot cull), an entry plane in front stays smaller, one behind
//     stays <= 0 -- all that tr_slab_hit(max(tn, 0) <= min(tf, limit <= TR_TLIM)) can see.
//   * M beyond 1e30 (or not finite): the axis is ignored (A = 0, B = -+inf).
// So: tn' <= max(tn, 0) and tf' >= min(tf, TR_TLIM) for the contract's (tn, tf) of the same decoded box -- the fused
// test accepts whatever the contract's test accepts (tests/host_sim checks exactly this over the fuzz corpus), the
// traversal visits a superset of nodes, the leaves decide: results are bit-identical.  In position units the margin
// is ~1.3 float spacings of the coordinates plus 7e-7 of the camera distance: a few hundredths of a grid cell for a
// camera within a few extents of a mesh near the origin.
TR_HD void tr_fuse_axis(float o, float inv, float base, float scale, float& k, float& e, float& A, float& Bn, float& Bf) {
    const float top = fmaf(65535.0f, scale, base);
    const float bo = base - o;
    const float M = fmaxf(fabsf(base), fabsf(top)) + fabsf(bo) + 131072.0f * scale;
    const bool usable = M <= 1.0e30f;                             // (false for NaN, too)
    const uint32_t be = (tr_f2u(M) >> 23) & 0xffu;               // M = m * 2^(be - 127), m in [1, 2)  (be = 0: M < 2^-126)
    const uint32_t ke = 353u - be > 254u ? 254u : 353u - be;      // kmax = 2^(226 - be): kmax * M < 2^100
    const float kmax = tr_u2f(ke << 23);
    const bool clamped = fabsf(inv) > kmax;
    const float kk = clamped ? copysignf(kmax, inv) : inv;
    const float Me = fmaxf(fabsf(base), fabsf(top)) + 15.0f * fabsf(bo) + 1769472.0f * scale;             // P + 15 |b - o| + 27 E
    const float ee = fabsf(kk) * Me * 7.450580596923828e-08f + (clamped ? 1.1e7f : 0.0f) + 1.0e-37f;      // 1.25 * 2^-24
    const float b0 = bo * kk;
    // (selects, no branch: an early return here left the compiler with a stack object for the B pairs)
    k = usable ? kk : 0.0f;
    e = usable ? ee : INFINITY;
    A = usable ? scale * kk : 0.0f;
    Bn = usable ? b0 - ee : -INFINITY;
    Bf = usable ? b0 + ee : INFINITY;
}
TR_HD void tr_ray_fuse(tr_ray& r, const tr_qframe& f) {
    tr_fuse_axis(r.ox, r.ix, f.base[0], f.scale[0], r.kx, r.ex, r.qax, r.qnx, r.qfx);
    tr_fuse_axis(r.oy, r.iy, f.base[1], f.scale[1], r.ky, r.ey, r.qay, r.qny, r.qfy);
    tr_fuse_axis(r.oz, r.iz, f.base[2], f.scale[2], r.kz, r.ez, r.qaz, r.qnz, r.qfz);
    r.qaz2 = r.qaz;
}
// the box a ray is anchored to (tr_ray_anchor, tr_math.h): the grid frame of the mesh, base ... plane 65535
TR_HD void tr_ray_anchor_q(const tr_qframe& f, float& ox, float& oy, float& oz, float dx, float dy, float dz) {
    const float hi[3] = {fmaf(65535.0f, f.scale[0], f.base[0]), fmaf(65535.0f, f.scale[1], f.base[1]), fmaf(65535.0f, f.scale[2], f.base[2])};
    tr_ray_anchor(f.base, hi, ox, oy, oz, dx, dy, dz);
}
// ray set-up of the kernels that walk the exact nodes: anchor, then the constants of tr_math.h
TR_HD bool tr_ray_setup_a(tr_ray& r, const tr_qframe& f, float ox, float oy, float oz, float dx, float dy, float dz) {
    tr_ray_anchor_q(f, ox, oy, oz, dx, dy, dz);
    return tr_ray_setup(r, ox, oy, oz, dx, dy, dz);
}
// ray set-up for the kernels that walk grid nodes / 8-wide nodes
TR_HD bool tr_ray_setup_q(tr_ray& r, const tr_qframe& f, float ox, float oy, float oz, float dx, float dy, float dz) {
    tr_ray_anchor_q(f, ox, oy, oz, dx, dy, dz);
    const bool valid = tr_ray_setup(r, ox, oy, oz, dx, dy, dz);
    tr_ray_fuse(r, f);
    return valid;
}

// largest grid plane <= lo / smallest grid plane >= hi, defined through the traversal's own decode
// (monotone in q); lo >= base and hi <= decode(65535) by construction.  Closed-form estimate plus a
// fix-up walk of a step or two (round 2 ran a 16-step binary search per plane: 12 searches per node
// on every build and refit).
TR_HD uint32_t tr_qestimate(float x, float scale, float base) {
    const float e = (x - base) / scale;          // scale is a power of two: the division is exact
    return !(e > 0.f) ? 0u : (e >= 65535.f ? 65535u : (uint32_t)e);
}
// (the walk is bounded: where ulp(base) >> scale -- a mesh far from the origin relative to its extent, a
// degenerate axis -- thousands of consecutive q decode to the same float and a linear walk would take up to
// 65535 steps per plane, 12 planes per node; after 4 steps the binary search of round 2 takes over.  Same
// result: the largest q with decode(q) <= lo / the smallest with decode(q) >= hi, decode being monotone.)
TR_HD uint32_t tr_qfloor(float lo, float scale, float base) {
    uint32_t q = tr_qestimate(lo, scale, base);
    int steps = 0;
    while (q > 0u && !(tr_qdecode(q, scale, base) <= lo) && steps < 4) { q--; steps++; }
    while (q < 65535u && tr_qdecode(q + 1u, scale, base) <= lo && steps < 4) { q++; steps++; }
    if (steps >= 4) {
        // largest q in [0, 65535] with decode(q) <= lo (decode(0) = base <= lo by construction; NaN: 0)
        uint32_t a = 0u, z = 65535u;
        while (a < z) {
            const uint32_t m = (a + z + 1u) >> 1;
            if (tr_qdecode(m, scale, base) <= lo) a = m; else z = m - 1u;
        }
        q = a;
    }
    return q;
}
TR_HD uint32_t tr_qceil(float hi, float scale, float base) {
    uint32_t q = tr_qestimate(hi, scale, base);
    int steps = 0;
    while (q < 65535u && !(tr_qdecode(q, scale, base) >= hi) && steps < 4) { q++; steps++; }
    while (q > 0u && tr_qdecode(q - 1u, scale, base) >= hi && steps < 4) { q--; steps++; }
    if (steps >= 4) {
        // smallest q in [0, 65535] with decode(q) >= hi (decode(65535) >= hi by construction; NaN: 65535)
        uint32_t a = 0u, z = 65535u;
        while (a < z) {
            const uint32_t m = (a + z) >> 1;
            if (tr_qdecode(m, scale, base) >= hi) z = m; else a = m + 1u;
        }
        q = a;
    }
    return q;
}
// Child boxes as 16-bit pairs {lo.x, lo.y | lo.z, hi.z | hi.x, hi.y} (low half first): every pair
// meets the SAME pair of frame and ray constants ((x,y) or (z,z)), so a node decodes with 6 packed
// fma and its 12 slab planes are 6 packed subtracts + 6 packed multiplies (tr_qnode_slabs).
struct alignas(32) tr_qnode {
    uint32_t q[6];   // q[0..2] child 0, q[3..5] child 1
    int32_t c0, c1;
};
static_assert(sizeof(tr_qnode) == 32, "quantised node must be 32 B");
TR_HD void tr_qnode_set_box(uint32_t* q, const float* lo, const float* hi, const tr_qframe& f) {
    const uint32_t lx = tr_qfloor(lo[0], f.scale[0], f.base[0]), ly = tr_qfloor(lo[1], f.scale[1], f.base[1]);
    const uint32_t lz = tr_qfloor(lo[2], f.scale[2], f.base[2]);
    const uint32_t hx = tr_qceil(hi[0], f.scale[0], f.base[0]), hy = tr_qceil(hi[1], f.scale[1], f.base[1]);
    const uint32_t hz = tr_qceil(hi[2], f.scale[2], f.base[2]);
    q[0] = lx | (ly << 16); q[1] = lz | (hz << 16); q[2] = hx | (hy << 16);
}

// 48 bytes, packed: half of the records straddle a 64-byte line
struct alignas(16) tr_tri {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
    int32_t face;  // original triangle index
    float esum;    // tr_tri_scale: |b - a|_1 + |c - a|_1, the triangle's factor of the inside test's error bound (tr_tri_fast)
    int32_t pad1;
};
static_assert(sizeof(tr_tri) == 48, "tri record must be 48 B");

struct tr_bvh_view {
    const tr_node* nodes;
    const tr_link* links;
    const tr_tri* tris;
    int64_t num_tris;
    const tr_qnode* qnodes;   // 32-byte grid nodes of the unordered schedule (same topology as `nodes`)
    tr_qframe frame;
    const tr_qframe* frame_dev;   // device copy of `frame`, kept current by build / refit / load (NULL: host simulation)
    // the float top (tr_top_rec below): 8 tables of TR_TOP_SLOTS records, kept current by build / refit / load at an address
    // that never changes.  NULL: none -- an empty handle, a handle with the table switched off (tr_bvh_set_float_top), and every view that is not tr_view_of's
    const struct tr_top_rec* top = nullptr;
};
// first statement of every kernel that takes a view: the frame as it is NOW (a graph replay after a refit: the arguments
// of the captured launch still hold the old one, and both the grid nodes' decode and the rays' anchor depend on it)
#if defined(__HIP_DEVICE_COMPILE__)
#define TR_VIEW_LIVE(b) do { if ((b).frame_dev) (b).frame = *(b).frame_dev; } while (0)
#else
#define TR_VIEW_LIVE(b) ((void)0)
#endif
enum tr_query { TR_Q_ANY = 0, TR_Q_FIRST = 1, TR_Q_CLOSEST = 2, TR_Q_COUNT = 3, TR_Q_LOCATION = 4 };

struct tr_counters {
    uint32_t nodes, tris, climbs;
};

// sorted list of the K nearest hits (by (t, face)); static indexing only
template <int K>
struct tr_topk {
    float t[K];
    int32_t face[K];
    int32_t slot[K];
    TR_HDM void init() {
#pragma unroll
        for (int i = 0; i < K; i++) { t[i] = INFINITY; face[i] = 0x7fffffff; slot[i] = -1; }
    }
    TR_HDM void insert(float nt, int32_t nface, int32_t nslot) {
#pragma unroll
        for (int i = 0; i < K; i++) {
            bool lt = tr_closer(nt, nface, t[i], face[i]);
            float tt = t[i]; int32_t tf_ = face[i], ts = slot[i];
            t[i] = lt ? nt : tt; face[i] = lt ? nface : tf_; slot[i] = lt ? nslot : ts;
            nt = lt ? tt : nt; nface = lt ? tf_ : nface; nslot = lt ? ts : nslot;
        }
    }
};

// K = 0: the multi-hit list lives in memory, unsorted (tr_intersects_count_topk).  A lane carries
// a pointer and a fill count instead of 3*K registers of sorted (t, face, slot): the K = 8
// kernel needed 92 VGPRs (5 waves/SIMD) and ran a 32-select insertion for the whole wave on
// almost every leaf trip.  Appending is one 8-byte store; a ray with more than `cap` hits
// replaces its farthest stored hit when the new one is closer (rare path: loads).  The fill
// pass ranks the <= cap entries of a ray by (t_key, face) -- same final order as the sorted list.
static_assert(sizeof(tr_hit_entry) == 8, "hit entries are 8 bytes (include/triro_hip.h)");
template <>
struct tr_topk<0> {
    tr_hit_entry* ent;    // this ray's `cap` entries (set by the kernel, not by init())
    const tr_tri* tris;   // faces for tie-breaks
    int32_t cap, n;
    TR_HDM void init() { n = 0; }
    TR_HDM void insert(float nt, int32_t nface, int32_t nslot) {
        if (n < cap) {
            ent[n].t_key = nt; ent[n].slot = nslot;
            n++;
            return;
        }
        // more than `cap` hits: keep the `cap` nearest by (t_key, face)
        int32_t mi = 0;
        float mt = ent[0].t_key;
        int32_t mf = tris[ent[0].slot].face;
        for (int32_t j = 1; j < cap; j++) {
            const float tj = ent[j].t_key;
            if (tj < mt) continue;
            const int32_t fj = tris[ent[j].slot].face;
            if (tj > mt || fj > mf) { mi = j; mt = tj; mf = fj; }
        }
        if (tr_closer(nt, nface, mt, mf)) { ent[mi].t_key = nt; ent[mi].slot = nslot; }
    }
};

struct tr_result {
    // closest / first / any
    float best_t;
    int32_t best_face;   // -1 = miss
    int32_t best_slot;
    // count
    int32_t count;
};
TR_HD void tr_set_best_t(tr_result& res, float t) {
    res.best_t = t;
}

// COMPACT addressing: byte offsets fit 32 bits (nodes*64 and tris*48 below 4 GiB), so the
// loads use an SGPR base + 32-bit VGPR offset instead of 64-bit per-lane address arithmetic
template <bool COMPACT>
TR_HD const tr_f4* tr_node_ptr(const tr_bvh_view& b, int32_t node) {
    if (COMPACT)
        return reinterpret_cast<const tr_f4*>(reinterpret_cast<const char*>(b.nodes) + ((uint32_t)node << 6));
    return reinterpret_cast<const tr_f4*>(b.nodes + node);
}
template <bool COMPACT>
TR_HD const tr_i4* tr_qnode_ptr(const tr_bvh_view& b, int32_t node) {
    if (COMPACT)
        return reinterpret_cast<const tr_i4*>(reinterpret_cast<const char*>(b.qnodes) + ((uint32_t)node << 5));
    return reinterpret_cast<const tr_i4*>(b.qnodes + node);
}
template <bool COMPACT>
TR_HD const tr_f4* tr_tri_ptr(const tr_bvh_view& b, int32_t slot) {
    if (COMPACT)
        return reinterpret_cast<const tr_f4*>(reinterpret_cast<const char*>(b.tris) + (uint32_t)slot * (uint32_t)sizeof(tr_tri));
    return reinterpret_cast<const tr_f4*>(b.tris + slot);
}

TR_HD void tr_result_init(tr_result& res) {
    tr_set_best_t(res, TR_TMAX); res.best_face = -1; res.best_slot = -1;
    res.count = 0;
}
// the limit a box's entry distance is culled against (tr_math.h, TR_CULL_SLACK)
template <int Q>
TR_HD float tr_cull_limit(const tr_result& res) {
    // (the product is recomputed per trip: kept in a register beside best_t it measured slower, profiles/r06_pmc_headline.txt)
    return (Q == TR_Q_FIRST || Q == TR_Q_CLOSEST) ? res.best_t * TR_CULL_SLACK : TR_TLIM;
}

template <bool STATS, bool COMPACT = false>
TR_HD tr_tri tr_load_tri(const tr_bvh_view& b, int32_t slot, tr_counters* cnt) {
    const tr_f4* p = tr_tri_ptr<COMPACT>(b, slot);
    tr_f4 q0 = p[0], q1 = p[1], q2 = p[2];
    tr_tri t;
    t.ax = q0.x; t.ay = q0.y; t.az = q0.z; t.bx = q0.w;
    t.by = q1.x; t.bz = q1.y; t.cx = q1.z; t.cy = q1.w;
    t.cz = q2.x;
    union { float f; int32_t i; } u;
    u.f = q2.y;
    t.face = u.i;
    t.esum = q2.z;
    t.pad1 = 0;
    if (STATS) cnt->tris++;
    return t;
}

// Fold one accepted/rejected leaf test into the per-query state.  `live` = the lane really
// owns this leaf (the code runs unpredicated for the whole wave).  Returns true when the ray
// is finished (ANY query, first accepted hit).
// Fold one decided leaf test into the per-query state.  Returns true when the ray is finished (ANY query, first hit).
template <int Q, int K>
TR_HD bool tr_fold_hit(bool hit, float t, int32_t face, int32_t slot, tr_result& res, tr_topk<K>& top) {
    if (Q == TR_Q_ANY) {
        if (hit) res.best_face = face;
        return hit;
    } else if (Q == TR_Q_COUNT) {
        res.count += hit ? 1 : 0;
    } else if (Q == TR_Q_LOCATION) {
        if (hit) { res.count++; top.insert(t, face, slot); }
    } else {
        if (hit && tr_closer(t, face, res.best_t, res.best_face < 0 ? 0x7fffffff : res.best_face)) {
            tr_set_best_t(res, t); res.best_face = face; res.best_slot = slot;
        }
    }
    return false;
}
// The leaf test of the traversal: the float32 part of the predicate (tr_tri_fast) here, inside the trip; a test it
// leaves UNDECIDED (< 1 % of them: the ray passes within rounding of an edge, or grazes the plane) is parked in `pe`
// (the triangle's slot) and decided by the float64 part at the END of the trip (tr_drain_exact) -- a real call that
// owns thirty registers: there the trip's node record and triangle are dead and the call fits under the kernels'
// register budget, inside the leaf block it cost every kernel a wave per SIMD.  Until then the candidate culls
// nothing, which changes no result.  `live` = the lane really owns this leaf (the code runs unpredicated for the
// whole wave).  At most one test per trip and lane, and `pe` is emptied before the next one.
template <int Q, int K>
TR_HD bool tr_fold_leaf(bool live, const tr_ray& r, const tr_tri& t, int32_t slot, tr_result& res, tr_topk<K>& top, int32_t& pe) {
    tr_hit h;
    h.t = 0.f;
    const int c = tr_tri_fast(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, t.esum, h);
    if (live && c == TR_UNDECIDED) pe = slot;
    return tr_fold_hit<Q, K>(live && c == TR_HIT, h.t, t.face, slot, res, top);
}
// decide the parked test (see tr_fold_leaf); wave-uniform skip when no lane has one.
// COLD: the branch is marked as unlikely -- the register allocator then saves the registers the float64 call clobbers
// AROUND THE CALL (four scratch stores and loads on 0.6 % of the leaf tests) instead of keeping six kernel-lifetime
// values in scratch for the whole kernel (a store per lane in the prologue, a load after the loop: 48 MB of L2 <->
// fabric traffic per launch of the headline, L2 misses +30 %).  Headline 0.1838 -> 0.1800 ms, every direct config
// -1...-4 %; the streaming closest kernel on the binary nodes gets 10 spills and +6 % from the same hint and keeps
// the plain branch (profiles/r06_ab_cold_drain.txt).
#ifndef TR_DRAIN_COLD
#define TR_DRAIN_COLD 1     // 0: no branch hint anywhere (A/B and fault-hunting builds)
#endif
template <int Q, int K, bool COMPACT = false, bool COLD = true>
TR_HD bool tr_drain_exact(const tr_bvh_view& b, const tr_ray& r, int32_t& pe, tr_result& res, tr_topk<K>& top) {
    bool fin = false;
    const bool any_parked = TR_WAVE_ANY(pe >= 0);
    if ((COLD && TR_DRAIN_COLD) ? __builtin_expect(any_parked, 0) : any_parked) {
        if (pe >= 0) {
            tr_counters* nc = nullptr;
            const tr_tri t = tr_load_tri<false, COMPACT>(b, pe, nc);
            const tr_exact_res e = tr_tri_exact_t(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
            float tt = e.t;
            if (__builtin_expect(e.tie != 0, 0)) {
                // an exact tie (the ray passes through an edge or a vertex): does this triangle own it?  The triangle is
                // FETCHED AGAIN for that question -- kept alive across the call above it would cost every kernel eight registers
#if defined(__HIP_DEVICE_COMPILE__)
                __asm__ volatile("" ::: "memory");
#endif
                const tr_tri u = tr_load_tri<false, COMPACT>(b, pe, nc);
                if (!tr_tie_own(r.dx, r.dy, r.dz, u.ax, u.ay, u.az, u.bx, u.by, u.bz, u.cx, u.cy, u.cz, e.tie)) tt = -1.0f;
            }
            const bool hit = tt >= TR_TMIN && tt <= TR_TMAX;
            fin = tr_fold_hit<Q, K>(hit, tt, t.face, pe, res, top);
            pe = -1;
        }
    }
    return fin;
}

// Far-child stack: TR_RING words per lane (LDS on the GPU: word s of lane t lives at base[s * stride], stride =
// block size, so a wave's accesses are bank-conflict free whatever the per-lane depths are).  Far children are owed
// at strictly increasing depths and paid deepest first, so the words are a DENSE stack indexed by RANK, not by
// depth: the entry owed at depth j sits in slot popcount(owned & ((1 << j) - 1)) mod N, a push goes to slot
// popcount(owned) mod N.  `owned` has a bit per depth whose far child went into the stack; a pop at depth j
// clears every bit from j upwards, so after it popcount(owned) IS the popped entry's slot.  The stealing hand-over
// (kernels_direct.inc) takes the SHALLOWEST entry -- the bottom of the stack -- by clearing its trail bit only:
// the owned bit stays behind as a ghost below every live entry, which keeps the ranks (and so the slots) of the
// others; that is why slots wrap mod N, and why the live entries are trail & owned.  A hierarchy can be 64 levels
// deep but a ray owes few far children AT ONCE (headline: 13 at most): a push that finds all N = TR_RING slots taken
// by live entries is not recorded (no owned bit) and that far child -- the deepest one owed, the next to be paid, the
// shortest way up -- is found by climbing the parent links, as without a stack.
// (Tried and measured slower: 8 slots of {node, entry distance} with entries beyond the cull limit dropped at the pop:
// DESIGN_experiments.md part R7.)
// The unordered schedule (tr_unord_step) keeps the same words as a ring of 16 nodes indexed by depth % 16.
#define TR_RING 16
struct tr_ring {
    int32_t* base;   // nullptr = no stack (always climb)
    int32_t stride;
    int32_t* row0;   // slot 0 of the block's FIRST lane (the address form of the plain stack, tr_aring); nullptr = base
};
// Ring accesses go through an explicit LDS pointer on the device.  With the generic pointer the compiler
// merged "pop the ring slot (LDS)" and "read the sibling from links[] (global)" -- two 4-byte loads that
// feed the same variable -- into ONE flat_load_dword with a selected address: every backtracking trip
// then sent a 64-lane flat load through the texture addresser (the busiest unit of the kernels) and
// waited for vmcnt AND lgkmcnt, where a ds_read_b32 would do.
TR_HD int32_t tr_ring_get(const tr_ring& ring, uint32_t slot) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) int32_t tr_lds_i32;
    return ((tr_lds_i32*)ring.base)[slot * ring.stride];
#else
    return ring.base[slot * ring.stride];
#endif
}
TR_HD void tr_ring_put(const tr_ring& ring, uint32_t slot, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) int32_t tr_lds_i32;
    ((tr_lds_i32*)ring.base)[slot * ring.stride] = v;
#else
    ring.base[slot * ring.stride] = v;
#endif
}

// Per-lane traversal state between two iterations.  W = uint64_t in general; uint32_t when
// the hierarchy is at most 32 levels high (halves the 64-bit shift/clz work per trip).
template <typename W>
struct tr_state_t {
    int32_t node;     // next internal node to visit, -1 = hierarchy exhausted
    uint32_t depth;
    W trail;          // bit k: the node at depth k on the current path still owes its far child
    W owned;          // bit k: that far child went into the far-child stack; its slot is its rank among the set bits (tr_ring)
    // leaves found by earlier node visits (tri slots, -1 = none), tested one per trip so that their triangle loads
    // overlap the next node's load (one memory round trip per iteration); up to two arrive per visit
    int32_t p0, p1, p2;
    int32_t pe;       // a leaf test the float32 part left undecided, waiting for tr_drain_exact (-1 = none)
};
typedef tr_state_t<uint64_t> tr_state;
typedef tr_state_t<uint32_t> tr_state32;

TR_HD uint32_t tr_top_bit(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }
TR_HD uint32_t tr_top_bit(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
TR_HD uint64_t tr_ring_mask(uint64_t) { return 0x0001000100010001ull; }      // the depths that share a slot of the unordered schedule's ring (tr_unord_step)
TR_HD uint32_t tr_ring_mask(uint32_t) { return 0x00010001u; }
TR_HD uint32_t tr_popc(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
TR_HD uint32_t tr_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// Far-child stack (tr_ring): push the far child owed at `depth` (every trail / owned bit is below `depth`).
template <typename W>
TR_HD void tr_push_far(const tr_ring ring, W trail, W& owned, uint32_t depth, int32_t node) {
    if (ring.base && tr_popc(owned & trail) < TR_RING) {      // (live entries: a hand-over leaves owned bits without a trail bit)
        tr_ring_put(ring, tr_popc(owned) & (TR_RING - 1), node);
        owned |= W(1) << depth;
    }
}
// Pay the deepest far child still owed (trail != 0), the one at depth j.  Returns true: `node` comes from the stack;
// false: it is not in the stack (a push onto a full one, or no stack at all) and the caller climbs to it.
template <typename W>
TR_HD bool tr_pop_far(const tr_ring ring, W& trail, W& owned, uint32_t& j, int32_t& node) {
    j = tr_top_bit(trail);
    const W bit = W(1) << j;
    trail &= ~bit;
    const bool own = (owned & bit) != 0;
    owned &= bit - 1;                                   // this entry and what a hand-over left behind above it
    if (!(ring.base && own)) return false;
    node = tr_ring_get(ring, tr_popc(owned) & (TR_RING - 1));
    return true;
}
// the slot of the SHALLOWEST live entry (trail & owned != 0), which the stealing launches hand to an idle lane; the
// caller clears its trail bit and leaves the owned bit where it is (tr_ring)
template <typename W>
TR_HD uint32_t tr_bottom_slot(W trail, W owned, uint32_t& j) {
    j = (uint32_t)__builtin_ctzll((unsigned long long)(trail & owned));
    return tr_popc((W)(owned & ((W(1) << j) - 1))) & (TR_RING - 1);
}

template <typename W>
TR_HD void tr_state_init(tr_state_t<W>& st) {
    st.node = 0; st.depth = 0; st.trail = 0; st.owned = 0;
    st.p0 = -1; st.p1 = -1; st.p2 = -1; st.pe = -1;
}

// ---- plain far-child stack (round 8): the stealing closest / first / any launch on the grid nodes -------------------
// The far children are a LIFO, and trail / owned / depth and the rank arithmetic above exist only to find an entry again
// by climbing when the TR_RING words did not hold it, and to let the hand-over take the bottom entry: about a third of
// the VALU instructions of a trip without a leaf block, on a kernel whose vector pipes are 92 % busy, for an overflow
// that no ray of an image of a closed surface ever has.  This walk keeps the same words as a stack with a stack
// pointer and nothing else:
//   sp = 2 * (slots in use) | lost.   push: sp < 2 * TR_RING ? store at slot sp / 2, sp += 2 : sp |= 1 (the child is
//   NOT recorded and the sticky `lost` bit says that this lane's walk is no longer complete);   pop: sp < 2 ? the walk
//   is over (node = -1) : sp -= 2, load slot sp / 2.
// Order, cull limit, leaf FIFO and alternation are those of the dense stack: without an overflow the walk visits exactly
// the same nodes and tests exactly the same leaves.  A ray with a lost child (on any lane that worked on it) is
// traversed AGAIN after the wave's loop by the stackless walk over the exact nodes (tr_traverse_more), starting from the
// best hit found so far: closest / first are a lexicographic minimum over candidates and any is an OR, so the order of
// the candidates does not matter and the result is the same bits.  Cold, correct, not fast.
// Hand-over (wave_traverse_steal): the donor gives its SHALLOWEST entry, slot `bot` -- the number of entries it has
// given away since its stack was last empty, which the kernel keeps in LDS, outside the trips -- and leaves -1 in its
// place (tr_plain_give).  Far children are internal nodes (>= 0), so when the walk pops down to a given-away slot it
// reads -1: exactly "nothing left", because everything below it was given away before it.  Given-away slots stay in
// use until the lane starts another walk: a donor's stack is shorter by its gifts, and a push that does not fit is
// lost like any other.
struct tr_plain_w {};      // in place of the trail word type: selects this walk in tr_fused_body and the state below
template <>
struct tr_state_t<tr_plain_w> {
    int32_t node;     // next internal node to visit, -1 = nothing left
    uint32_t sp;      // 2 * slots in use | lost
    int32_t p0, p1, p2;
    int32_t pe;
};
typedef tr_state_t<tr_plain_w> tr_pstate;
TR_HD void tr_state_init(tr_pstate& st) {
    st.node = 0; st.sp = 0;
    st.p0 = -1; st.p1 = -1; st.p2 = -1; st.pe = -1;
}
TR_HD void tr_plain_push(const tr_ring ring, uint32_t& sp, int32_t node) {
    if (sp < 2u * TR_RING) {
        tr_ring_put(ring, sp >> 1, node);
        sp += 2u;
    } else {
        sp |= 1u;
    }
}
TR_HD int32_t tr_plain_pop(const tr_ring ring, uint32_t& sp) {
    if (sp < 2u) return -1;
    sp -= 2u;
    return tr_ring_get(ring, sp >> 1);
}
TR_HD bool tr_plain_lost(uint32_t sp) { return (sp & 1u) != 0; }
// entries a lane could still give away, and the hand-over of the shallowest of them (see above)
TR_HD bool tr_plain_can_give(uint32_t sp, uint32_t bot) { return (sp >> 1) > bot; }
TR_HD int32_t tr_plain_give(const tr_ring ring, uint32_t& bot) {
    const int32_t node = tr_ring_get(ring, bot);
    tr_ring_put(ring, bot, -1);
    bot++;
    return node;
}

// ---- the plain stack by LDS byte address (round 10): what the kernels run -------------------------------------------
// The same stack, the same slots, the same hand-over; what the lane keeps is not a slot count but
//   sa = the BYTE ADDRESS of its next free slot, counted from slot 0 of the block's first lane (tr_ring::row0: a
//   constant of the kernel that the LDS instructions carry in their offset field; on the host an int32_t[]),
// so that a push is a store and an add and a pop a subtraction and a load: no shift, no merge with the lane's base.  Slot
// s of lane t lies at 4 * t + s * stride with stride = 4 * block size > 4 * t, so WHICH slot an address belongs to does
// not depend on the lane and both ends of the stack are compile-time constants:
//   push: sa < TR_RING * stride (UNSIGNED) ? store at sa, sa += stride : the child is lost;
//   pop:  sa < stride (SIGNED) ? nothing left (-1) : sa -= stride, load at sa.
// The sticky `lost` flag is bit 31 of sa, set by the push that does not fit.  It costs the trips nothing and no access
// ever uses an address with the flag in it: to the push's unsigned test a flagged sa is beyond the top (every later
// child is dropped as well), to the pop's signed test it is below the bottom -- the walk goes on down to the next node
// without a hit child and ENDS at that pop.  The ray is traversed again from the top anyway (tr_traverse_more), so
// nothing the walk would still find is needed.  The form above (sp) goes on walking after a loss; up to the loss the
// two hand out the same nodes (tests/host_sim/plain_addr_model.cpp drives them side by side).
struct tr_plaina_w {};     // selects this walk in tr_fused_body
template <>
struct tr_state_t<tr_plaina_w> {
    int32_t node;     // next internal node to visit, -1 = nothing left
    uint32_t sa;      // byte address of the next free slot | lost
    int32_t p0, p1, p2;
    int32_t pe;
};
typedef tr_state_t<tr_plaina_w> tr_astate;
struct tr_aring {
    int32_t* row0;    // address 0: slot 0 of the block's first lane
    uint32_t stride;  // bytes from one slot of a lane to its next
};
TR_HD tr_aring tr_aring_of(const tr_ring& ring) { return tr_aring{ring.row0 ? ring.row0 : ring.base, 4u * (uint32_t)ring.stride}; }
// a fresh walk's sa: the lane's slot 0
TR_HD uint32_t tr_addr_start(const tr_ring& ring) { return ring.row0 ? 4u * (uint32_t)(ring.base - ring.row0) : 0u; }
TR_HD void tr_state_init(tr_astate& st, uint32_t sa0) {
    st.node = 0; st.sa = sa0;
    st.p0 = -1; st.p1 = -1; st.p2 = -1; st.pe = -1;
}
TR_HD int32_t tr_addr_get(const tr_aring& ar, uint32_t addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) int32_t tr_lds_i32;
    typedef __attribute__((address_space(3))) char tr_lds_i8;
    return *(tr_lds_i32*)((tr_lds_i8*)ar.row0 + addr);
#else
    return ar.row0[addr >> 2];
#endif
}
TR_HD void tr_addr_put(const tr_aring& ar, uint32_t addr, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) int32_t tr_lds_i32;
    typedef __attribute__((address_space(3))) char tr_lds_i8;
    *(tr_lds_i32*)((tr_lds_i8*)ar.row0 + addr) = v;
#else
    ar.row0[addr >> 2] = v;
#endif
}
constexpr uint32_t TR_ADDR_LOST = 0x80000000u;
TR_HD void tr_addr_push(const tr_aring& ar, uint32_t& sa, int32_t node) {
    if (sa < TR_RING * ar.stride) {
        tr_addr_put(ar, sa, node);
        sa += ar.stride;
    } else {
        sa |= TR_ADDR_LOST;
    }
}
TR_HD int32_t tr_addr_pop(const tr_aring& ar, uint32_t& sa) {
    if ((int32_t)sa < (int32_t)ar.stride) return -1;
    sa -= ar.stride;
    return tr_addr_get(ar, sa);
}
TR_HD bool tr_addr_lost(uint32_t sa) { return (sa & TR_ADDR_LOST) != 0; }
// Outside the trips (the hand-over of wave_traverse_steal): the lane's slot 0 and its slots in use, from sa alone
TR_HD uint32_t tr_addr_bottom(const tr_aring& ar, uint32_t sa) { return (sa & ~TR_ADDR_LOST) % ar.stride; }
TR_HD uint32_t tr_addr_slots(const tr_aring& ar, uint32_t sa) { return (sa & ~TR_ADDR_LOST) / ar.stride; }
// (a walk that lost a child gives nothing more away: it ends at its next pop)
TR_HD bool tr_addr_can_give(const tr_aring& ar, uint32_t sa, uint32_t bot) { return !tr_addr_lost(sa) && tr_addr_slots(ar, sa) > bot; }
TR_HD int32_t tr_addr_give(const tr_aring& ar, uint32_t sa, uint32_t& bot) {
    const uint32_t a = tr_addr_bottom(ar, sa) + bot * ar.stride;
    const int32_t node = tr_addr_get(ar, a);
    tr_addr_put(ar, a, -1);
    bot++;
    return node;
}

template <typename W>
TR_HD bool tr_pending(const tr_state_t<W>& st) { return st.p0 >= 0 || st.p1 >= 0; }
template <typename W>
TR_HD bool tr_done(const tr_state_t<W>& st) { return st.node < 0 && st.p0 < 0 && st.p1 < 0 && st.pe < 0; }

// Slab intervals of both children of a node held in three 16-byte registers:
// n0 = lo0.x lo0.y lo0.z hi0.z | n1 = hi0.x hi0.y lo1.x lo1.y | n2 = lo1.z hi1.z hi1.x hi1.y.
// On the device the 12 planes are packed FP32 (v_pk_add_f32 / v_pk_mul_f32: the same IEEE
// subtract and multiply per plane as tr_slab, two planes per instruction).
TR_HD void tr_node_slabs(const tr_ray& r, const tr_f4& n0, const tr_f4& n1, const tr_f4& n2,
                         float& tn0, float& tf0, float& tn1, float& tf1) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float tr_v2 __attribute__((ext_vector_type(2)));
    const tr_v2 oxy = {r.ox, r.oy}, ozz = {r.oz, r.oz};
    const tr_v2 ixy = {r.ix, r.iy}, izz = {r.iz, r.iz};
    const tr_v2 a = (tr_v2{n0.x, n0.y} - oxy) * ixy;   // child 0: x1 y1
    const tr_v2 b = (tr_v2{n0.z, n0.w} - ozz) * izz;   //          z1 z2
    const tr_v2 c = (tr_v2{n1.x, n1.y} - oxy) * ixy;   //          x2 y2
    const tr_v2 d = (tr_v2{n1.z, n1.w} - oxy) * ixy;   // child 1: x1 y1
    const tr_v2 e = (tr_v2{n2.x, n2.y} - ozz) * izz;   //          z1 z2
    const tr_v2 f = (tr_v2{n2.z, n2.w} - oxy) * ixy;   //          x2 y2
    tn0 = fmaxf(fmaxf(fminf(a.x, c.x), fminf(a.y, c.y)), fminf(b.x, b.y));
    tf0 = fminf(fminf(fmaxf(a.x, c.x), fmaxf(a.y, c.y)), fmaxf(b.x, b.y)) * TR_SLAB_PAD;
    tn1 = fmaxf(fmaxf(fminf(d.x, f.x), fminf(d.y, f.y)), fminf(e.x, e.y));
    tf1 = fminf(fminf(fmaxf(d.x, f.x), fmaxf(d.y, f.y)), fmaxf(e.x, e.y)) * TR_SLAB_PAD;
#else
    tr_slab(r, n0.x, n0.y, n0.z, n1.x, n1.y, n0.w, tn0, tf0);
    tr_slab(r, n1.z, n1.w, n2.x, n2.z, n2.w, n2.y, tn1, tf1);
#endif
}

// NODE PHASE: visit st.node (lane must have a node and no queued leaf): fetch the 64-B node,
// test both child boxes, queue hit leaf children in (p0, p1), then move to the next node
// (near child, or the deepest owed far child; -1 when the hierarchy is exhausted).
template <int Q, bool STATS>
TR_HD void tr_node_step(const tr_bvh_view& b, const tr_ray& r, tr_state& st, const tr_result& res,
                        tr_counters* cnt, const tr_ring ring) {
    const tr_f4* np = reinterpret_cast<const tr_f4*>(b.nodes + st.node);
    const tr_f4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
    if (STATS) cnt->nodes++;
    // n3 = c0 c1 parent sibling
    float tn0, tf0, tn1, tf1;
    tr_node_slabs(r, n0, n1, n2, tn0, tf0, tn1, tf1);
    union { float f; int32_t i; } u0, u1, u2, u3;
    u0.f = n3.x; u1.f = n3.y; u2.f = n3.z; u3.f = n3.w;
    const int32_t c0 = u0.i, c1 = u1.i;
    int32_t parent = u2.i, sibling = u3.i;
    const float lim = tr_cull_limit<Q>(res);
    bool h0 = tr_slab_hit(tn0, tf0, lim);
    bool h1 = tr_slab_hit(tn1, tf1, lim);
    // leaf children are queued for the leaf phase
    if (h0 && c0 < 0) { st.p0 = ~c0; h0 = false; }
    if (h1 && c1 < 0) { st.p1 = ~c1; h1 = false; }
    if (h0 | h1) {
        const bool both = h0 & h1;
        const bool swap = both ? (tn1 < tn0) : h1;   // descend into c1?
        if (both) {
            tr_push_far(ring, st.trail, st.owned, st.depth, swap ? c0 : c1);
            st.trail |= (1ull << st.depth);
        }
        st.node = swap ? c1 : c0;
        st.depth++;
    } else if (st.trail == 0) {
        st.node = -1;
    } else {
        // backtrack to the deepest ancestor that still owes its far child
        uint32_t j = 0;
        int32_t far = -1;
        if (tr_pop_far(ring, st.trail, st.owned, j, far)) {
            st.node = far;
        } else {
            int32_t node = st.node;
            uint32_t depth = st.depth;
            while (depth > j + 1) {   // climb; `node` is at `depth`, (parent, sibling) its links
                node = parent;
                const tr_link l = b.links[node];
                parent = l.parent; sibling = l.sibling;
                depth--;
                if (STATS) cnt->climbs++;
            }
            st.node = sibling;        // far child at depth j+1 (internal by construction)
        }
        st.depth = j + 1;
    }
}

// LEAF PHASE: test the queued leaves (both triangle loads are issued before either test).
// Runs unpredicated for the calling lanes; lanes without a queued leaf in a slot compute on
// triangle 0 and discard.  Sets st.node = -1 when an ANY query is satisfied.
template <int Q, int K, bool STATS>
TR_HD void tr_leaf_step(const tr_bvh_view& b, const tr_ray& r, tr_state& st, tr_result& res,
                        tr_topk<K>& top, tr_counters* cnt) {
    const int32_t q0 = st.p0, q1 = st.p1;
    tr_counters* nc = nullptr;
    const bool any1 = TR_WAVE_ANY(q1 >= 0);
    const tr_tri t0 = tr_load_tri<false>(b, q0 >= 0 ? q0 : 0, nc);
    tr_tri t1 = t0;
    if (any1) t1 = tr_load_tri<false>(b, q1 >= 0 ? q1 : 0, nc);
    if (STATS && q0 >= 0) cnt->tris++;
    bool fin = tr_fold_leaf<Q, K>(q0 >= 0, r, t0, q0, res, top, st.pe);
    fin = tr_drain_exact<Q, K>(b, r, st.pe, res, top) || fin;
    if (any1) {
        const bool live = q1 >= 0 && !fin;
        if (STATS && live) cnt->tris++;
        fin = tr_fold_leaf<Q, K>(live, r, t1, q1, res, top, st.pe) || fin;
        fin = tr_drain_exact<Q, K>(b, r, st.pe, res, top) || fin;
    }
    st.p0 = -1; st.p1 = -1;
    if (Q == TR_Q_ANY && fin) st.node = -1;
}

// FUSED STEP (software-pipelined schedule): one trip = node fetch for every lane that has a
// node + the test of a leaf queued by an EARLIER trip.  The node loads are issued first, so
// the triangle loads and the node loads are in flight together: one memory round trip per
// trip.  Lanes never sit out.
// Slab intervals of both children of a 32-byte grid node held in two 16-byte registers:
// w0 = q[0..3], w1 = q[4], q[5], c0, c1.  The contract's form: plane = fma(q, scale, base) per 16-bit half, then
// tr_slab's subtract and multiply per plane.  The kernels use the fused form below; tests/host_sim checks the two
// against each other.
TR_HD void tr_qnode_slabs_contract(const tr_ray& r, const tr_qframe& f, const tr_i4& w0, const tr_i4& w1,
                                   float& tn0, float& tf0, float& tn1, float& tf1) {
    const uint32_t q0 = (uint32_t)w0.x, q1 = (uint32_t)w0.y, q2 = (uint32_t)w0.z, q3 = (uint32_t)w0.w;
    const uint32_t q4 = (uint32_t)w1.x, q5 = (uint32_t)w1.y;
    const float sx = f.scale[0], sy = f.scale[1], sz = f.scale[2], bx = f.base[0], by = f.base[1], bz = f.base[2];
    tr_slab(r, tr_qdecode(q0 & 0xffffu, sx, bx), tr_qdecode(q0 >> 16, sy, by), tr_qdecode(q1 & 0xffffu, sz, bz),
            tr_qdecode(q2 & 0xffffu, sx, bx), tr_qdecode(q2 >> 16, sy, by), tr_qdecode(q1 >> 16, sz, bz), tn0, tf0);
    tr_slab(r, tr_qdecode(q3 & 0xffffu, sx, bx), tr_qdecode(q3 >> 16, sy, by), tr_qdecode(q4 & 0xffffu, sz, bz),
            tr_qdecode(q5 & 0xffffu, sx, bx), tr_qdecode(q5 >> 16, sy, by), tr_qdecode(q4 >> 16, sz, bz), tn1, tf1);
}

// The fused form (tr_ray_fuse): per child three v_perm_b32 (entry / exit planes of this ray), six conversions, THREE
// packed fma, one max3, one min3 -- 14 instead of 22 instructions; no pad multiply (the margin e is in B).  Host and
// device evaluate the same fma per plane: identical (tn, tf), so tests/host_sim walks the very path the kernels walk.
TR_HD void tr_qnode_slabs(const tr_ray& r, const tr_qframe& f, const tr_i4& w0, const tr_i4& w1,
                          float& tn0, float& tf0, float& tn1, float& tf1) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t q0 = (uint32_t)w0.x, q1 = (uint32_t)w0.y, q2 = (uint32_t)w0.z, q3 = (uint32_t)w0.w;
    const uint32_t q4 = (uint32_t)w1.x, q5 = (uint32_t)w1.y;
    typedef float tr_v2 __attribute__((ext_vector_type(2)));
    const tr_v2 axy = {r.qax, r.qay}, azz = {r.qaz, r.qaz2};
    const tr_v2 nxy = {r.qnx, r.qny}, fxy = {r.qfx, r.qfy}, bz = {r.qnz, r.qfz};
#define TR_UNPK(w) tr_v2{(float)((w) & 0xffffu), (float)((w) >> 16)}
    {
        const uint32_t pn = __builtin_amdgcn_perm(q2, q0, r.sel_n), pf = __builtin_amdgcn_perm(q2, q0, r.sel_f);
        const uint32_t zz = __builtin_amdgcn_perm(q1, q1, r.sel_z);      // (entry z | exit z << 16)
        const tr_v2 a = __builtin_elementwise_fma(TR_UNPK(pn), axy, nxy);
        const tr_v2 c = __builtin_elementwise_fma(TR_UNPK(pf), axy, fxy);
        const tr_v2 b = __builtin_elementwise_fma(TR_UNPK(zz), azz, bz);
        tn0 = fmaxf(fmaxf(a.x, a.y), b.x);
        tf0 = fminf(fminf(c.x, c.y), b.y);
    }
    {
        const uint32_t pn = __builtin_amdgcn_perm(q5, q3, r.sel_n), pf = __builtin_amdgcn_perm(q5, q3, r.sel_f);
        const uint32_t zz = __builtin_amdgcn_perm(q4, q4, r.sel_z);
        const tr_v2 a = __builtin_elementwise_fma(TR_UNPK(pn), axy, nxy);
        const tr_v2 c = __builtin_elementwise_fma(TR_UNPK(pf), axy, fxy);
        const tr_v2 b = __builtin_elementwise_fma(TR_UNPK(zz), azz, bz);
        tn1 = fmaxf(fmaxf(a.x, a.y), b.x);
        tf1 = fminf(fminf(c.x, c.y), b.y);
    }
#undef TR_UNPK
#else
    (void)f;
    const bool nx = r.ix < 0.f, ny = r.iy < 0.f, nz = r.iz < 0.f;      // as sel_n / sel_f / sel_z (tr_ray_setup)
    const uint32_t q[6] = {(uint32_t)w0.x, (uint32_t)w0.y, (uint32_t)w0.z, (uint32_t)w0.w, (uint32_t)w1.x, (uint32_t)w1.y};
    float tn[2], tf[2];
    for (int c = 0; c < 2; c++) {
        const uint32_t lox = q[3 * c] & 0xffffu, loy = q[3 * c] >> 16, loz = q[3 * c + 1] & 0xffffu;
        const uint32_t hiz = q[3 * c + 1] >> 16, hix = q[3 * c + 2] & 0xffffu, hiy = q[3 * c + 2] >> 16;
        const float ax = fmaf((float)(nx ? hix : lox), r.qax, r.qnx), ay = fmaf((float)(ny ? hiy : loy), r.qay, r.qny);
        const float az = fmaf((float)(nz ? hiz : loz), r.qaz, r.qnz);
        const float cx = fmaf((float)(nx ? lox : hix), r.qax, r.qfx), cy = fmaf((float)(ny ? loy : hiy), r.qay, r.qfy);
        const float cz = fmaf((float)(nz ? loz : hiz), r.qaz, r.qfz);
        tn[c] = fmaxf(fmaxf(ax, ay), az);
        tf[c] = fminf(fminf(cx, cy), cz);
    }
    tn0 = tn[0]; tf0 = tf[0]; tn1 = tn[1]; tf1 = tf[1];
#endif
}

// Backtracking without the ring and without parent / sibling in the node record: climb the parent
// links from `node` (at `depth`) to the ancestor at depth j+1 and return its sibling -- the far
// child owed at depth j (internal by construction).  One dependent 8-byte load per level.
template <bool STATS>
TR_HD int32_t tr_climb(const tr_bvh_view& b, int32_t node, uint32_t depth, uint32_t j, tr_counters* cnt) {
    tr_link l = b.links[node];
    if (STATS) cnt->climbs++;
    while (depth > j + 1) {
        node = l.parent;
        l = b.links[node];
        depth--;
        if (STATS) cnt->climbs++;
    }
    return l.sibling;
}

// A fetched node record for the fused trip: the exact 64-byte node (four 16-byte words) or the
// 32-byte grid node (two).  With the full predicate at the leaves (tr_fold_leaf) the trip only needs
// CONSERVATIVE child boxes, so the pruning queries can walk the grid nodes too: two gathers per
// visit instead of four, for a decode of 18 VALU instructions.
struct tr_rec_f { tr_f4 n0, n1, n2, n3; };
struct tr_rec_q { tr_i4 w0, w1; };
TR_HD void tr_rec_slabs(const tr_bvh_view&, const tr_ray& r, const tr_rec_f& n, float& tn0, float& tf0, float& tn1, float& tf1) {
    tr_node_slabs(r, n.n0, n.n1, n.n2, tn0, tf0, tn1, tf1);
}
TR_HD void tr_rec_slabs(const tr_bvh_view& b, const tr_ray& r, const tr_rec_q& n, float& tn0, float& tf0, float& tn1, float& tf1) {
    tr_qnode_slabs(r, b.frame, n.w0, n.w1, tn0, tf0, tn1, tf1);
}
TR_HD void tr_rec_children(const tr_rec_f& n, int32_t& c0, int32_t& c1) {
    union { float f; int32_t i; } u0, u1;
    u0.f = n.n3.x; u1.f = n.n3.y; c0 = u0.i; c1 = u1.i;
}
TR_HD void tr_rec_children(const tr_rec_q& n, int32_t& c0, int32_t& c1) { c0 = n.w1.z; c1 = n.w1.w; }
// parent / sibling of the visited node: the first step of a climb comes with the exact record
// (n3 = c0 c1 parent sibling); the grid node does not carry them (tr_climb reads links[])
TR_HD void tr_rec_links(const tr_rec_f& n, int32_t& parent, int32_t& sibling) {
    union { float f; int32_t i; } u2, u3;
    u2.f = n.n3.z; u3.f = n.n3.w; parent = u2.i; sibling = u3.i;
}
TR_HD void tr_rec_links(const tr_rec_q&, int32_t& parent, int32_t& sibling) { parent = -1; sibling = -1; }

// everything of a trip after the node record has arrived (n0..n3: in vector registers, or -- on
// trips where the whole wave visits the same node -- in scalar registers)
// TEST = false: a trip WITHOUT the leaf block (tr_fused_step)
template <int Q, int K, bool STATS, bool COMPACT, typename W, bool TEST, bool COLD, typename REC>
TR_HD void tr_fused_body(const tr_bvh_view& b, const tr_ray& r, tr_state_t<W>& st, tr_result& res,
                         tr_topk<K>& top, tr_counters* cnt, const tr_ring ring, const bool has_node,
                         const REC& rec) {
    if (STATS && has_node) cnt->nodes++;
    bool fin = false;
    const int32_t q0 = st.p0;
    if (TEST && TR_WAVE_ANY(q0 >= 0)) {
        tr_counters* nc = nullptr;
        const tr_tri t0 = tr_load_tri<false, COMPACT>(b, q0 >= 0 ? q0 : 0, nc);
        const bool live = q0 >= 0;
        if (STATS && live) cnt->tris++;
        fin = tr_fold_leaf<Q, K>(live, r, t0, q0, res, top, st.pe);
    }
    if (Q == TR_Q_ANY && fin) { st.node = -1; st.p1 = -1; st.p2 = -1; }
    float tn0, tf0, tn1, tf1;
    tr_rec_slabs(b, r, rec, tn0, tf0, tn1, tf1);
    int32_t c0, c1, parent, sibling;
    tr_rec_children(rec, c0, c1);
    tr_rec_links(rec, parent, sibling);
    const float lim = tr_cull_limit<Q>(res);
    const bool go = has_node && st.node >= 0;
    bool h0 = tr_slab_hit(tn0, tf0, lim) && go;
    bool h1 = tr_slab_hit(tn1, tf1, lim) && go;
    // Leaf schedule: ONE leaf test per trip out of a 3-slot per-lane FIFO (a node visit can add two
    // leaves while one is consumed; the node waits only when the FIFO is full).  Testing both leaves
    // of the previous visit in the same trip gives the same results with 12 more live registers and
    // is 5 % slower at >= 4 M rays.
    // New FIFO = (carried entries, new leaf of child 0, new leaf of child 1), written as selects
    // (no shift-then-push: every move is a v_cndmask).  The head (p0) was consumed above; b =
    // old p1 and c = old p2 are carried.  When c is valid the node waited (go is false, no new
    // leaves) and c takes the place of "leaf of child 1" in the formulas below.
    if (!TEST) {
        // the head was NOT consumed; a lane that visits its node on such a trip holds at most one
        // queued leaf (p0), so FIFO = (p0, new leaf of child 0, new leaf of child 1) still fits.
        // Lanes that do not visit keep their FIFO as it is.
        const bool l0 = h0 && c0 < 0, l1 = h1 && c1 < 0;
        h0 = h0 && c0 >= 0;
        h1 = h1 && c1 >= 0;
        if (go) {
            const bool hb = st.p0 >= 0, two = l0 && l1;
            const int32_t xi = l0 ? ~c0 : (l1 ? ~c1 : -1);
            st.p2 = (hb && two) ? ~c1 : -1;
            st.p1 = hb ? xi : (two ? ~c1 : -1);
            st.p0 = hb ? st.p0 : xi;
        }
    } else {
        const bool l0 = h0 && c0 < 0;
        const bool wait = st.p2 >= 0;
        const bool l1 = (h1 && c1 < 0) || wait;
        h0 = h0 && c0 >= 0;
        h1 = h1 && c1 >= 0;
        const int32_t i1 = wait ? st.p2 : ~c1;
        const bool hb = st.p1 >= 0, two = l0 && l1;
        const int32_t xi = l0 ? ~c0 : (l1 ? i1 : -1);      // first new entry
        st.p0 = hb ? st.p1 : xi;
        st.p1 = hb ? xi : (two ? i1 : -1);
        st.p2 = (hb && two) ? i1 : -1;
    }
    if constexpr (std::is_same<W, tr_plain_w>::value) {
        // the plain stack (tr_plain_push): no trail, no depth, no climb.  The descend path's select is written FIRST and for
        // every lane, the pop's load into the same register behind it: with the pop in a branch of its own in front, the
        // select overwrote a register with a load outstanding and the compiler made the whole wave wait for LDS (and for
        // the push's store) in the middle of the body; now the popped node is waited for where the next trip needs it.
        // KEEP THIS ORDER: an if / else of descend and pop computes the same and brings the wait back (headline +1.2 %,
        // wait cycles per wave -3.5 %: DESIGN_experiments.md part R9, with the assembly of both forms)
        if (go) {
            const bool both = h0 && h1;
            const bool swap = (both && tn1 < tn0) || !h0;   // descend into c1?
            if (both) tr_plain_push(ring, st.sp, swap ? c0 : c1);
            st.node = swap ? c1 : c0;
            if (!(h0 || h1)) st.node = tr_plain_pop(ring, st.sp);
        }
    } else if constexpr (std::is_same<W, tr_plaina_w>::value) {
        // the same walk with the stack pointer as an LDS byte address (tr_addr_push), in the same order
        if (go) {
            const tr_aring ar = tr_aring_of(ring);
            const bool both = h0 && h1;
            const bool swap = (both && tn1 < tn0) || !h0;   // descend into c1?
            if (both) tr_addr_push(ar, st.sa, swap ? c0 : c1);
            st.node = swap ? c1 : c0;
            if (!(h0 || h1)) st.node = tr_addr_pop(ar, st.sa);
        }
    } else if (go) {
        if (h0 || h1) {
            const bool both = h0 && h1;
            const bool swap = (both && tn1 < tn0) || !h0;   // descend into c1?
            if (both) {
                tr_push_far(ring, st.trail, st.owned, st.depth, swap ? c0 : c1);
                st.trail |= (W(1) << st.depth);
            }
            st.node = swap ? c1 : c0;
            st.depth++;
        } else if (st.trail == 0) {
            st.node = -1;
        } else {
            uint32_t j = 0;
            int32_t far = -1;
            if (!tr_pop_far(ring, st.trail, st.owned, j, far)) {      // not in the stack (the rare push onto a full one): climb
                if constexpr (std::is_same<REC, tr_rec_f>::value) {
                    int32_t node = st.node;
                    uint32_t depth = st.depth;
                    while (depth > j + 1) {
                        node = parent;
                        const tr_link l = b.links[node];
                        parent = l.parent; sibling = l.sibling;
                        depth--;
                        if (STATS) cnt->climbs++;
                    }
                    far = sibling;
                } else {
                    far = tr_climb<STATS>(b, st.node, st.depth, j, cnt);
                }
            }
            st.node = far;
            st.depth = j + 1;
        }
    }
    // the test this trip's leaf block left undecided, now that the trip's record and triangle are dead (tr_fold_leaf)
    if (TEST) {
        if (tr_drain_exact<Q, K, COMPACT, COLD>(b, r, st.pe, res, top) && Q == TR_Q_ANY) { st.node = -1; st.p0 = -1; st.p1 = -1; st.p2 = -1; }
        st.pe = -1;     // (it is: said once more so that the compiler does not carry it around the loop)
    }
}


// UNI: look for wave-uniform trips (below).  Worth it for large coherent batches (4 M rays: -4 %,
// 16.7 M: -5 %), a loss where the texture path is not the busiest unit or uniform trips are rare
// (1 M rays +-0, 262 k rays +5 %, coarse meshes +3 %, incoherent batches +2 %): the test costs two
// ballots and a readlane on every trip.
//
// TEST: this trip has a leaf block.  The leaf block -- three triangle loads, Moller-Trumbore, a
// division: 3 of the trip's 7 vector-memory instructions and about half of its VALU instructions --
// is executed by the whole wave whenever ANY lane has a queued leaf, i.e. on nearly every trip, while
// only ~8 % of the lane-trips have one.  The callers therefore alternate trips with and without it:
// on a trip without, a lane visits its node if it holds at most one queued leaf (so that two new
// ones still fit).  A leaf is tested at most one trip later than before; same tests, same results.
// QN: walk the 32-byte grid nodes instead of the exact 64-byte ones (see tr_rec_q).
template <int Q, int K, bool STATS, bool COMPACT = false, typename W = uint64_t, bool UNI = false, bool TEST = true,
          bool QN = false, bool COLD = true>
TR_HD void tr_fused_step(const tr_bvh_view& b, const tr_ray& r, tr_state_t<W>& st, tr_result& res,
                         tr_topk<K>& top, tr_counters* cnt, const tr_ring ring) {
    // one leaf test per trip: the head of the lane's FIFO (p0, p1, p2).  The node is visited
    // unless the FIFO is full (it then waits one trip: no fetch, no new leaves).
    const int32_t room = TEST ? st.p2 : st.p1;     // must be empty (-1) for the node to be visited
    const bool has_node = st.node >= 0 && room < 0;
#if defined(__HIP_DEVICE_COMPILE__)
    // Wave-uniform trips: 36-44 % of the node visits of an image-shaped batch happen on trips where
    // every visiting lane is at the SAME node (the top of the tree under an 8x8 pixel tile).  The
    // record is then fetched once, by the scalar unit, instead of by a 64-lane gather of four
    // dwordx4 that all hit the same line: no texture-path work at all for that trip.
    if (UNI) {
        const unsigned long long m = __ballot(has_node);
        if (m != 0ull) {
            const int32_t nu = __builtin_amdgcn_readlane(st.node, (int)__builtin_ctzll(m));
            if (__ballot(has_node && st.node != nu) == 0ull) {
                // constant address space: the node array is read-only while queries run, and a
                // uniform address in that space is what selects the scalar memory path
                if constexpr (QN) {
                    typedef const __attribute__((address_space(4))) tr_i4* tr_ci4p;
                    const tr_ci4p sp = (tr_ci4p)(unsigned long long)tr_qnode_ptr<COMPACT>(b, nu);
                    const tr_rec_q rec = {sp[0], sp[1]};
                    tr_fused_body<Q, K, STATS, COMPACT, W, TEST, COLD>(b, r, st, res, top, cnt, ring, has_node, rec);
                } else {
                    typedef const __attribute__((address_space(4))) tr_f4* tr_cf4p;
                    const tr_cf4p sp = (tr_cf4p)(unsigned long long)tr_node_ptr<COMPACT>(b, nu);
                    const tr_rec_f rec = {sp[0], sp[1], sp[2], sp[3]};
                    tr_fused_body<Q, K, STATS, COMPACT, W, TEST, COLD>(b, r, st, res, top, cnt, ring, has_node, rec);
                }
                return;
            }
        }
    }
#endif
    // node index or 0, from the sign bits.  (A select under `has_node` keeps the SGPR-base + 32-bit-offset form of the
    // node loads with the present compiler -- the loss of it was the reason for this form -- and is two VALU instructions
    // shorter in the loop of two trips, but measured no faster: DESIGN_experiments.md part R10.)
    const int32_t nidx = st.node & ~(st.node >> 31) & (room >> 31);
    if constexpr (QN) {
        const tr_i4* np = tr_qnode_ptr<COMPACT>(b, nidx);
        const tr_rec_q rec = {np[0], np[1]};
        tr_fused_body<Q, K, STATS, COMPACT, W, TEST, COLD>(b, r, st, res, top, cnt, ring, has_node, rec);
    } else {
        const tr_f4* np = tr_node_ptr<COMPACT>(b, nidx);
        const tr_rec_f rec = {np[0], np[1], np[2], np[3]};
        tr_fused_body<Q, K, STATS, COMPACT, W, TEST, COLD>(b, r, st, res, top, cnt, ring, has_node, rec);
    }
}

// DESCENT STEP: a trip of a lane whose leaf FIFO is empty and which has nothing parked (p0 = p1 = p2 = pe = -1), for the
// plain stack by LDS byte address over the grid nodes.  With an empty FIFO both flavours of tr_fused_step do the same: no leaf
// block, no drain, the node is visited, and the FIFO afterwards holds exactly the accepted leaf children.  This is that trip
// with everything left out whose result is known: room / has_node, the FIFO's selects, the wave-any tests, the drain.  The
// caller (wave_traverse_steal) runs it for lanes with st.node >= 0 while NO lane of the wave holds a leaf, and enters the
// reported leaves -- l0 / l1: child 0 / 1 is an accepted leaf, c0 / c1 the children -- into the FIFO itself, on the one
// trip that finds some: p0 = the first of them, p1 = the second.  Same fetch, same box test, same cull limit, and the
// statements of tr_fused_body's tr_plaina_w branch in their order (the descend select first, the pop behind it: part R9).
// (The report as two registers -- the accepted child or 0, negative = a leaf -- makes the loop eleven scalar instructions
// shorter and the allocator keep kernel-lifetime values in scratch in the DEEP instantiations: part R11, not this form.)
template <int Q, bool STATS, bool COMPACT>
TR_HD void tr_descent_step(const tr_bvh_view& b, const tr_ray& r, tr_astate& st, const tr_result& res, tr_counters* cnt,
                           const tr_ring ring, bool& l0, bool& l1, int32_t& c0, int32_t& c1) {
    const tr_i4* np = tr_qnode_ptr<COMPACT>(b, st.node);
    const tr_rec_q rec = {np[0], np[1]};
    if (STATS) cnt->nodes++;
    float tn0, tf0, tn1, tf1;
    tr_rec_slabs(b, r, rec, tn0, tf0, tn1, tf1);
    tr_rec_children(rec, c0, c1);
    const float lim = tr_cull_limit<Q>(res);
    bool h0 = tr_slab_hit(tn0, tf0, lim);
    bool h1 = tr_slab_hit(tn1, tf1, lim);
    l0 = h0 && c0 < 0;
    l1 = h1 && c1 < 0;
    h0 = h0 && c0 >= 0;
    h1 = h1 && c1 >= 0;
    const tr_aring ar = tr_aring_of(ring);
    const bool both = h0 && h1;
    const bool swap = (both && tn1 < tn0) || !h0;   // descend into c1?
    if (both) tr_addr_push(ar, st.sa, swap ? c0 : c1);
    st.node = swap ? c1 : c0;
    if (!(h0 || h1)) st.node = tr_addr_pop(ar, st.sa);
}

// UNIFORM TRIP: tr_descent_step's trip for a wave whose visiting lanes are all at ONE node and whose rays all point into ONE
// octant.  The record (w0, w1) and the octant are then the same in every lane -- on the device they sit in scalar registers
// -- and everything that depends on them alone is done once for the wave, on the scalar unit, and in as few instructions as
// the vector unit saves: the wave pays for every instruction it issues, of either kind (part R17: a first form with
// 112 scalar instructions per trip was 2 % SLOWER with 4 % fewer vector instructions).  Three pieces, which the kernel
// (wave_traverse_steal) and the host simulation (tests/host_sim/uniform_top_model.cpp) put together in the same way:
//   tr_uniform_test   per lane: the box test of both children -- the conversion of each chosen plane (one scalar operand
//                     each), the same fma((float)q, a, n) per plane as tr_qnode_slabs, the same tr_slab_hit against the same
//                     cull limit -- as three compares: box 0 / 1 accepted, child 1 nearer;
//   tr_uniform_wave   per wave, on lane masks (bit k = lane k): from the three compares of every lane (the device's ballots)
//                     and the children, the lanes that accept a leaf child, push, descend into child 1, have no child to go
//                     to -- tr_descent_step's formulas, 64 lanes per scalar instruction;
//   tr_lane_in        a lane's bit of such a mask (on the device the mask IS the condition register: no instruction).
// The lane's next node is NOT written and its far-child stack is NOT popped inside the loop: the caller goes on to child
// `sw` while that is the same child for every lane, and leaves the loop -- writing the nodes, popping where `pop` -- after
// the first trip on which it is not, some lane has no child to go to, or a leaf child is accepted.
struct tr_uoctant {
    uint32_t mxy;        // 0xffff in the half of an (x | y << 16) pair whose axis the rays walk in the negative direction
    uint32_t she, shf;   // shift of the (lo.z | hi.z << 16) pair that brings the entry / the exit plane down
};
// from the selectors of any ray of the wave (tr_ray_setup: sel_n, sel_z)
TR_HD tr_uoctant tr_uniform_octant(uint32_t sel_n, uint32_t sel_z) {
    const bool nx = (sel_n & 0x0400u) != 0u, ny = (sel_n & 0x04000000u) != 0u, nz = (sel_z & 2u) != 0u;
    return tr_uoctant{(nx ? 0xffffu : 0u) | (ny ? 0xffff0000u : 0u), nz ? 16u : 0u, nz ? 0u : 16u};
}
template <int Q>
TR_HD void tr_uniform_test(const tr_ray& r, const tr_i4& w0, const tr_i4& w1, const tr_uoctant& oct, const tr_result& res,
                           bool& a0, bool& a1, bool& lt) {
    const uint32_t q[6] = {(uint32_t)w0.x, (uint32_t)w0.y, (uint32_t)w0.z, (uint32_t)w0.w, (uint32_t)w1.x, (uint32_t)w1.y};
    float tn[2], tf[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        // {lo.x, lo.y} and {hi.x, hi.y} with the halves of the negative axes exchanged: {entry x, entry y}, {exit x, exit y}
        const uint32_t t = (q[3 * c] ^ q[3 * c + 2]) & oct.mxy;
        const uint32_t e = q[3 * c] ^ t, f = q[3 * c + 2] ^ t, z = q[3 * c + 1];
        const float ex = (float)(e & 0xffffu), ey = (float)(e >> 16), ez = (float)((z >> oct.she) & 0xffffu);
        const float fx = (float)(f & 0xffffu), fy = (float)(f >> 16), fz = (float)((z >> oct.shf) & 0xffffu);
#if defined(__HIP_DEVICE_COMPILE__)
        typedef float tr_v2 __attribute__((ext_vector_type(2)));      // the pairs of tr_qnode_slabs
        const tr_v2 a = __builtin_elementwise_fma(tr_v2{ex, ey}, tr_v2{r.qax, r.qay}, tr_v2{r.qnx, r.qny});
        const tr_v2 b = __builtin_elementwise_fma(tr_v2{fx, fy}, tr_v2{r.qax, r.qay}, tr_v2{r.qfx, r.qfy});
        const tr_v2 d = __builtin_elementwise_fma(tr_v2{ez, fz}, tr_v2{r.qaz, r.qaz2}, tr_v2{r.qnz, r.qfz});
        tn[c] = fmaxf(fmaxf(a.x, a.y), d.x);
        tf[c] = fminf(fminf(b.x, b.y), d.y);
#else
        tn[c] = fmaxf(fmaxf(fmaf(ex, r.qax, r.qnx), fmaf(ey, r.qay, r.qny)), fmaf(ez, r.qaz, r.qnz));
        tf[c] = fminf(fminf(fmaf(fx, r.qax, r.qfx), fmaf(fy, r.qay, r.qfy)), fmaf(fz, r.qaz, r.qfz));
#endif
    }
    const float lim = tr_cull_limit<Q>(res);
    a0 = tr_slab_hit(tn[0], tf[0], lim);
    a1 = tr_slab_hit(tn[1], tf[1], lim);
    lt = tn[1] < tn[0];
}
struct tr_uwave {
    uint64_t l0, l1;     // child 0 / 1 is an accepted leaf                     (tr_descent_step: l0, l1)
    uint64_t both;       // both children are accepted internal nodes: push     (both)
    uint64_t sw;         // descend into child 1                                (swap; set for a lane of `pop` as well)
    uint64_t pop;        // no accepted internal child                          (!(h0 || h1))
};
// act: the lanes with a node; a0 / a1 / lt: tr_uniform_test's compares of every lane, whatever it computed them from
TR_HD tr_uwave tr_uniform_wave(uint64_t act, uint64_t a0, uint64_t a1, uint64_t lt, int32_t c0, int32_t c1) {
    const uint64_t m0 = a0 & act, m1 = a1 & act;
    const uint64_t h0 = c0 >= 0 ? m0 : 0ull, h1 = c1 >= 0 ? m1 : 0ull;
    tr_uwave u;
    u.l0 = m0 ^ h0;
    u.l1 = m1 ^ h1;
    u.both = h0 & h1;
    u.sw = ((u.both & lt) | ~h0) & act;
    u.pop = act & ~(h0 | h1);
    return u;
}
TR_HD bool tr_lane_in(uint64_t mask, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return __builtin_amdgcn_inverse_ballot_w64(mask);
#else
    return ((mask >> lane) & 1ull) != 0ull;
#endif
}

// FLOAT TOP: what tr_uniform_test derives from a record and an octant -- which plane of each axis is the entry and which the
// exit plane, and each chosen 16-bit plane as a float -- depends on the hierarchy alone, and is the same on every trip of
// every wave of every launch that visits the node from that octant.  It is therefore done once per build and refit, for the
// top TR_TOP_LEVELS levels of the tree: eight tables, one per octant (index nx | ny << 1 | nz << 2: the axes the rays walk in
// the negative direction), each an implicit heap -- slot 0 is the root (arena node 0), the children of slot i are 2i + 1 and
// 2i + 2, a slot exists iff every node on its path is an internal node, absent slots are zero and never read -- of 64-byte
// records: the twelve planes as floats, in the operand pairs of tr_uniform_test's packed fma, and the children as the grid node
// holds them.  (float)q is exact for a 16-bit q, so the record's plane has the bits the conversion gives and
// fma(plane, a, n) is the same number.  Twelve levels: of 8, 10 and 12 the smallest whose table loop runs within 5 % of
// twelve's trips on the headline (10 levels: 88 %, profiles/r18_float_top_model.txt), and the largest allowed -- 2 MiB, half
// of one XCD's L2.
#define TR_TOP_LEVELS 12
#define TR_TOP_SLOTS ((1u << TR_TOP_LEVELS) - 1u)      // heap slots of one octant's table
struct alignas(64) tr_top_rec {
    float p[12];         // per child c: {entry x, entry y}, {exit x, exit y}, {entry z, exit z} at p[6 c ...]
    int32_t c0, c1;      // the arena indices of the children; negative: a leaf
    uint32_t pad[2];     // zero
};
static_assert(sizeof(tr_top_rec) == 64, "a record of the float top is one 64-byte line");
TR_HD uint32_t tr_octant_index(uint32_t sel_n, uint32_t sel_z) {
    return ((sel_n & 0x0400u) ? 1u : 0u) | ((sel_n & 0x04000000u) ? 2u : 0u) | ((sel_z & 2u) ? 4u : 0u);
}
// tr_uniform_octant of the rays of octant `o`
TR_HD tr_uoctant tr_octant_of_index(uint32_t o) {
    return tr_uoctant{((o & 1u) ? 0xffffu : 0u) | ((o & 2u) ? 0xffff0000u : 0u), (o & 4u) ? 16u : 0u, (o & 4u) ? 0u : 16u};
}
// the record of grid node `n` for octant `o`: tr_uniform_test's selection and conversion, statement by statement
TR_HD void tr_top_fill(tr_top_rec& t, const tr_qnode& n, uint32_t o) {
    const tr_uoctant oct = tr_octant_of_index(o);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const uint32_t x = (n.q[3 * c] ^ n.q[3 * c + 2]) & oct.mxy;
        const uint32_t e = n.q[3 * c] ^ x, f = n.q[3 * c + 2] ^ x, z = n.q[3 * c + 1];
        t.p[6 * c + 0] = (float)(e & 0xffffu); t.p[6 * c + 1] = (float)(e >> 16);
        t.p[6 * c + 2] = (float)(f & 0xffffu); t.p[6 * c + 3] = (float)(f >> 16);
        t.p[6 * c + 4] = (float)((z >> oct.she) & 0xffffu); t.p[6 * c + 5] = (float)((z >> oct.shf) & 0xffffu);
    }
    t.c0 = n.c0; t.c1 = n.c1;
    t.pad[0] = 0u; t.pad[1] = 0u;
}
// tr_uniform_test on a record of the rays' octant: the same fma per plane, the same tr_slab_hit against the same cull limit,
// the same three compares.  `p`: the record's twelve planes (on the device: in scalar registers).
template <int Q, typename P>
TR_HD void tr_top_test(const tr_ray& r, const P& p, const tr_result& res, bool& a0, bool& a1, bool& lt) {
    float tn[2], tf[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef float tr_v2 __attribute__((ext_vector_type(2)));
        const tr_v2 a = __builtin_elementwise_fma(tr_v2{p[6 * c + 0], p[6 * c + 1]}, tr_v2{r.qax, r.qay}, tr_v2{r.qnx, r.qny});
        const tr_v2 b = __builtin_elementwise_fma(tr_v2{p[6 * c + 2], p[6 * c + 3]}, tr_v2{r.qax, r.qay}, tr_v2{r.qfx, r.qfy});
        const tr_v2 d = __builtin_elementwise_fma(tr_v2{p[6 * c + 4], p[6 * c + 5]}, tr_v2{r.qaz, r.qaz2}, tr_v2{r.qnz, r.qfz});
        tn[c] = fmaxf(fmaxf(a.x, a.y), d.x);
        tf[c] = fminf(fminf(b.x, b.y), d.y);
#else
        tn[c] = fmaxf(fmaxf(fmaf(p[6 * c + 0], r.qax, r.qnx), fmaf(p[6 * c + 1], r.qay, r.qny)), fmaf(p[6 * c + 4], r.qaz, r.qnz));
        tf[c] = fminf(fminf(fmaf(p[6 * c + 2], r.qax, r.qfx), fmaf(p[6 * c + 3], r.qay, r.qfy)), fmaf(p[6 * c + 5], r.qaz, r.qfz));
#endif
    }
    const float lim = tr_cull_limit<Q>(res);
    a0 = tr_slab_hit(tn[0], tf[0], lim);
    a1 = tr_slab_hit(tn[1], tf[1], lim);
    lt = tn[1] < tn[0];
}
// The table's builders work slot by slot: the level of heap slot `slot` (the bits of slot + 1 below its leading one are the
// path from the root: 0 = child 0), and the slot's eight records from its grid node -- `qn` NULL: the slot is absent, zeros.
// `top`: 8 tables of `slots` records.
TR_HD int tr_top_level(uint32_t slot) {
    int level = 0;
    while (((slot + 1u) >> (level + 1)) != 0u) level++;
    return level;
}
TR_HD void tr_top_write_slot(tr_top_rec* top, const tr_qnode* qn, uint32_t slot, uint32_t slots) {
    for (uint32_t o = 0; o < 8u; o++) {
        tr_top_rec t;
        if (qn) tr_top_fill(t, *qn, o);
        else { for (int k = 0; k < 12; k++) t.p[k] = 0.f; t.c0 = 0; t.c1 = 0; t.pad[0] = 0u; t.pad[1] = 0u; }
        top[(size_t)o * slots + slot] = t;
    }
}
// The node of heap slot `slot`: the walk from the root (node 0) along the slot's bits.  kids(node, c0, c1) hands out a
// node's two children in the caller's numbering; a negative child is a leaf and ends the walk (-> negative: the slot is
// absent).  ONE walk for the builder's kernels (k_emit over the Karras arrays, k_update_boxes over the traversal nodes), for
// a load (tr_top_upload, over the blob's bytes on the host) and for tr_top_build_slot.
template <typename Kids>
TR_HD int32_t tr_top_walk(uint32_t slot, Kids kids) {
    const uint32_t path = slot + 1u;
    int32_t node = 0;
    for (int k = tr_top_level(slot) - 1; k >= 0 && node >= 0; k--) {
        int32_t c0, c1;
        kids(node, c0, c1);
        node = ((path >> k) & 1u) ? c1 : c0;
    }
    return node;
}
// The table as a function of the grid nodes alone: what the host simulation and the tests hold the downloaded table to.
// (The kernels build each record from the boxes they quantise themselves and a load builds it from unaligned bytes, so
// neither calls this function; they share tr_top_walk, tr_top_fill and tr_top_write_slot with it.)  A child index outside the
// `num_nodes` grid nodes ends the walk like a leaf.
TR_HD void tr_top_build_slot(tr_top_rec* top, const tr_qnode* qnodes, int64_t num_nodes, uint32_t slot, uint32_t slots) {
    const int32_t node = tr_top_walk(slot, [=](int32_t n, int32_t& c0, int32_t& c1) {
        c0 = qnodes[n].c0 < num_nodes ? qnodes[n].c0 : -1;
        c1 = qnodes[n].c1 < num_nodes ? qnodes[n].c1 : -1;
    });
    tr_top_write_slot(top, node >= 0 ? qnodes + node : nullptr, slot, slots);
}


// ---- unordered two-phase schedule (any / count / location) --------------------------------------
// Queries that do not prune by distance gain nothing from near-first order or from testing a
// leaf as soon as it is found -- and the fused trip pays for both: its Moller-Trumbore block and
// its three triangle loads run on (almost) every trip of the wave although only ~5 % of the
// lanes have a leaf to test (profiles/r01j: the texture path, TA/TD, is the busiest unit of the
// launch and costs ~18 cycles per wave-instruction however few lanes take part).  Here box-hit
// leaves are only QUEUED (per-lane LIFO of triangle slots in LDS: slot s of lane t at
// base[s * stride]); the wave tests them in a separate leaf phase that runs when it is worth a
// wave-instruction: a lane's queue is nearly full, enough lanes have something queued, or no lane
// has a node left.  Any order of the leaf tests gives the same count / hit set, so results are
// bit-identical to the fused trip and to the oracle.  The triangle's own slab interval (the
// [tn, tf] of the hit predicate) is recomputed from its vertices (tr_tri_hit: the same
// tr_tri_box + tr_slab the builder stored in the parent), so the queue holds 4 bytes per leaf.
constexpr int TR_LEAFQ = 6;
struct tr_leafq {
    int32_t* base;
    int32_t stride;
};

template <typename W>
struct tr_ustate_t {
    int32_t node;     // next internal node to visit, -1 = hierarchy exhausted
    uint32_t depth;
    W trail, owned;   // as in tr_state_t
    int32_t nq;       // queued leaves
    int32_t pe;       // a leaf test waiting for tr_drain_exact (-1 = none; tr_fold_leaf)
};

template <typename W>
TR_HD void tr_ustate_init(tr_ustate_t<W>& st) { st.node = 0; st.depth = 0; st.trail = 0; st.owned = 0; st.nq = 0; st.pe = -1; }
template <typename W>
TR_HD bool tr_udone(const tr_ustate_t<W>& st) { return st.node < 0 && st.nq == 0 && st.pe < 0; }
// a lane may visit its node only while the queue can take both children
template <typename W>
TR_HD bool tr_ucan_node(const tr_ustate_t<W>& st) { return st.node >= 0 && st.nq <= TR_LEAFQ - 2; }

// One trip of the unordered schedule.  `go_node`: this lane visits its node (tr_ucan_node);
// `leaf_phase`: WAVE-UNIFORM, the lanes that have a queued leaf pop and test one.  The node's four
// loads are issued before the leaf phase so that both fetches share one memory round trip.
// Children are entered c0 first; for ANY the nearer one first (a hit found sooner ends the ray
// sooner).
template <int Q, int K, bool STATS, bool COMPACT, typename W>
TR_HD void tr_unord_step(const tr_bvh_view& b, const tr_ray& r, bool go_node, bool leaf_phase,
                         tr_ustate_t<W>& st, tr_result& res, tr_topk<K>& top, tr_counters* cnt,
                         const tr_ring ring, const tr_leafq lq) {
    const int32_t nidx = go_node ? st.node : 0;
    const tr_i4* np = COMPACT ? reinterpret_cast<const tr_i4*>(reinterpret_cast<const char*>(b.qnodes) + ((uint32_t)nidx << 5))
                              : reinterpret_cast<const tr_i4*>(b.qnodes + nidx);
    const tr_i4 w0 = np[0], w1 = np[1];
    if (STATS && go_node) cnt->nodes++;
    bool fin = false;
    if (leaf_phase) {
        // pop one slot, fetch the triangle, evaluate the full predicate (box of the triangle ->
        // slab -> Moller-Trumbore); lanes without a queued leaf compute on record 0 and discard
        const bool gl = st.nq > 0;
        int32_t slot = 0;
        if (gl) { st.nq--; slot = lq.base[st.nq * lq.stride]; }
        tr_counters* nc = nullptr;
        const tr_tri t = tr_load_tri<false, COMPACT>(b, slot, nc);
        if (STATS && gl) cnt->tris++;
        fin = tr_fold_leaf<Q, K>(gl, r, t, slot, res, top, st.pe);   // (ANY: the first accepted hit ends the ray)
    }
    if (Q == TR_Q_ANY && fin) { st.node = -1; st.nq = 0; }
    const bool go = go_node && !fin;
    float tn0, tf0, tn1, tf1;
    tr_qnode_slabs(r, b.frame, w0, w1, tn0, tf0, tn1, tf1);
    const int32_t c0 = w1.z, c1 = w1.w;
    bool h0 = tr_slab_hit(tn0, tf0, TR_TLIM) && go;
    bool h1 = tr_slab_hit(tn1, tf1, TR_TLIM) && go;
    if (h0 && c0 < 0) { lq.base[st.nq * lq.stride] = ~c0; st.nq++; h0 = false; }
    if (h1 && c1 < 0) { lq.base[st.nq * lq.stride] = ~c1; st.nq++; h1 = false; }
    if (go) {
        if (h0 || h1) {
            const bool both = h0 && h1;
            const bool swap = (Q == TR_Q_ANY) ? ((both && tn1 < tn0) || !h0) : !h0;   // descend into c1?
            // (this schedule keeps the words as a RING of 16 nodes indexed by depth: slot = depth % 16, a push takes the
            // slot from the entry 16 levels up, which is then found by climbing.  The dense stack of the fused trip costs
            // these kernels two registers -- the 64-bit-addressing count launch a wave per SIMD -- and they have no cull
            // limit to drop entries by.)
            if (both) {
                st.trail |= (W(1) << st.depth);
                if (ring.base) {
                    const uint32_t slot = st.depth & (TR_RING - 1);
                    tr_ring_put(ring, slot, swap ? c0 : c1);
                    st.owned = (st.owned & ~(tr_ring_mask(W(0)) << slot)) | (W(1) << st.depth);
                }
            }
            st.node = swap ? c1 : c0;
            st.depth++;
        } else if (st.trail == 0) {
            st.node = -1;
        } else {
            const uint32_t j = tr_top_bit(st.trail);
            st.trail &= ~(W(1) << j);
            if (ring.base && ((st.owned >> j) & W(1))) st.node = tr_ring_get(ring, j & (TR_RING - 1));
            else st.node = tr_climb<STATS>(b, st.node, st.depth, j, cnt);
            st.depth = j + 1;
        }
    }
    if (leaf_phase) {      // (wave-uniform) the test the leaf phase left undecided
        if (tr_drain_exact<Q, K, COMPACT>(b, r, st.pe, res, top) && Q == TR_Q_ANY) { st.node = -1; st.nq = 0; }
        st.pe = -1;
    }
}

// one ray: node trips while the queue has room, a leaf test otherwise (host simulation; this is
// the schedule with the LATEST possible leaf tests, so it exercises the queue limits)
template <int Q, int K, bool STATS>
TR_HD void tr_traverse_unordered(const tr_bvh_view& b, const tr_ray& r, bool valid, tr_result& res,
                                 tr_topk<K>& top, tr_counters* cnt, const tr_ring ring, const tr_leafq lq) {
    tr_result_init(res);
    if (Q == TR_Q_LOCATION) top.init();
    if (!valid || b.num_tris < 2) return;
    tr_ustate_t<uint64_t> st;
    tr_ustate_init(st);
    while (!tr_udone(st)) {
        const bool cn = tr_ucan_node(st);
        tr_unord_step<Q, K, STATS, false, uint64_t>(b, r, cn, !cn, st, res, top, cnt, ring, lq);
        TR_CONVERGE();
    }
}

// The second traversal of a ray whose plain stack lost a far child (tr_plain_push / tr_addr_push): the whole hierarchy once more with
// the stackless walk over the exact nodes (no ring: every far child is found by climbing), `res` keeping what the first
// traversal found -- its best hit is the starting bound (closest / first), a hit ends it at once (any).  `r` needs the
// constants of tr_ray_setup_a only.
template <int Q, int K, bool STATS>
TR_HD void tr_traverse_more(const tr_bvh_view& b, const tr_ray& r, tr_result& res, tr_topk<K>& top, tr_counters* cnt) {
    if (Q == TR_Q_ANY && res.best_face >= 0) return;
    tr_state st;
    tr_state_init(st);
    while (!tr_done(st)) {
        if (tr_pending(st)) tr_leaf_step<Q, K, STATS>(b, r, st, res, top, cnt);
        else tr_node_step<Q, STATS>(b, r, st, res, cnt, tr_ring{nullptr, 0});
        TR_CONVERGE();
    }
}

// Full traversal of one ray (generic schedule: leaf phase whenever something is queued).
// The wave-level kernels run the two phases under votes instead (traverse.hip).
template <int Q, int K, bool STATS>
TR_HD void tr_traverse(const tr_bvh_view& b, const tr_ray& r, bool valid, tr_result& res,
                       tr_topk<K>& top, tr_counters* cnt, const tr_ring ring = tr_ring{nullptr, 0}) {
    tr_result_init(res);
    if (Q == TR_Q_LOCATION) top.init();
    if (!valid || b.num_tris < 2) return;   // F < 2 is handled by the brute-force kernel
    tr_state st;
    tr_state_init(st);
    while (!tr_done(st)) {
        if (tr_pending(st)) tr_leaf_step<Q, K, STATS>(b, r, st, res, top, cnt);
        else tr_node_step<Q, STATS>(b, r, st, res, cnt, ring);
        TR_CONVERGE();
    }
}
