// tr_walk.h -- what the walks of the satellite queries (tr_nearest.h, tr_range.h, tr_within.h, tr_cross.h, tr_boxes.h,
// tr_tris.h and the scene walks on them) share, once: the node-id stack of a lane, the row limit of a FILL, the ordering of
// a segment of rows, the stackless re-walk and the box-culled set walk.  Host + device, as the headers that use it.  What a
// query accepts and why a subtree may be skipped stays with the query (THE CONTRACT and CULLING of its header).
#pragma once
#include "tr_bvh.h"

// NODE-ID STACK.  Entry e of a lane is word e of its column of a tr_ring (LDS on the device); sp = 2 * entries in use | lost,
// cap2 = 2 * entries the walk may use.  A push that does not fit sets the sticky lost bit and drops the node: the walk that
// ends with it set is repeated without a stack (tr_rewalk).
TR_HD bool tr_walk_lost(uint32_t sp) { return (sp & 1u) != 0; }
TR_HD void tr_walk_push(const tr_ring stack, uint32_t cap2, uint32_t& sp, int32_t node) {
    const uint32_t w = sp & ~1u;
    if (w < cap2) {
        tr_ring_put(stack, w >> 1, node);
        sp += 2u;
    } else {
        sp |= 1u;
    }
}
TR_HD int32_t tr_walk_pop(const tr_ring stack, uint32_t& sp) {
    if (sp < 2u) return -1;
    sp -= 2u;
    return tr_ring_get(stack, sp >> 1);
}

// ROW LIMIT.  The rows a query may write: [off, off + count) cut to [0, total); nothing for a negative count or an offset
// outside.
TR_HD int32_t tr_rows_limit(int32_t count, int64_t off, int64_t total) {
    if (count <= 0 || off < 0 || off >= total) return 0;
    const int64_t room = total - off;
    return (int64_t)count < room ? count : (int32_t)room;
}

// ORDERING.  m rows into ascending order, in place: rows.before(i, j) compares rows i and j, rows.swap(i, j) exchanges
// everything that rides with them.  A heapsort: no scratch, and every index it forms is below m whatever the rows hold (the
// comparisons only choose between indices already bounded by `end`) -- keys that compare false both ways (NaN) leave the
// order of such rows unspecified and the rows a permutation.
template <class R>
TR_HD void tr_rows_sift(const R rows, int32_t root, int32_t end) {
    for (;;) {
        int32_t child = 2 * root + 1;
        if (child >= end) break;
        if (child + 1 < end && rows.before(child, child + 1)) child++;
        if (!rows.before(root, child)) break;
        rows.swap(root, child);
        root = child;
    }
}
template <class R>
TR_HD void tr_rows_sort(const R rows, int32_t m) {
    for (int32_t i = m / 2 - 1; i >= 0; i--) tr_rows_sift(rows, i, m);
    for (int32_t end = m - 1; end > 0; end--) {
        rows.swap(0, end);
        tr_rows_sift(rows, 0, end);
    }
}

// THE RE-WALK.  The whole tree again without a stack, for a lane whose first walk lost a push (the caller has dropped what that
// walk found): children in fixed order, up through the parent links.  phase 0: arriving from above (child 0 next), 1: child 0
// done (child 1 next), 2: both done (climb).  Cold, correct, not fast; nothing here depends on the depth.  The query is the
// probe:
//   done()                 it has what it came for (ANY a face, FILL all its rows), or false
//   child(node, phase, c)  loads `node`, gives the id of child `phase` in c and returns whether that child survives the culling
//   leaf(slot)             evaluates the triangle in `slot`
template <class P>
TR_HD void tr_rewalk(const tr_bvh_view& b, const P& probe) {
    int32_t node = 0;
    int phase = 0;
    for (;;) {
        if (probe.done()) break;
        if (phase == 2) {
            const int32_t parent = b.links[node].parent;
            if (parent < 0) break;
            phase = b.nodes[parent].c0 == node ? 1 : 2;
            node = parent;
            continue;
        }
        int32_t c;
        const bool go = probe.child(node, phase, c);
        phase++;
        if (!go) continue;
        if (c < 0) {
            probe.leaf(~c);
        } else {
            node = c;
            phase = 0;
        }
    }
}

// THE SET WALK.  any / count / list of the faces a query accepts: the walk visits one node per call from the root
// (probe.visit(st, stack, cap2): both child boxes tested, leaf children that survive evaluated, of the internal children that
// survive one visited next and the other pushed on the node-id stack), never culls by what it has found, and ends early only
// once probe.done().  A lane that ends with the lost bit set DISCARDS its partial count / write cursor and repeats the walk
// with tr_rewalk: each walk visits a node at most once, so nothing is counted twice.  Below two triangles there is no
// hierarchy: the one triangle is tested directly.  FILL writes in walk order and never beyond acc.limit rows.
enum tr_set_mode { TR_SET_ANY = 0, TR_SET_COUNT = 1, TR_SET_FILL = 2 };
struct tr_walk_state {
    int32_t node;    // next internal node to visit, -1 = nothing left
    uint32_t sp;     // 2 * entries in use | lost
};
// the walk has what it came for: ANY a face, FILL all its rows (acc: `count` found, of which min(count, limit) were written)
template <int MODE, class A>
TR_HD bool tr_set_full(const A& acc) {
    return MODE == TR_SET_ANY ? acc.count > 0 : (MODE == TR_SET_FILL ? acc.count >= acc.limit : false);
}

// one query, start to end, on one lane (the host simulation; the kernel runs the first walk as a wave loop).  capacity: the
// entries of the stack, stack_entries: 1 .. capacity, 0 = all of them.  Returns the number of faces found (FILL: min(it,
// acc.limit) rows are written and still in walk order); *lost (may be null): the first walk overflowed its stack.
template <class P>
TR_HD int32_t tr_set_query(const tr_bvh_view& b, const P& probe, bool valid, const tr_ring stack, int stack_entries, int capacity,
                           bool* lost) {
    valid = valid && b.num_tris > 0;
    probe.acc.count = 0;
    if (lost) *lost = false;
    if (valid && b.num_tris >= 2 && !probe.done()) {
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : capacity);
        tr_walk_state st;
        st.node = 0; st.sp = 0;
        while (st.node >= 0) probe.visit(st, stack, cap2);
        if (lost) *lost = tr_walk_lost(st.sp);
        if (tr_walk_lost(st.sp) && !probe.done()) {
            probe.acc.count = 0;
            tr_rewalk(b, probe);
        }
    } else if (valid && !probe.done()) {
        probe.leaf(0);      // no hierarchy below two triangles
    }
    return probe.acc.count;
}

#if defined(__HIPCC__)
// ... and the body of its kernel: one query per lane, BS lanes per workgroup, the stack of a lane a column of LDS (STACK node
// ids: 4 x STACK x BS bytes per workgroup).  The kernel has loaded query i (valid, in_range) and built the probe on an
// accumulator without rows; FILL: the rows of the query are offsets[i] .. , at most tr_rows_limit of them, and rows(off)
// points the accumulator at them.  ANY: out8[i] = 0 / 1.  COUNT: out32[i] = the number of faces found.
template <int MODE, int STACK, class P, class R>
__device__ __forceinline__ void tr_set_kernel(const tr_bvh_view& b, const P& probe, const tr_ring stack, bool valid, bool in_range, int64_t i,
                                              const int32_t* count, const int64_t* offsets, int64_t total,
                                              const R rows, int stack_entries, uint8_t* out8,
                                              int32_t* out32) {
    probe.acc.count = 0; probe.acc.limit = 0;
    if (MODE == TR_SET_FILL && in_range) {
        const int64_t off = offsets[i];
        probe.acc.limit = tr_rows_limit(count[i], off, total);
        if (probe.acc.limit > 0) rows(off);
    }
    const bool walk = valid && !probe.done();      // (FILL: a query without rows has nothing to do)
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : STACK);
        tr_walk_state st;
        st.node = walk ? 0 : -1; st.sp = 0;
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) probe.visit(st, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_walk_lost(st.sp) && !probe.done()) {      // cold: the partial result is dropped, not added to
            probe.acc.count = 0;
            tr_rewalk(b, probe);
        }
    } else if (walk) {
        probe.leaf(0);      // no hierarchy below two triangles
    }
    if (in_range) {
        if (MODE == TR_SET_ANY) out8[i] = probe.acc.count > 0 ? 1 : 0;
        if (MODE == TR_SET_COUNT) out32[i] = probe.acc.count;
    }
}
#endif
