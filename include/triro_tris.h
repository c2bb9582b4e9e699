/* triro_tris.h -- C ABI of libtriro_tris.so: the faces of a mesh that meet each of n query triangles, on the acceleration
 * structure of libtriro_hip.so (the narrow phase of mesh against mesh: collision, interference checks, contact pairs; the
 * broad phase is triro_boxes.h).
 *
 * Per query triangle Q = (p, q, r) (nine float32; csrc/tr_tris.h has the contract):
 *   face T MEETS Q iff T is active, both triangles have area and the closed triangles share a point -- touching counts.  The
 *            predicate is one fixed sequence: the three coordinate axes as exact float32 comparisons, then seventeen
 *            separating axes in float64 (the two normals, the nine edge cross products, the six in-plane edge normals),
 *            separation always strict
 *   any      = at least one face meets Q
 *   count    = how many faces meet it (int32)
 *   list     = those faces by original face index, ascending, at rows offsets[i] .. offsets[i] + count[i]
 *   the query is valid when all nine values are finite.  A triangle, on either side, whose float64 normal is exactly 0 is
 *   DEGENERATE: such a face is never met and such a query meets nothing (unlike the box query, which accepts segments and
 *   points).  An invalid or degenerate query, a mesh of zero triangles or one without an active face with area: any = 0,
 *   count = 0, an empty list.
 * A triangle with a NaN or an infinite coordinate is INACTIVE: never met, as in triro_nearest.h.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 *
 * Every entry: one query per lane; query i is d_tri[9 i .. 9 i + 8] = p, q, r.  Every element of every output given is
 * written, invalid queries included.  No entry allocates and none synchronises: even the first call on a device can be
 * captured in a graph.  stack_entries limits the per-lane stack (results do not depend on it: a walk whose stack overflowed
 * is repeated without a stack); 0 takes the whole capacity, smaller values are for tests.  Refused before any device work:
 * bvh == NULL, n < 0, d_tri == NULL or a required output == NULL with n > 0, stack_entries outside 0 .. capacity, more than
 * 2^31 - 1 blocks of 128 queries, total < 0.
 */
#ifndef TRIRO_TRIS_H
#define TRIRO_TRIS_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_TRIS_ABI_VERSION 1
int tr_tris_abi_version(void);

/* entries of the per-lane stack (TR_TRIS_STACK of csrc/tr_tris.h) */
int tr_tris_stack_capacity(void);

int tr_tris_any(const tr_bvh *bvh,
        const float *d_tri,                       /* [n,9] dense float32 (equivalently [n,3,3]) */
        int64_t n,
        uint8_t *d_any,                           /* [n] 0 / 1 */
        int stack_entries,                        /* 0: all; 1..capacity: tests */
        void *stream);

int tr_tris_count(const tr_bvh *bvh, const float *d_tri, int64_t n,
        int32_t *d_count,                         /* [n] */
        int stack_entries, void *stream);

/*
 * The lists, after tr_tris_count and tr_hits_scan(d_count, n, INT32_MAX, d_offsets, ...) of libtriro_hip.so on the same
 * queries: the faces of query i, ascending, at rows d_offsets[i] .. d_offsets[i] + d_count[i] of d_face.  Two launches: the
 * walk, then the ordering of each query's rows; no scratch.  With total == 0 nothing is launched and d_face may be NULL.
 * Never writes a row >= total and never more than d_count[i] rows of query i: counts and offsets that do not belong to
 * these queries (the caller's error) give wrong rows, never a write outside the array.
 */
int tr_tris_fill(const tr_bvh *bvh, const float *d_tri, int64_t n,
        const int32_t *d_count,                   /* [n] from tr_tris_count */
        const int64_t *d_offsets,                 /* [n] exclusive scan of d_count */
        int64_t total,                            /* rows of the output */
        int32_t *d_face,                          /* [total] */
        int stack_entries, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_TRIS_H */
