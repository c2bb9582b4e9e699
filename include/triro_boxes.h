/* triro_boxes.h -- C ABI of libtriro_boxes.so: the faces of a mesh that meet each of n axis-aligned boxes, on the
 * acceleration structure of libtriro_hip.so (the volume query behind surface voxelisation, cropping, binning faces into a
 * grid and the broad phase of mesh against mesh).
 *
 * Per closed box [lo, hi] (six float32; csrc/tr_boxes.h has the contract):
 *   face T MEETS the box iff T is active and the closed triangle and the closed box share a point -- touching counts.  The
 *            predicate is one fixed sequence: the three box axes as exact float32 comparisons, then the triangle's plane
 *            against the box's extreme corners and the nine edge-cross-axis tests in float64, separation always strict
 *   any      = at least one face meets the box
 *   count    = how many faces meet it (int32)
 *   list     = those faces by original face index, ascending, at rows offsets[i] .. offsets[i] + count[i]; per row,
 *              optionally, inside = 1 iff all three vertices of the face lie in the box (exact comparisons)
 *   the query is valid when all six values are finite and lo <= hi on every axis (flat boxes, lines, points and +-FLT_MAX
 *   bounds included).  An invalid query, a mesh of zero triangles or one without an active triangle: any = 0, count = 0, an
 *   empty list.
 * A triangle with a NaN or an infinite coordinate is INACTIVE: never met, as in triro_nearest.h.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 *
 * Every entry: one box per lane; box i is d_lo[3 i .. 3 i + 2], d_hi[3 i .. 3 i + 2].  Every element of every output given
 * is written, invalid queries included.  No entry allocates and none synchronises: even the first call on a device can be
 * captured in a graph.  stack_entries limits the per-lane stack (results do not depend on it: a walk whose stack overflowed
 * is repeated without a stack); 0 takes the whole capacity, smaller values are for tests.  Refused before any device work:
 * bvh == NULL, n < 0, d_lo == NULL, d_hi == NULL or a required output == NULL with n > 0, stack_entries outside
 * 0 .. capacity, more than 2^31 - 1 blocks of 128 boxes, total < 0.
 */
#ifndef TRIRO_BOXES_H
#define TRIRO_BOXES_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_BOXES_ABI_VERSION 1
int tr_boxes_abi_version(void);

/* entries of the per-lane stack (TR_BOXES_STACK of csrc/tr_boxes.h) */
int tr_boxes_stack_capacity(void);

int tr_boxes_any(const tr_bvh *bvh,
        const float *d_lo, const float *d_hi,     /* [n,3] dense float32 each */
        int64_t n,
        uint8_t *d_any,                           /* [n] 0 / 1 */
        int stack_entries,                        /* 0: all; 1..capacity: tests */
        void *stream);

int tr_boxes_count(const tr_bvh *bvh, const float *d_lo, const float *d_hi, int64_t n,
        int32_t *d_count,                         /* [n] */
        int stack_entries, void *stream);

/*
 * The lists, after tr_boxes_count and tr_hits_scan(d_count, n, INT32_MAX, d_offsets, ...) of libtriro_hip.so on the same
 * boxes: the faces of box i, ascending, at rows d_offsets[i] .. d_offsets[i] + d_count[i] of d_face (and their `inside`
 * flags at the same rows of d_inside).  Two launches: the walk, then the ordering of each box's rows; no scratch.  With
 * total == 0 nothing is launched and the row arrays may be NULL.  Never writes a row >= total and never more than
 * d_count[i] rows of box i: counts and offsets that do not belong to these boxes (the caller's error) give wrong rows,
 * never a write outside the arrays.
 */
int tr_boxes_fill(const tr_bvh *bvh, const float *d_lo, const float *d_hi, int64_t n,
        const int32_t *d_count,                   /* [n] from tr_boxes_count */
        const int64_t *d_offsets,                 /* [n] exclusive scan of d_count */
        int64_t total,                            /* rows of the outputs */
        int32_t *d_face,                          /* [total] */
        uint8_t *d_inside,                        /* [total] 0 / 1, or NULL */
        int stack_entries, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_BOXES_H */
