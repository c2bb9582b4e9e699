/* triro_planes.h -- C ABI of libtriro_planes.so: the faces of a mesh that each of n planes meets, and the segments in which a
 * plane cuts them -- the section of a mesh (slicing, contouring, cross-section measurement), on the acceleration structure of
 * libtriro_hip.so.
 *
 * Per plane (origin o, normal n: six float32, the normal not normalised; csrc/tr_planes.h has the contract):
 *   s(v)     = fma(n_z, d_z, fma(n_y, d_y, n_x * d_x)), d_k = (double)v_k - (double)o_k: the signed value of a vertex, float64
 *   face T MEETS the plane iff T is active and its vertices are neither all s > 0 nor all s < 0 -- touching counts
 *   face T is CUT iff T is active, has a vertex with s > 0 and either one with s < 0 or two with s == 0: the faces that own a
 *            row of the section, which is the boundary of the surface strictly on the positive side
 *   cut      = 0: the entry answers for MEET, 1: for CUT
 *   any      = at least one such face (uint8)
 *   count    = how many (int32)
 *   list     = those faces by original face index, ascending, at rows offsets[i] .. offsets[i] + count[i]; with cut = 1,
 *              optionally, segments = (p0, p1) per row, float32 [rows, 2, 3], directed along (face normal) x (plane normal); a
 *              crossing point is interpolated from the negative to the positive vertex of its edge, so the two faces of an
 *              edge produce the same bits
 *   the query is valid when all six values are finite and n != (0, 0, 0).  An invalid query, a mesh of zero triangles or one
 *   without an active triangle: any = 0, count = 0, an empty list.
 * A triangle with a NaN or an infinite coordinate is INACTIVE: never met, as in triro_nearest.h.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 *
 * Every entry: one wave per plane; plane i is d_origins[3 i .. 3 i + 2], d_normals[3 i .. 3 i + 2].  Every element of every
 * output given is written, invalid queries included.  No entry allocates and none synchronises: even the first call on a
 * device can be captured in a graph.  frontier_entries limits the per-wave frontier (results do not depend on it: a push that
 * does not fit is walked by its lane without a stack); 0 takes the whole capacity, smaller values are for tests.  Refused
 * before any device work: bvh == NULL, n < 0, d_origins == NULL, d_normals == NULL or a required output == NULL with n > 0,
 * cut other than 0 / 1, frontier_entries outside 0 .. capacity, more than 2^31 - 1 planes, total < 0, d_segments with cut == 0.
 */
#ifndef TRIRO_PLANES_H
#define TRIRO_PLANES_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_PLANES_ABI_VERSION 1
int tr_planes_abi_version(void);

/* entries of the per-wave frontier (TR_PLANES_FRONTIER of csrc/tr_planes.h) */
int tr_planes_frontier_capacity(void);

int tr_planes_any(const tr_bvh *bvh,
        const float *d_origins, const float *d_normals,   /* [n,3] dense float32 each */
        int64_t n,
        uint8_t *d_any,                                   /* [n] 0 / 1 */
        int cut,                                          /* 0: faces met; 1: faces cut */
        int frontier_entries,                             /* 0: all; 1..capacity: tests */
        void *stream);

int tr_planes_count(const tr_bvh *bvh, const float *d_origins, const float *d_normals, int64_t n,
        int32_t *d_count,                                 /* [n] */
        int cut, int frontier_entries, void *stream);

/*
 * The lists, after tr_planes_count and tr_hits_scan(d_count, n, INT32_MAX, d_offsets, ...) of libtriro_hip.so on the same
 * planes with the same `cut`: the faces of plane i, ascending, at rows d_offsets[i] .. d_offsets[i] + d_count[i] of d_face
 * (and, with cut = 1, their segments at the same rows of d_segments).  Two launches, the walk and the ordering of each
 * plane's rows, and one more for the segments; no scratch.  With total == 0 nothing is launched and the row arrays may be
 * NULL.  Never writes a row >= total and never more than d_count[i] rows of plane i: counts and offsets that do not belong
 * to these planes (the caller's error) give wrong rows, never a write outside the arrays.
 */
int tr_planes_fill(const tr_bvh *bvh, const float *d_origins, const float *d_normals, int64_t n,
        const int32_t *d_count,                           /* [n] from tr_planes_count */
        const int64_t *d_offsets,                         /* [n] exclusive scan of d_count */
        int64_t total,                                    /* rows of the outputs */
        int32_t *d_face,                                  /* [total] */
        float *d_segments,                                /* [total,2,3], or NULL; needs cut == 1 */
        int cut, int frontier_entries, void *stream);

/*
 * The ordering pass of tr_planes_fill on its own: the int32 keys of segment i, rows d_offsets[i] .. d_offsets[i] +
 * d_count[i] of d_key cut to [0, total), into ascending order in place, one workgroup per segment.  Words outside the
 * segments are not touched.
 */
int tr_planes_order(int device, int64_t n, const int32_t *d_count, const int64_t *d_offsets, int64_t total,
        int32_t *d_key,                                   /* [total] */
        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_PLANES_H */
