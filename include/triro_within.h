/* triro_within.h -- C ABI of libtriro_within.so: the faces of a mesh within a distance r of each of n points, on the
 * acceleration structure of libtriro_hip.so (what trimesh.proximity.nearby_faces and a closest_point with a maximum
 * distance answer on the CPU).
 *
 * Per point p and radius r (float32), with d2(p, T) the float64 squared distance of libtriro_nearest.so (triro_nearest.h;
 * csrc/tr_nearest.h has its contract, csrc/tr_within.h this one) and R2 = (double)r * (double)r, an exact product:
 *   face T is WITHIN iff T is active and d2(p, T) <= R2 -- not strict: a face at exactly r is within
 *   any      = at least one face is within
 *   count    = how many faces are within (int32)
 *   list     = those faces by original face index, ascending, at rows offsets[i] .. offsets[i] + count[i]; per row,
 *              optionally, distance = (float)sqrt(d2) and closest = the float64 closest point rounded to float32,
 *              exactly what tr_closest_point gives for that face
 *   bounded nearest = the face within that minimises (d2, face index) lexicographically: tr_closest_point's answer, bit
 *              for bit, where that answer's float64 d2 <= R2 (the float32 distance <= r does not imply it), else no face
 *   the query is valid when p is finite and r >= 0 (-0.0 and +Inf included; r = 0 keeps the faces that contain p, r = +Inf
 *   every active face).  An invalid query, a mesh of zero triangles or one without an active triangle: any = 0, count = 0,
 *   an empty list, and for the bounded nearest tri = -1, distance = +Inf, closest = NaN.
 * A triangle with a NaN or an infinite coordinate is INACTIVE: never within, as in triro_nearest.h.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 *
 * Every entry: one point per lane; the radius of point i is d_radius[i] where d_radius is given, else `radius`.  Every
 * element of every output given is written, invalid queries included.  No entry allocates and none synchronises: even
 * the first call on a device can be captured in a graph.  stack_entries limits the per-lane stack (results do not depend
 * on it: a walk whose stack overflowed is repeated without a stack); 0 takes the whole capacity, smaller values are for
 * tests.  Refused before any device work: bvh == NULL, n < 0, d_points == NULL or a required output == NULL with n > 0,
 * stack_entries outside 0 .. capacity, more than 2^31 - 1 blocks of 128 points, total < 0.
 */
#ifndef TRIRO_WITHIN_H
#define TRIRO_WITHIN_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_WITHIN_ABI_VERSION 1
int tr_within_abi_version(void);

/* entries of the per-lane stack of any / count / fill (TR_WITHIN_STACK of csrc/tr_within.h); tr_within_closest takes up to
 * tr_nearest_stack_capacity() */
int tr_within_stack_capacity(void);

int tr_within_any(const tr_bvh *bvh,
        const float *d_points, int64_t n,         /* [n,3] dense float32 */
        const float *d_radius,                    /* [n] dense or NULL */
        float radius,                             /* used where d_radius is NULL */
        uint8_t *d_any,                           /* [n] 0 / 1 */
        int stack_entries,                        /* 0: all; 1..capacity: tests */
        void *stream);

int tr_within_count(const tr_bvh *bvh, const float *d_points, int64_t n, const float *d_radius, float radius,
        int32_t *d_count,                         /* [n] */
        int stack_entries, void *stream);

/*
 * The lists, after tr_within_count and tr_hits_scan(d_count, n, INT32_MAX, d_offsets, ...) of libtriro_hip.so on the same
 * points and radii: the faces of point i, ascending, at rows d_offsets[i] .. d_offsets[i] + d_count[i] of d_face (and the
 * optional outputs at the same rows).  Two launches: the walk, then the ordering of each point's rows.  d_slot is scratch
 * of `total` int32 that carries the arena slot beside the face through the ordering; it is required where d_distance or
 * d_closest3 is given and may be NULL otherwise.  With total == 0 nothing is launched and the row arrays may be NULL.
 * Never writes a row >= total and never more than d_count[i] rows of point i: counts and offsets that do not belong to
 * these points and radii (the caller's error) give wrong rows, never a write outside the arrays.
 */
int tr_within_fill(const tr_bvh *bvh, const float *d_points, int64_t n, const float *d_radius, float radius,
        const int32_t *d_count,                   /* [n] from tr_within_count */
        const int64_t *d_offsets,                 /* [n] exclusive scan of d_count */
        int64_t total,                            /* rows of the outputs */
        int32_t *d_face,                          /* [total] */
        float   *d_distance,                      /* [total]   or NULL */
        float   *d_closest3,                      /* [total,3] or NULL */
        int32_t *d_slot,                          /* [total] scratch; NULL allowed without d_distance and d_closest3 */
        int stack_entries, void *stream);

/* tr_closest_point bounded by the radius from the first node: outputs as there, (-1, +Inf, NaN) where no face is within */
int tr_within_closest(const tr_bvh *bvh, const float *d_points, int64_t n, const float *d_radius, float radius,
        float   *d_closest,                       /* [n,3] or NULL */
        float   *d_distance,                      /* [n]   or NULL */
        int32_t *d_tri,                           /* [n] */
        int stack_entries,                        /* 0: all; 1..tr_nearest_stack_capacity() */
        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_WITHIN_H */
