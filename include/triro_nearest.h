/* triro_nearest.h -- C ABI of libtriro_nearest.so: the nearest triangle of a mesh to each of n points, on the
 * acceleration structure of libtriro_hip.so (what trimesh.proximity.closest_point answers on the CPU).
 *
 * Per point p, with d2(p, T) the squared distance to triangle T evaluated in float64 from the float32 inputs by one fixed
 * sequence of operations (csrc/tr_nearest.h has the contract):
 *   tri      = the original face index of the triangle that minimises (d2, face index) lexicographically: on exactly
 *              equal d2 the smaller face index wins, whatever the traversal order
 *   closest  = the float64 closest point on that triangle, rounded to float32
 *   distance = (float)sqrt(d2), the square root in float64; +Inf beyond the float range
 *   a point with a non-finite component, a mesh of zero triangles or one without an active triangle: tri = -1,
 *   distance = +Inf, closest = NaN
 * Zero-area triangles are the segment or point they degenerate to.  Finite inputs never give NaN.  A triangle with a NaN
 * or an infinite coordinate is INACTIVE: it offers no candidate and is never returned, exactly as no ray query of
 * libtriro_hip.so ever hits it; the other triangles answer as if it were not there.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 */
#ifndef TRIRO_NEAREST_H
#define TRIRO_NEAREST_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_NEAREST_ABI_VERSION 1
int tr_nearest_abi_version(void);

/* entries of the per-lane far-child stack (TR_NEAR_STACK of csrc/tr_nearest.h) */
int tr_nearest_stack_capacity(void);

/*
 * One launch, one point per lane.  Every element of every output given is written, invalid points included.  The call
 * never allocates and never synchronises: even the first call on a device can be captured in a graph.
 * stack_entries limits the far-child stack of a lane (results do not depend on it: a walk whose stack overflowed is
 * repeated without a stack); 0 takes the whole capacity, smaller values are for tests.
 * Refused before any device work: bvh == NULL, n < 0, d_points == NULL or d_tri == NULL with n > 0, stack_entries
 * outside 0 .. capacity, more than 2^31 - 1 blocks of 128 points.
 */
int tr_closest_point(const tr_bvh *bvh,
        const float *d_points, int64_t n,         /* [n,3] dense float32 */
        float   *d_closest,                       /* [n,3] or NULL */
        float   *d_distance,                      /* [n]   or NULL */
        int32_t *d_tri,                           /* [n] */
        int stack_entries,                        /* 0: all; 1..capacity: tests */
        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_NEAREST_H */
