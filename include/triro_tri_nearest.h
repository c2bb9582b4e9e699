/* triro_tri_nearest.h -- C ABI of libtriro_tri_nearest.so: the nearest face of a mesh to each of n query TRIANGLES, on the
 * acceleration structure of libtriro_hip.so: how far apart two meshes are (clearance between parts, the minimum distance of a
 * robot link to its surroundings; trimesh.collision.CollisionManager.min_distance_* on the CPU).
 *
 * Per query triangle Q = (p, q, r), with d2(Q, T) the squared distance to face T evaluated in float64 from the float32 inputs
 * by one fixed sequence of operations (csrc/tr_tri_nearest.h has the contract):
 *   d2       = the minimum over fifteen candidate pairs of points -- each vertex of one triangle against the other triangle
 *              (tr_closest_point's function), each edge of Q against each edge of T --, and 0 EXACTLY where both triangles have
 *              area and meet (tr_tris_any's predicate, triro_tris.h)
 *   tri      = the original face index of the face that minimises (d2, face index) lexicographically among the faces with
 *              d2 <= max_distance^2 (float64; a face at exactly max_distance is admitted): on exactly equal d2 the smaller face
 *              index wins, whatever the traversal order
 *   distance = (float)sqrt(d2), the square root in float64; +Inf beyond the float range
 *   closest_mesh, closest_query = the two points of the winning pair's minimal candidate, on the face and on Q, rounded to
 *              float32.  For a pair that meets they are THE NEAREST BOUNDARY FEATURES, NOT A COMMON POINT.
 *   a query with a non-finite value, a NaN or negative max_distance, a mesh of zero triangles or one without an active face,
 *   or no face within max_distance: tri = -1, distance = +Inf, both points NaN
 * A triangle without area, on either side, is the segment or point it degenerates to, and -- as in triro_tris.h -- meets
 * nothing: one that pierces the interior of the other triangle has the (positive) distance of the nearest boundary features.
 * Finite inputs never give NaN.  A face with a NaN or an infinite coordinate is INACTIVE: it is never returned.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on `stream`,
 * the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links against
 * libtriro_hip.so; libtriro_hip.so does not know about it.
 */
#ifndef TRIRO_TRI_NEAREST_H
#define TRIRO_TRI_NEAREST_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_TRI_NEAREST_ABI_VERSION 1
int tr_tri_nearest_abi_version(void);

/* entries of the per-lane far-child stack (TR_NEAR_STACK of csrc/tr_nearest.h) */
int tr_tri_nearest_stack_capacity(void);

/*
 * One launch, one query triangle per lane.  Every element of every output given is written, invalid queries included.  The
 * call never allocates and never synchronises: even the first call on a device can be captured in a graph.
 * stack_entries limits the far-child stack of a lane (results do not depend on it: a walk whose stack overflowed is repeated
 * without a stack); 0 takes the whole capacity, smaller values are for tests.
 * Refused before any device work: bvh == NULL, n < 0, d_triangles == NULL or d_tri == NULL with n > 0, stack_entries outside
 * 0 .. capacity, more than 2^31 - 1 blocks of 128 triangles.
 */
int tr_triangles_nearest(const tr_bvh *bvh,
        const float *d_triangles, int64_t n,      /* [n,9] dense float32: p, q, r */
        const float *d_max,                       /* [n], or NULL: max_distance for every query */
        float max_distance,                       /* read when d_max is NULL; +Inf: unbounded */
        int32_t *d_tri,                           /* [n] */
        float   *d_distance,                      /* [n]   or NULL */
        float   *d_closest_mesh,                  /* [n,3] or NULL */
        float   *d_closest_query,                 /* [n,3] or NULL */
        int stack_entries,                        /* 0: all; 1..capacity: tests */
        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_TRI_NEAREST_H */
