/* triro_scene_nearest.h -- C ABI of libtriro_scene_nearest.so: closest_point on an INSTANCED SCENE (triro_scene.h): the nearest
 * placed triangle to a world point, which placed copy it belongs to, the closest point and the distance.  What
 * tr_closest_point (triro_nearest.h) and tr_within_closest (triro_within.h) answer on one mesh, on placed copies of several
 * meshes without baking them into one: clearance checks, the distance field of an assembly, snapping a point cloud to the
 * nearest part -- and a moved part costs a commit, not a rebuild.
 *
 * Per world point p (csrc/tr_scene_nearest.h has the contract, on those of csrc/tr_scene.h and csrc/tr_nearest.h):
 *   - the placed vertices of a triangle of valid instance k are the float32 results of the scene's own placement chain
 *     (three fmaf per coordinate, the chain that produces `loc` of the ray queries) on its float32 vertices; a placed triangle
 *     with a non-finite coordinate -- the member's was, or the placement overflowed -- offers no candidate, nor does an
 *     instance without a finite inverse or a member without triangles;
 *   - the squared distance to a placed triangle is the float64 sequence of tr_closest_point on those float32 vertices;
 *   - the winner minimises (squared distance, instance, face index in the member mesh) lexicographically among the placed
 *     triangles within max_distance (squared distance <= max_distance^2 in float64: one at exactly max_distance is within);
 *     max_distance = +Inf: unbounded; NaN or negative: nothing is accepted;
 *   - closest = the float64 closest point on the placed triangle rounded to float32, in world space; distance = the float32
 *     square root as tr_closest_point takes it;
 *   - a point with a non-finite component, an empty scene, or no accepted candidate: instance -1, tri -1, distance +Inf,
 *     closest NaN; every element of every output given is written;
 *   - the answer equals tr_closest_point (tr_within_closest under a bounded max_distance) on the mesh that concatenates, in
 *     instance order, the faces of every valid instance with vertices placed by that chain, bit for bit; one instance at the
 *     identity is tr_closest_point of that mesh (for meshes without a negative-zero coordinate);
 *   - results do not depend on the order of traversal, on stack capacity or on launch shape.
 *
 * Conventions are those of triro_hip.h and triro_scene.h: d_* are DEVICE pointers on the scene's device, work is enqueued
 * on `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so and reads the committed table of a tr_scene of libtriro_scene.so, which it never changes.
 *
 * One launch, one point per lane, linear in the number of instances.  The entry never allocates and never synchronises: even
 * the first call on a scene can be captured in a graph.  stack_entries limits the per-lane stack (results do not depend on
 * it: a lane whose stack overflowed in an instance walks that instance again without a stack); 0 takes the whole capacity,
 * smaller values are for tests.
 * Refused before any device work (TR_ERR_INVALID_ARG): scene == NULL, a stale scene ("scene is stale: commit it again",
 * triro_scene.h), n < 0, more than 2^31 - 1 blocks of 128 points, a NULL d_points, d_instance or d_tri with n > 0,
 * stack_entries outside 0 .. capacity.
 */
#ifndef TRIRO_SCENE_NEAREST_H
#define TRIRO_SCENE_NEAREST_H

#include "triro_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_SCENE_NEAREST_ABI_VERSION 1
int tr_scene_nearest_abi_version(void);

/* entries of the per-lane stack (TR_NEAR_STACK of csrc/tr_nearest.h) */
int tr_scene_nearest_stack_capacity(void);

int tr_scene_closest_point(const tr_scene *scene,
        const float *d_points,                            /* [n, 3] dense */
        int64_t n,
        const float *d_max_distance,                      /* [n], or NULL: max_distance for every point */
        float max_distance,                               /* read when d_max_distance is NULL; +Inf: unbounded */
        float *d_closest,                                 /* [n, 3] or NULL */
        float *d_distance,                                /* [n] or NULL */
        int32_t *d_instance,                              /* [n] */
        int32_t *d_tri,                                   /* [n]: the face index in the member mesh */
        int stack_entries,                                /* 0: all; 1..capacity: tests */
        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_SCENE_NEAREST_H */
