/* triro_scene_points.h -- C ABI of libtriro_scene_points.so: contains_points on an INSTANCED SCENE (triro_scene.h): which
 * placed copies of the member meshes hold a point -- any, how many, and the ascending list of their indices.  What
 * tr_contains_points (triro_points.h) answers on one mesh, on placed copies of several meshes without baking them into one:
 * occupancy, CSG-style classification, voxelising an assembly, labelling a point cloud by part.
 *
 * Per world point p, with ONE world direction d per call (csrc/tr_scene_points.h has the contract, on those of
 * csrc/tr_scene.h, csrc/tr_cross.h and csrc/tr_points.h):
 *   - per valid instance k, c+ is the number of faces of its member that the ray (W p, W_lin d) crosses under the default
 *     bounds [0, 1e7] -- tr_scene_cross_count of a scene that holds instance k alone -- and c- the same for (p, -d), -d being
 *     the exact negation of the world direction, taken before the transform;
 *   - p is INSIDE instance k iff c+ and c- are both odd (the parity rule of tr_contains_points); there is no box test, no
 *     `broken` output and no retry direction: an open member contains nothing on the side where one of the two rays escapes;
 *   - a point or a direction with a non-finite component is inside nothing; a transformed ray that leaves the float32 range
 *     is not inside that instance; an instance without a finite inverse and a member without triangles contain nothing;
 *   - any = inside some instance; count = the number of containing instances; list = their indices ascending, uncapped, at
 *     rows offsets[i] .. offsets[i] + count[i];
 *   - any == (count > 0); the list of a point is the set of instances in which the rows of tr_scene_cross_fill on (p, d) and
 *     on (p, -d) each hold an odd number of rows; one instance at the identity gives the parity of tr_cross_count on (p, +-d)
 *     of that mesh (for points and a direction without a negative-zero component);
 *   - results do not depend on the order of traversal, on stack capacity or on launch shape.
 *
 * Conventions are those of triro_hip.h and triro_scene.h: d_* are DEVICE pointers on the scene's device, work is enqueued
 * on `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so and reads the committed table of a tr_scene of libtriro_scene.so, which it never changes.
 *
 * Every entry: one launch, one point per lane.  d_points is dense float32 [n, 3], d_dir3 three float32.  No entry allocates
 * and none synchronises: even the first call on a scene can be captured in a graph.  stack_entries limits the per-lane stack
 * (results do not depend on it: a pass whose stack overflowed is repeated without a stack); 0 takes the whole capacity,
 * smaller values are for tests.
 * Refused before any device work (TR_ERR_INVALID_ARG): scene == NULL, a stale scene ("scene is stale: commit it again",
 * triro_scene.h), n < 0, more than 2^31 - 1 blocks of 128 points, a NULL required argument with n > 0, total < 0, a NULL
 * d_instance with total > 0, stack_entries outside 0 .. capacity.
 */
#ifndef TRIRO_SCENE_POINTS_H
#define TRIRO_SCENE_POINTS_H

#include "triro_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_SCENE_POINTS_ABI_VERSION 1
int tr_scene_points_abi_version(void);

/* entries of the per-lane stack (TR_CROSS_STACK of csrc/tr_cross.h) */
int tr_scene_points_stack_capacity(void);

/* Every element of d_any (0 or 1) is written, invalid points included.  A point is finished by its first instance. */
int tr_scene_points_any(const tr_scene *scene,
        const float *d_points,                            /* [n, 3] dense */
        int64_t n,
        const float *d_dir3,                              /* [3] */
        uint8_t *d_any,                                   /* [n] */
        int stack_entries,                                /* 0: all; 1..capacity: tests */
        void *stream);

/* Every element of d_count is written, invalid points included. */
int tr_scene_points_count(const tr_scene *scene, const float *d_points, int64_t n, const float *d_dir3,
        int32_t *d_count,                                 /* [n] */
        int stack_entries, void *stream);

/*
 * The lists, after tr_scene_points_count and tr_hits_scan(d_count, n, INT32_MAX, d_offsets, ...) of libtriro_hip.so on the
 * same points and direction: the instances that hold point i, ascending, at rows d_offsets[i] .. d_offsets[i] + d_count[i]
 * of d_instance.  With total == 0 nothing is launched and d_instance may be NULL.
 * Never writes a row >= total and never more than d_count[i] rows of point i: counts and offsets that do not belong to
 * these points and this direction (the caller's error) give wrong rows, never a write outside the array.
 */
int tr_scene_points_fill(const tr_scene *scene, const float *d_points, int64_t n, const float *d_dir3,
        const int32_t *d_count,                           /* [n] from tr_scene_points_count */
        const int64_t *d_offsets,                         /* [n] exclusive scan of d_count */
        int64_t total,                                    /* rows of d_instance */
        int32_t *d_instance,                              /* [total] */
        int stack_entries, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_SCENE_POINTS_H */
