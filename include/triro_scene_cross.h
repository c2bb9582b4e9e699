/* triro_scene_cross.h -- C ABI of libtriro_scene_cross.so: EVERY crossing of a world ray over an INSTANCED SCENE
 * (triro_scene.h) on a per-ray interval [tmin, tmax]: how many (instance, triangle) pairs a ray crosses within the interval,
 * and the uncapped list of them ordered along the ray.  What tr_cross_count / tr_cross_fill (triro_cross.h) answer on one
 * mesh, on placed copies of several meshes without baking them into one: transparency, x-ray thickness, crossing parity,
 * "what lies between these two points", trimesh.ray.intersects_location / intersects_id(multiple_hits=True) on a scene.
 *
 * Per world ray (o, d) with bounds lo = tmin[i] (0 where d_tmin is NULL) and hi = tmax[i] (1e7 where d_tmax is NULL)
 * (csrc/tr_scene_cross.h has the contract, on those of csrc/tr_scene.h and csrc/tr_cross.h):
 *   - the world ray and its bounds are checked once, as for tr_scene_any: a ray with a non-finite component, a NaN bound or
 *     an empty interval crosses nothing: count 0, no rows;
 *   - the ray in an instance's frame is (W o, W_lin d) as for tr_scene_any; the bounds are not transformed; an instance
 *     without a finite inverse and a member without triangles are crossed by nothing;
 *   - a CROSSING is a pair (instance, face of its member) that the per-triangle predicate of libtriro_range.so accepts for
 *     the transformed ray, with the distance t that predicate returns, unchanged (an affine map preserves the ray parameter);
 *   - count = the number of crossings over all instances (int32; more than 2^31 - 1 crossings of one ray are outside the
 *     contract);
 *   - list  = the crossings by (t, instance index, face index) ascending (-0.0 == +0.0 is a tie in t), at rows
 *     offsets[i] .. offsets[i] + count[i]; per row instance, face (the index in the MEMBER mesh) and t, and optionally
 *     front, loc and uv as tr_scene_closest writes them for that (instance, triangle), and ray = i + ray_base;
 *   - count > 0 is tr_scene_any's answer and the first row of a ray is tr_scene_closest's; one instance at the identity
 *     gives the rows of tr_cross_fill (for rays without a negative-zero component);
 *   - results do not depend on the order of traversal, on stack capacity or on launch shape.
 *
 * Conventions are those of triro_hip.h and triro_scene.h: d_* are DEVICE pointers on the scene's device, work is enqueued
 * on `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so and reads the committed table of a tr_scene of libtriro_scene.so, which it never changes.
 *
 * Every entry: one ray per lane.  Rays are a tr_rays as for tr_intersects_*: any strides, broadcast allowed.  d_tmin /
 * d_tmax are dense float32 [nray] or NULL.  No entry allocates and none synchronises: even the first call on a scene can be
 * captured in a graph.  stack_entries limits the per-lane stack (results do not depend on it: an instance's walk whose stack
 * overflowed is repeated without a stack); 0 takes the whole capacity, smaller values are for tests.
 * Refused before any device work (TR_ERR_INVALID_ARG): scene == NULL, a stale scene ("scene is stale: commit it again",
 * triro_scene.h), rays == NULL, nray < 0 or a shape that does not multiply to it, a NULL ray pointer or a NULL required
 * argument with nray > 0, stack_entries outside 0 .. capacity, more than 2^31 - 1 blocks of 128 rays, total < 0, a NULL
 * required row array with total > 0.
 */
#ifndef TRIRO_SCENE_CROSS_H
#define TRIRO_SCENE_CROSS_H

#include "triro_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_SCENE_CROSS_ABI_VERSION 1
int tr_scene_cross_abi_version(void);

/* entries of the per-lane stack (TR_CROSS_STACK of csrc/tr_cross.h) */
int tr_scene_cross_stack_capacity(void);

/* One launch.  Every element of d_count is written, invalid rays included. */
int tr_scene_cross_count(const tr_scene *scene, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        int32_t *d_count,                                 /* [nray] */
        int stack_entries,                                /* 0: all; 1..capacity: tests */
        void *stream);

/*
 * The lists, after tr_scene_cross_count and tr_hits_scan(d_count, nray, INT32_MAX, d_offsets, ...) of libtriro_hip.so on
 * the same rays and bounds: the crossings of ray i, ordered, at rows d_offsets[i] .. d_offsets[i] + d_count[i] of
 * d_instance, d_face and d_t (and the optional outputs at the same rows).  Two launches: the walk, then the ordering of each
 * ray's rows.  d_slot is scratch of `total` int32 that carries the arena slot beside the face through the ordering; it is
 * required where d_front, d_loc3 or d_uv2 is given and may be NULL otherwise.  With total == 0 nothing is launched and the
 * row arrays may be NULL.
 * Never writes a row >= total and never more than d_count[i] rows of ray i: counts and offsets that do not belong to these
 * rays and bounds (the caller's error) give wrong rows, never a write outside the arrays.
 */
int tr_scene_cross_fill(const tr_scene *scene, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        const int32_t *d_count,                           /* [nray] from tr_scene_cross_count */
        const int64_t *d_offsets,                         /* [nray] exclusive scan of d_count */
        int64_t total,                                    /* rows of the outputs */
        int32_t *d_instance,                              /* [total] */
        int32_t *d_face,                                  /* [total] */
        float   *d_t,                                     /* [total] */
        uint8_t *d_front,                                 /* [total]    or NULL */
        float   *d_loc3,                                  /* [total, 3] or NULL */
        float   *d_uv2,                                   /* [total, 2] or NULL */
        int64_t *d_ray,                                   /* [total]    or NULL: the ray of each row, + ray_base */
        int64_t ray_base,
        int32_t *d_slot,                                  /* [total] scratch; NULL allowed without d_front, d_loc3 and d_uv2 */
        int stack_entries, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_SCENE_CROSS_H */
