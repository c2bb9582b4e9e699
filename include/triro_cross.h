/* triro_cross.h -- C ABI of libtriro_cross.so: EVERY crossing of a ray on a per-ray interval [tmin, tmax], on the
 * acceleration structure of libtriro_hip.so: how many triangles a ray crosses within the interval, and the uncapped list of
 * them ordered along the ray (what trimesh.ray.intersects_location returns and an OptiX any-hit program with tmin / tmax
 * collects; tr_intersects_location keeps at most 32 hits of [0, 1e7] and no distance).
 *
 * Per ray (o, d) with bounds lo = tmin[i] (0 where d_tmin is NULL) and hi = tmax[i] (1e7 where d_tmax is NULL), exactly as
 * triro_range.h (csrc/tr_range.h has that contract, csrc/tr_cross.h this one):
 *   - distances are parametric (P = o + t d) and MEASURED FROM THE ORIGIN GIVEN: the ray is never anchored;
 *   - the interval is [max(lo, 0), min(hi, 1e7)], CLOSED; lo > hi is empty;
 *   - a ray with a non-finite component, a NaN bound or an empty interval crosses nothing: count 0, no rows;
 *   - triangle T is a CROSSING iff the per-triangle predicate of libtriro_range.so accepts it, with the distance t that
 *     predicate returns; a ray through a shared edge or vertex crosses exactly one owner;
 *   - count = the number of crossings (int32, uncapped);
 *   - list  = the crossings by (t, original face index) ascending (-0.0 == +0.0 is a tie, broken by the face), at rows
 *     offsets[i] .. offsets[i] + count[i]; per row face and t, and optionally front, loc and uv as tr_range_closest writes
 *     them for that triangle, and ray = i + ray_base.  The first row of a ray is tr_range_closest's answer.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 *
 * Every entry: one ray per lane.  Rays are a tr_rays as for tr_intersects_*: any strides, broadcast allowed.  d_tmin /
 * d_tmax are dense float32 [nray] or NULL.  No entry allocates and none synchronises: even the first call on a device can
 * be captured in a graph.  stack_entries limits the per-lane stack (results do not depend on it: a walk whose stack
 * overflowed is repeated without a stack); 0 takes the whole capacity, smaller values are for tests.
 * Refused before any device work (TR_ERR_INVALID_ARG): bvh == NULL, rays == NULL, nray < 0 or a shape that does not
 * multiply to it, a NULL ray pointer or a NULL required argument with nray > 0, stack_entries outside 0 .. capacity, more
 * than 2^31 - 1 blocks of 128 rays, total < 0, a NULL required row array with total > 0.
 */
#ifndef TRIRO_CROSS_H
#define TRIRO_CROSS_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_CROSS_ABI_VERSION 1
int tr_cross_abi_version(void);

/* entries of the per-lane stack (TR_CROSS_STACK of csrc/tr_cross.h) */
int tr_cross_stack_capacity(void);

/* One launch.  Every element of d_count is written, invalid rays included. */
int tr_cross_count(const tr_bvh *bvh, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        int32_t *d_count,                                 /* [nray] */
        int stack_entries,                                /* 0: all; 1..capacity: tests */
        void *stream);

/*
 * The lists, after tr_cross_count and tr_hits_scan(d_count, nray, INT32_MAX, d_offsets, ...) of libtriro_hip.so on the same
 * rays and bounds: the crossings of ray i, ordered, at rows d_offsets[i] .. d_offsets[i] + d_count[i] of d_face and d_t (and
 * the optional outputs at the same rows).  Two launches: the walk, then the ordering of each ray's rows.  d_slot is scratch
 * of `total` int32 that carries the arena slot beside the face through the ordering; it is required where d_front, d_loc3
 * or d_uv2 is given and may be NULL otherwise.  With total == 0 nothing is launched and the row arrays may be NULL.
 * Never writes a row >= total and never more than d_count[i] rows of ray i: counts and offsets that do not belong to these
 * rays and bounds (the caller's error) give wrong rows, never a write outside the arrays.
 */
int tr_cross_fill(const tr_bvh *bvh, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        const int32_t *d_count,                           /* [nray] from tr_cross_count */
        const int64_t *d_offsets,                         /* [nray] exclusive scan of d_count */
        int64_t total,                                    /* rows of the outputs */
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
#endif /* TRIRO_CROSS_H */
