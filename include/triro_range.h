/* triro_range.h -- C ABI of libtriro_range.so: ray queries on a per-ray interval [tmin, tmax], on the acceleration
 * structure of libtriro_hip.so.  Is the segment from a to b blocked, what is the first hit beyond tmin, what is the first
 * hit within tmax: what optixTrace's tmin / tmax answer and the reference never exposes (it traces [0, 1e7] always).
 *
 * Per ray (o, d) with bounds lo = tmin[i] (0 where d_tmin is NULL) and hi = tmax[i] (1e7 where d_tmax is NULL)
 * (csrc/tr_range.h has the contract):
 *   - distances are parametric (P = o + t d) and MEASURED FROM THE ORIGIN GIVEN: a range ray is never anchored;
 *   - the interval is [max(lo, 0), min(hi, 1e7)], CLOSED: a hit at exactly either end counts; lo > hi is empty: a miss;
 *   - a ray with a non-finite component or a NaN bound misses everything;
 *   - whether a hit lies in the interval is decided as its correctly rounded distance decides it: a float32 distance
 *     within 2^-10 relative of a bound is replaced by the float64-derived one before it is compared;
 *   - any: some triangle is hit within the interval.  closest: the hit that minimises (t, original face index); hit, front,
 *     tri, loc and uv as tr_intersects_closest writes them (a miss: 0, 0, -1, 0, 0), t = its distance, +Inf for a miss;
 *   - with both bounds NULL a ray that tr_intersects_* does not anchor gets the bits of tr_intersects_any / _closest.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 */
#ifndef TRIRO_RANGE_H
#define TRIRO_RANGE_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_RANGE_ABI_VERSION 1
int tr_range_abi_version(void);

/* entries of the per-lane far-child stack (TR_RANGE_STACK of csrc/tr_range.h) */
int tr_range_stack_capacity(void);

/*
 * One launch each, one ray per lane.  Rays are a tr_rays as for tr_intersects_*: any strides, broadcast allowed.
 * d_tmin / d_tmax are dense float32 [nray] or NULL.  Every element of every output given is written, invalid rays
 * included.  A call never allocates and never synchronises: even the first call on a device can be captured in a graph.
 * stack_entries limits the far-child stack of a lane (results do not depend on it: a walk whose stack overflowed is
 * repeated without a stack); 0 takes the whole capacity, smaller values are for tests.
 * Refused before any device work (TR_ERR_INVALID_ARG): bvh == NULL, rays == NULL, nray < 0 or a shape that does not
 * multiply to it, a NULL ray pointer or a NULL required output (d_hit of tr_range_any, d_tri of tr_range_closest) with
 * nray > 0, stack_entries outside 0 .. capacity, more than 2^31 - 1 blocks of 128 rays.
 */
int tr_range_any(const tr_bvh *bvh, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        uint8_t *d_hit,                                   /* [nray] */
        int stack_entries,                                /* 0: all; 1..capacity: tests */
        void *stream);

int tr_range_closest(const tr_bvh *bvh, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        int32_t *d_tri,                                   /* [nray] */
        float   *d_t,                                     /* [nray]    or NULL */
        uint8_t *d_hit,                                   /* [nray]    or NULL */
        uint8_t *d_front,                                 /* [nray]    or NULL */
        float   *d_loc3,                                  /* [nray, 3] or NULL */
        float   *d_uv2,                                   /* [nray, 2] or NULL */
        int stack_entries,
        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_RANGE_H */
