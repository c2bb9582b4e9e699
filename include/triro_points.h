/* triro_points.h -- C ABI of libtriro_points.so: RayMeshIntersector.contains_points (ray_optix.py:231-279 of the
 * reference) as ONE launch on the acceleration structure of libtriro_hip.so.
 *
 * The reference answers "is p inside the mesh" with two intersects_count launches on (p, d) and (p, -d) and a handful
 * of tensor operations on the counts (ray_optix.py:238-267).  Here one kernel traces both rays of a point in the same
 * lane and writes the decision: 12 bytes in and 2 bytes out per point, no ray tensors, no count tensors.  The counts are
 * those of tr_intersects_count on the same rays, bit for bit (same ray set-up, same hit predicate).
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the device of the handle, work is enqueued on
 * `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so; libtriro_hip.so does not know about it.
 */
#ifndef TRIRO_POINTS_H
#define TRIRO_POINTS_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_POINTS_ABI_VERSION 1
int tr_points_abi_version(void);

/* 0 generic (64-bit), 1 compact, 2 deep: the instantiation a call on this handle
   takes NOW (handle + option "compact"; the rule of the count launch); -1: bvh == NULL.
   Also the init path: it allocates what tr_contains_points needs on the handle's device. */
int tr_contains_addressing(const tr_bvh *bvh);

/*
 * Per point p:
 *   in_box  = every p[k] > lo[k] and every p[k] < hi[k]   (strict; false for a NaN; true when both box pointers are NULL)
 *   c+, c-  = hit counts of the rays (p, d) and (p, -d), as tr_intersects_count returns them (non-finite rays count 0)
 *   inside  = in_box && (c+ & 1) && (c- & 1)
 *   broken  = !((c+ & 1) && (c- & 1)) && (c+ == 0 || c- == 0)
 * Every point is traced, in the box or not.  d_summary2 = {points in the box, broken points}; it is zeroed by the call
 * (also when n == 0; a 16-byte device-to-device copy from zeros the library keeps on the device) and filled by the
 * kernel.  h_summary2 == NULL: the call neither synchronises nor allocates -- it can be captured in a graph -- once
 * those zeros exist on the device: tr_contains_addressing makes them (call it when the handle is set up), and so does
 * the first tr_contains_points on a device, which must therefore not be a captured one.  Otherwise the two totals are
 * copied to the host and the stream is synchronised.
 */
int tr_contains_points(const tr_bvh *bvh,
        const float *d_points, int64_t n,        /* [n,3] dense float32               */
        const float *d_dir3,                     /* DEVICE, 3 floats: the + direction */
        const float *d_box_lo3, const float *d_box_hi3, /* DEVICE; both NULL: no box test */
        uint8_t *d_inside,                       /* [n]                               */
        uint8_t *d_broken,                       /* [n]                               */
        int32_t *d_counts,                       /* [2,n] (+d row, then -d row) or NULL */
        int64_t *d_summary2,                     /* {points in the box, broken points} */
        int64_t *h_summary2,                     /* NULL, or host copy after a sync   */
        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_POINTS_H */
