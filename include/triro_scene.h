/* triro_scene.h -- C ABI of libtriro_scene.so: ray queries over INSTANCED SCENES -- placed copies of several meshes -- on
 * the acceleration structures of libtriro_hip.so.  What OptiX answers with instance acceleration structures: a forest,
 * a warehouse of shelves, a robot's links against its surroundings, without baking every copy into one mesh, and with an
 * object moved rigidly (or by any affine map) by committing twelve floats instead of rebuilding anything.
 *
 * A SCENE refers to `nmesh` MEMBER handles (tr_bvh*, all on the scene's device, owned by the caller and alive for as long
 * as the scene is) and holds `ninst` INSTANCES: a member index and a placement M, object -> world, twelve float32,
 * row-major 3 x 4 (rows x, y, z; the fourth column is the translation).  M is any invertible affine map: scales and
 * mirrors are allowed.  The same member may be placed any number of times; one BVH serves all its copies.
 *
 * Per world ray (o, d) with bounds lo = tmin[i] (0 where d_tmin is NULL) and hi = tmax[i] (1e7 where NULL)
 * (csrc/tr_scene.h has the contract, on top of the range contract of csrc/tr_range.h):
 *   - an affine map preserves the ray parameter, so distances are the world ray's own (P = o + t d), measured from the
 *     origin given, never anchored, and comparable between instances;
 *   - W = M^-1 is computed at commit in float64 (adjugate formula) and rounded once to float32; the ray in an instance's
 *     frame is (W o, W_lin d) by a fixed sequence of fmaf;
 *   - an instance whose M has a non-finite entry or no finite inverse is hit by nothing, as is a member without triangles;
 *   - per instance the answer is that of tr_range_any / tr_range_closest for the transformed ray and the same bounds;
 *   - any: some instance is hit within the interval.  closest: the hit that minimises (t, instance index, face index);
 *     instance and tri (the face index in the MEMBER mesh) name it, uv is as in object space, loc is M applied to the
 *     object-space location, front is what the placed triangle looks like from the ray (inverted under a mirror);
 *     a miss: hit 0, front 0, instance -1, tri -1, loc 0, uv 0, t +Inf;
 *   - a ray with a non-finite component or a NaN bound misses everything; every output is written for every ray;
 *   - results do not depend on the order of traversal, on stack capacity or on launch shape.
 *
 * WHEN A COMMITTED SCENE GOES STALE.  tr_scene_commit records, per member, the device arrays of the handle (nodes, parent
 * links, triangle records), its triangle count and its device; the kernels read the members through that table.  A query
 * first compares, on the host, every member's current arrays, count and device with what was committed and refuses with
 * TR_ERR_INVALID_ARG, "scene is stale: commit it again", when one differs.
 *   Calls that KEEP a member's arrays -- the scene stays valid and shows the new geometry with the next query:
 *     tr_bvh_refit (it rewrites the triangle records and the boxes in place; the triangle count cannot change);
 *     tr_bvh_update with the SAME triangle count (the arena is reused and carved identically; the hierarchy is rebuilt in
 *     place);  every query, tr_bvh_serialize, tr_bvh_download*, tr_bvh_replica_hash, tr_bvh_get_info.
 *   Calls that MOVE them (or change the count) -- commit again:
 *     tr_bvh_update with another triangle count (the arrays are carved at other offsets of the arena, and a count beyond
 *     the arena's capacity replaces the arena); a tr_bvh_update or tr_bvh_refit that FAILED (the handle is reset to no
 *     triangles); replacing the handle: tr_bvh_destroy and a new tr_bvh_build or tr_bvh_deserialize (a load).
 *   Destroying a member while a scene still names it is the caller's error: the stale check reads the handle.
 *
 * Conventions are those of triro_hip.h: d_* are DEVICE pointers on the scene's device, work is enqueued on `stream`, the
 * return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links against
 * libtriro_hip.so; libtriro_hip.so does not know about it.
 */
#ifndef TRIRO_SCENE_H
#define TRIRO_SCENE_H

#include "triro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_SCENE_ABI_VERSION 1
int tr_scene_abi_version(void);

typedef struct tr_scene tr_scene;

typedef struct tr_scene_info_t {
    int32_t device;           /* HIP device ordinal of the scene and all its members   */
    int32_t stack_capacity;   /* entries of the per-lane far-child stack                */
    int64_t num_members;
    int64_t num_instances;
    int64_t valid_instances;  /* instances that can be hit (finite invertible M, a member with triangles) */
    int64_t table_bytes;      /* device memory owned by the scene (capacity of the table) */
    int64_t commits;          /* successful tr_scene_commit calls so far                */
} tr_scene_info_t;

/* An empty scene (no instance: every ray misses) on `device` (< 0: the current device).  Allocates nothing on the device. */
int tr_scene_create(int device, tr_scene **out);
int tr_scene_destroy(tr_scene *scene);

/*
 * (Re)define the scene from HOST arrays: members[nmesh], mesh_of_instance[ninst] (int32), M[ninst, 12] (float32).  The
 * only entry that allocates or copies: the per-instance records are computed on the host, the members' device arrays are
 * read from their handles, and ONE table is uploaded on `stream` (which is synchronised once, so the host arrays may be
 * reused on return).  The table only grows; the call is safe at any time, also between queries (a launch already
 * enqueued on another stream that still reads the table must have finished: the caller's to order, as for tr_bvh_update).
 * Refused before any device work (TR_ERR_INVALID_ARG): scene == NULL, a negative count, members == NULL with nmesh > 0,
 * mesh_of_instance or M == NULL with ninst > 0, a NULL member, a member on another device than the scene's, a member
 * index outside 0 .. nmesh - 1.  A refused commit leaves the previous scene in place; one that fails in the HIP runtime
 * while the table is uploaded leaves an empty scene (every ray misses) until the next successful commit.
 */
int tr_scene_commit(tr_scene *scene, const tr_bvh *const *members, int64_t nmesh,
        const int32_t *mesh_of_instance, const float *M, int64_t ninst, void *stream);

int tr_scene_info(const tr_scene *scene, tr_scene_info_t *info);

/*
 * One launch each, one ray per lane.  Rays are a tr_rays as for tr_intersects_*: any strides, broadcast allowed.
 * d_tmin / d_tmax are dense float32 [nray] or NULL.  Every element of every output given is written, invalid rays
 * included.  A call never allocates and never synchronises: even the first call on a scene can be captured in a graph.
 * stack_entries as for tr_range_*: 0 takes the whole capacity, smaller values are for tests (same results).
 * Refused before any device work (TR_ERR_INVALID_ARG): scene == NULL, a stale scene (see above), rays == NULL, nray < 0
 * or a shape that does not multiply to it, a NULL ray pointer or a NULL required output (d_hit of tr_scene_any, d_tri of
 * tr_scene_closest) with nray > 0, stack_entries outside 0 .. capacity, more than 2^31 - 1 blocks of 128 rays.
 */
int tr_scene_any(const tr_scene *scene, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        uint8_t *d_hit,                                   /* [nray] */
        int stack_entries,                                /* 0: all; 1..capacity: tests */
        void *stream);

int tr_scene_closest(const tr_scene *scene, const tr_rays *rays,
        const float *d_tmin, const float *d_tmax,         /* [nray] dense or NULL */
        int32_t *d_instance,                              /* [nray]    or NULL */
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
#endif /* TRIRO_SCENE_H */
