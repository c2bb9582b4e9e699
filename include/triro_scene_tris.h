/* triro_scene_tris.h -- C ABI of libtriro_scene_tris.so: triangle queries on an INSTANCED SCENE (triro_scene.h): the (instance,
 * face) pairs of the placed copies that meet each of n world triangles.  What tr_tris_any / tr_tris_count / tr_tris_fill
 * (triro_tris.h) answer on one mesh, on placed copies of several meshes without baking them into one: does this part collide
 * with its surroundings and where, a robot's links against a cell, contact pairs of a moving mesh -- and a moved copy costs a
 * commit, not a rebuild.
 *
 * Per world triangle Q = (p, q, r) (nine float32; csrc/tr_scene_tris.h has the contract, on those of csrc/tr_scene_nearest.h
 * and csrc/tr_tris.h):
 *   - the placed vertices of a face of valid instance k are the float32 results of the scene's own placement chain (three fmaf
 *     per coordinate, the chain that produces `loc` of the ray queries) on its float32 vertices; a placed triangle with a
 *     non-finite coordinate -- the member's was, or the placement overflowed -- is never met, nor is anything of an instance
 *     without a finite inverse or of a member without triangles;
 *   - the pair (instance, face) MEETS Q iff the predicate of libtriro_tris.so says so on Q and the placed float32 vertices:
 *     both triangles have area (the placed one as placed) and the closed triangles share a point, touching included;
 *   - any   = at least one pair meets Q;
 *   - count = the number of pairs that meet it over all instances (int32; more than 2^31 - 1 pairs of one query are outside the
 *     contract);
 *   - list  = the pairs by (instance index, face index in the MEMBER mesh) ascending, at rows offsets[i] .. offsets[i] +
 *     count[i] of d_instance and d_face;
 *   - a query with a NaN or an infinity or without area, and an empty scene: any = 0, count = 0, no rows; every element of
 *     every output given is written;
 *   - the answers equal tr_tris_any / tr_tris_count / tr_tris_fill on the mesh that concatenates, in instance order, the faces
 *     of every valid instance with vertices placed by that chain, (instance, face) being the baked face index through the
 *     instance offsets; one instance at the identity gives tr_tris_* of that mesh (negative-zero coordinates included: no
 *     output carries the sign of a zero);
 *   - results do not depend on the order of traversal, on stack capacity or on launch shape.
 *
 * Conventions are those of triro_hip.h and triro_scene.h: d_* are DEVICE pointers on the scene's device, work is enqueued
 * on `stream`, the return value is a tr_status and tr_last_error() (of libtriro_hip.so) has the message.  The library links
 * against libtriro_hip.so and reads the committed table of a tr_scene of libtriro_scene.so, which it never changes.
 *
 * Every entry: one query per lane, query i is d_tri[9 i .. 9 i + 8] = p, q, r; linear in the number of instances.  No entry
 * allocates and none synchronises: even the first call on a scene can be captured in a graph.  stack_entries limits the
 * per-lane stack (results do not depend on it: a lane whose stack overflowed in an instance walks that instance again without
 * a stack); 0 takes the whole capacity, smaller values are for tests.
 * Refused before any device work (TR_ERR_INVALID_ARG): scene == NULL, a stale scene ("scene is stale: commit it again",
 * triro_scene.h), n < 0, d_tri == NULL or a required output == NULL with n > 0, stack_entries outside 0 .. capacity, more than
 * 2^31 - 1 blocks of 128 queries, total < 0, a NULL row array with total > 0.
 */
#ifndef TRIRO_SCENE_TRIS_H
#define TRIRO_SCENE_TRIS_H

#include "triro_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TR_SCENE_TRIS_ABI_VERSION 1
int tr_scene_tris_abi_version(void);

/* entries of the per-lane stack (TR_TRIS_STACK of csrc/tr_tris.h) */
int tr_scene_tris_stack_capacity(void);

int tr_scene_tris_any(const tr_scene *scene,
        const float *d_tri,                               /* [n,9] dense float32 (equivalently [n,3,3]), world space */
        int64_t n,
        uint8_t *d_any,                                   /* [n] 0 / 1 */
        int stack_entries,                                /* 0: all; 1..capacity: tests */
        void *stream);

int tr_scene_tris_count(const tr_scene *scene, const float *d_tri, int64_t n,
        int32_t *d_count,                                 /* [n] */
        int stack_entries, void *stream);

/*
 * The lists, after tr_scene_tris_count and tr_hits_scan(d_count, n, INT32_MAX, d_offsets, ...) of libtriro_hip.so on the same
 * queries: the pairs of query i, ascending by (instance, face), at rows d_offsets[i] .. d_offsets[i] + d_count[i] of
 * d_instance and d_face.  Two launches: the walk, then the ordering of each query's rows; no scratch.  With total == 0 nothing
 * is launched and the row arrays may be NULL.
 * Never writes a row >= total and never more than d_count[i] rows of query i: counts and offsets that do not belong to these
 * queries (the caller's error) give wrong rows, never a write outside the arrays.
 */
int tr_scene_tris_fill(const tr_scene *scene, const float *d_tri, int64_t n,
        const int32_t *d_count,                           /* [n] from tr_scene_tris_count */
        const int64_t *d_offsets,                         /* [n] exclusive scan of d_count */
        int64_t total,                                    /* rows of the outputs */
        int32_t *d_instance,                              /* [total] */
        int32_t *d_face,                                  /* [total]: the face index in the member mesh */
        int stack_entries, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIRO_SCENE_TRIS_H */
