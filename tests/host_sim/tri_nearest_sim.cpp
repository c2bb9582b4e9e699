// tri_nearest_sim.cpp -- TEST-ONLY: csrc/tr_tri_nearest.h built for the host (libtri_nearest_sim.so, tests/host_sim/tri_nearest_sim.py).
// Three entries: one pair (tr_tn_pair: d2 in float64 and the two witness points), the brute force of it over every active
// triangle (tr_near_active) of a mesh with the lexicographic minimum (d2, face index) among those within the bound -- the
// oracle of the GPU tests --, and the walk (tr_tn_query) over the arrays of a hierarchy (sim.SimBVH: built on the host, or
// downloaded from the GPU builder), query by query.
#include <cstdint>
#include <cstring>

#include "../../trimesh-ray-optix_amd/csrc/tr_tri_nearest.h"

namespace {

tr_tris_q load_query(const float* p) {
    tr_tris_q q;
    q.px = p[0]; q.py = p[1]; q.pz = p[2]; q.qx = p[3]; q.qy = p[4]; q.qz = p[5]; q.rx = p[6]; q.ry = p[7]; q.rz = p[8];
    return q;
}

}  // namespace

extern "C" {

int sim_tri_nearest_stack_capacity(void) { return TR_NEAR_STACK; }

// query [9], face [9] (both finite): *d2, on_query [3], on_face [3] in float64
void sim_tri_nearest_pair(const float* query, const float* face, double* d2, double* on_query, double* on_face) {
    tr_tris_q q = load_query(query);
    const tr_box qb = tr_tris_box(q);
    const tr_tn_pt c = tr_tn_pair(q, qb, face[0], face[1], face[2], face[3], face[4], face[5], face[6], face[7], face[8]);
    *d2 = c.d2;
    on_query[0] = c.xx; on_query[1] = c.xy; on_query[2] = c.xz;
    on_face[0] = c.yx; on_face[1] = c.yy; on_face[2] = c.yz;
}

// vertices [nv, 3], faces [nf, 3], tri [n, 9], radii [n] or null (unbounded); tri_out [n], distance [n], closest_mesh [n, 3],
// closest_query [n, 3]
void sim_tri_nearest_brute(const float* verts, const int32_t* faces, int64_t nf, const float* tri, int64_t n, const float* radii,
                           int32_t* tri_out, float* distance, float* closest_mesh, float* closest_query) {
    for (int64_t i = 0; i < n; i++) {
        tr_tris_q q = load_query(tri + 9 * i);
        const float r = radii ? radii[i] : INFINITY;
        const bool valid = tr_tn_valid(q, r);
        const tr_box qb = tr_tris_box(q);
        const double R2 = tr_within_r2(r);
        tr_tn_pt bp = {INFINITY, 0, 0, 0, 0, 0, 0};
        int32_t bf = -1;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            if (!tr_near_active(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2])) continue;
            const tr_tn_pt p = tr_tn_pair(q, qb, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
            if (!(p.d2 <= R2)) continue;
            if (bf < 0 || p.d2 < bp.d2) { bp = p; bf = (int32_t)f; }      // (ascending f: the first of equals is the smallest index)
        }
        const float nan = tr_u2f(0x7fc00000u);
        tri_out[i] = bf;
        distance[i] = bf >= 0 ? tr_near_distance(bp.d2) : INFINITY;
        closest_mesh[3 * i] = bf >= 0 ? (float)bp.yx : nan; closest_mesh[3 * i + 1] = bf >= 0 ? (float)bp.yy : nan;
        closest_mesh[3 * i + 2] = bf >= 0 ? (float)bp.yz : nan;
        closest_query[3 * i] = bf >= 0 ? (float)bp.xx : nan; closest_query[3 * i + 1] = bf >= 0 ? (float)bp.xy : nan;
        closest_query[3 * i + 2] = bf >= 0 ? (float)bp.xz : nan;
    }
}

// the walk on (nodes, links, tris) of nf triangles; stack_entries: 0 = all, 1 .. TR_NEAR_STACK.  lost[i] (may be null): the
// first walk of query i overflowed its stack (the result then comes from the second, stackless walk)
void sim_tri_nearest_walk(const void* nodes, const void* links, const void* tris, int64_t nf, const float* tri, int64_t n,
                          const float* radii, int stack_entries, int32_t* tri_out, float* distance, float* closest_mesh,
                          float* closest_query, uint8_t* lost) {
    tr_bvh_view v;
    memset(&v, 0, sizeof(v));
    v.nodes = (const tr_node*)nodes; v.links = (const tr_link*)links; v.tris = (const tr_tri*)tris; v.num_tris = nf;
    int32_t mem[2 * TR_NEAR_STACK];
    const tr_ring stack = {mem, 1};
    for (int64_t i = 0; i < n; i++) {
        bool l = false;
        tr_tn_query(v, load_query(tri + 9 * i), radii ? radii[i] : INFINITY, stack, stack_entries, tri_out + i, distance + i,
                    closest_mesh + 3 * i, closest_query + 3 * i, &l);
        if (lost) lost[i] = l ? 1 : 0;
    }
}

}  // extern "C"
