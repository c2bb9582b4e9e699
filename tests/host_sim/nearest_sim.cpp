// nearest_sim.cpp -- TEST-ONLY: csrc/tr_nearest.h built for the host (libnearest_sim.so, tests/host_sim/nearest_sim.py).
// Two entries: the brute force of the per-triangle function tr_near_tri over every active triangle (tr_near_active: all nine
// coordinates finite) of a mesh with the lexicographic minimum (d2, face index) -- the oracle of the GPU tests -- and the walk (tr_near_query) over the arrays
// of a hierarchy (sim.SimBVH: built on the host, or downloaded from the GPU builder), point by point.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_nearest.h"

extern "C" {

int sim_nearest_stack_capacity(void) { return TR_NEAR_STACK; }

// vertices [nv, 3], faces [nf, 3]; closest [n, 3], distance [n], tri [n]
void sim_nearest_brute(const float* verts, const int32_t* faces, int64_t nf, const float* points, int64_t n, float* closest,
                       float* distance, int32_t* tri) {
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        const bool valid = tr_near_valid(p[0], p[1], p[2]);
        double best = INFINITY;
        tr_near_pt bp = {INFINITY, 0, 0, 0};
        int32_t bf = -1;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            if (!tr_near_active(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2])) continue;
            const tr_near_pt q = tr_near_tri(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
            if (bf < 0 || q.d2 < best) { best = q.d2; bp = q; bf = (int32_t)f; }      // (ascending f: the first of equals is the smallest index)
        }
        if (bf >= 0) {
            closest[3 * i] = (float)bp.x; closest[3 * i + 1] = (float)bp.y; closest[3 * i + 2] = (float)bp.z;
            distance[i] = tr_near_distance(bp.d2);
        } else {
            closest[3 * i] = closest[3 * i + 1] = closest[3 * i + 2] = tr_u2f(0x7fc00000u);
            distance[i] = INFINITY;
        }
        tri[i] = bf;
    }
}

// the walk on (nodes, links, tris) of nf triangles; stack_entries: 0 = all, 1 .. TR_NEAR_STACK.  lost[i] (may be null): the
// first walk of point i overflowed its stack (the result then comes from the second, stackless walk)
void sim_nearest_walk(const void* nodes, const void* links, const void* tris, int64_t nf, const float* points, int64_t n,
                      int stack_entries, float* closest, float* distance, int32_t* tri, uint8_t* lost) {
    tr_bvh_view v;
    memset(&v, 0, sizeof(v));
    v.nodes = (const tr_node*)nodes; v.links = (const tr_link*)links; v.tris = (const tr_tri*)tris; v.num_tris = nf;
    int32_t mem[2 * TR_NEAR_STACK];
    const tr_ring stack = {mem, 1};
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        tr_near_query(v, p[0], p[1], p[2], stack, stack_entries, closest + 3 * i, distance + i, tri + i);
        if (lost) {
            // the same first walk again, only to report whether it overflowed
            lost[i] = 0;
            if (tr_near_valid(p[0], p[1], p[2]) && nf >= 2) {
                tr_near_best best;
                tr_near_init(best);
                tr_near_state st;
                st.node = 0; st.sp = 0;
                const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
                while (st.node >= 0) tr_near_visit(v, p[0], p[1], p[2], st, best, stack, cap2);
                lost[i] = tr_near_lost(st.sp) ? 1 : 0;
            }
        }
    }
}

}  // extern "C"

#ifdef NEAREST_SIM_MAIN
// a stand-alone program around the same routines (for a sanitizer build of host code: g++ -fsanitize=... -DNEAREST_SIM_MAIN):
// the brute force on an octahedron with known answers, and the walk -- every stack limit, the second walk included -- on a
// complete binary hierarchy put together by hand over the same eight triangles, against the brute force
#include <cstdio>
int main() {
    const float vs[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const int32_t fs[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    const int nf = 8;
    std::vector<float> pts = {0, 0, 0, 3, 0, 0, NAN, 0, 0};
    for (int x = -3; x <= 3; x++) for (int y = -3; y <= 3; y++) for (int z = -3; z <= 3; z++) { pts.push_back(0.4f * x); pts.push_back(0.4f * y); pts.push_back(0.4f * z); }
    const int64_t n = (int64_t)pts.size() / 3;
    std::vector<float> c(3 * n), d(n), c2(3 * n), d2(n);
    std::vector<int32_t> t(n), t2(n);
    sim_nearest_brute(vs, fs, nf, pts.data(), n, c.data(), d.data(), t.data());
    printf("centre: tri %d distance %.9g; beyond +x: tri %d distance %.9g closest %g %g %g; nan: tri %d\n", t[0], d[0], t[1], d[1],
           c[3], c[4], c[5], t[2]);
    bool ok = t[0] == 0 && d[1] == 2.0f && c[3] == 1.0f && t[1] == 0 && t[2] == -1;
    // a complete binary tree: node i < 3 has the nodes 2 i + 1 and 2 i + 2, node i >= 3 the leaves 2 (i - 3) and 2 (i - 3) + 1
    std::vector<tr_tri> tris(nf);
    std::vector<tr_node> nodes(nf - 1);
    std::vector<tr_link> links(nf - 1);
    float lo[15][3], hi[15][3];      // boxes of the nodes 0 .. 6 and of the leaves (7 + slot)
    for (int k = 0; k < nf; k++) {
        const float *a = vs + 3 * fs[3 * k], *b = vs + 3 * fs[3 * k + 1], *cc = vs + 3 * fs[3 * k + 2];
        memset(&tris[k], 0, sizeof(tr_tri));
        tris[k].ax = a[0]; tris[k].ay = a[1]; tris[k].az = a[2]; tris[k].bx = b[0]; tris[k].by = b[1]; tris[k].bz = b[2];
        tris[k].cx = cc[0]; tris[k].cy = cc[1]; tris[k].cz = cc[2]; tris[k].face = k;
        tr_tri_box(a[0], a[1], a[2], b[0], b[1], b[2], cc[0], cc[1], cc[2], lo[7 + k], hi[7 + k]);
    }
    for (int i = nf - 2; i >= 0; i--) {
        const int l = 2 * i + 1, r = 2 * i + 2;      // (heap numbering: 7 .. 14 are the leaves)
        memset(&nodes[i], 0, sizeof(tr_node));
        tr_node_set_box(nodes[i].box0, lo[l], hi[l]);
        tr_node_set_box(nodes[i].box1, lo[r], hi[r]);
        nodes[i].c0 = l < 7 ? l : ~(l - 7); nodes[i].c1 = r < 7 ? r : ~(r - 7);
        nodes[i].parent = i ? (i - 1) / 2 : -1; nodes[i].sibling = i ? ((i & 1) ? i + 1 : i - 1) : 0;
        links[i].parent = nodes[i].parent; links[i].sibling = nodes[i].sibling;
        for (int a = 0; a < 3; a++) { lo[i][a] = fminf(lo[l][a], lo[r][a]); hi[i][a] = fmaxf(hi[l][a], hi[r][a]); }
    }
    std::vector<uint8_t> lost(n);
    sim_nearest_walk(nodes.data(), links.data(), tris.data(), nf, pts.data(), n, 1, c2.data(), d2.data(), t2.data(), lost.data());
    int nlost = 0;
    for (int64_t i = 0; i < n; i++) nlost += lost[i];
    printf("walks that overflowed a stack of one entry: %d of %lld\n", nlost, (long long)n);
    ok = ok && nlost > 0;
    for (int entries = 0; entries <= TR_NEAR_STACK; entries++) {
        sim_nearest_walk(nodes.data(), links.data(), tris.data(), nf, pts.data(), n, entries, c2.data(), d2.data(), t2.data(), nullptr);
        ok = ok && memcmp(c.data(), c2.data(), c.size() * sizeof(float)) == 0 && memcmp(d.data(), d2.data(), d.size() * sizeof(float)) == 0 &&
             memcmp(t.data(), t2.data(), t.size() * sizeof(int32_t)) == 0;
    }
    printf("walk on the hand-made hierarchy at every stack limit: %s\n", ok ? "same bits as the brute force" : "DIFFERENT");
    return ok ? 0 : 1;
}
#endif
