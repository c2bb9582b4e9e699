// range_sim.cpp -- TEST-ONLY: csrc/tr_range.h built for the host (librange_sim.so, tests/host_sim/range_sim.py).
// Two entries: the brute force of the per-triangle predicate tr_range_tri over every triangle of a mesh -- any, and the
// lexicographic closest (t, face index) with all its outputs: the oracle of the GPU tests -- and the walk (tr_range_query)
// over the arrays of a hierarchy (sim.SimBVH: built on the host, or downloaded from the GPU builder), ray by ray.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_range.h"

extern "C" {

int sim_range_stack_capacity(void) { return TR_RANGE_STACK; }

// vertices [nv, 3], faces [nf, 3]; rays dense [n, 3] + [n, 3]; tmin / tmax [n] or null.  Outputs [n] (loc [n, 3], uv [n, 2]):
// any, then the closest query's hit, front, tri, t, loc, uv; count[n] = accepted triangles of the ray; accepted (may be null)
// [n, cap]: their face indices in ascending order, -1 beyond the count
void sim_range_brute(const float* verts, const int32_t* faces, int64_t nf, const float* origins, const float* dirs, const float* tmin,
                     const float* tmax, int64_t n, uint8_t* any, uint8_t* hit, uint8_t* front, int32_t* tri, float* t, float* loc,
                     float* uv, int32_t* count, int32_t* accepted, int32_t cap) {
    for (int64_t i = 0; i < n; i++) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        tr_ray r;
        float lo, hi;
        bool valid = tr_ray_setup(r, o[0], o[1], o[2], d[0], d[1], d[2]);
        valid = tr_range_bounds(tmin ? tmin[i] : 0.0f, tmax ? tmax[i] : TR_TMAX, lo, hi) && valid;
        tr_range_best best;
        tr_range_init(best);
        int32_t cnt = 0;
        for (int32_t k = 0; accepted && k < cap; k++) accepted[(int64_t)cap * i + k] = -1;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            float tt;
            if (!tr_range_tri(r, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], lo, hi, tt)) continue;
            tr_range_fold(tt, (int32_t)f, (int32_t)f, best);
            if (accepted && cnt < cap) accepted[(int64_t)cap * i + cnt] = (int32_t)f;
            cnt++;
        }
        count[i] = cnt;
        any[i] = cnt > 0 ? 1 : 0;
        hit[i] = 0; front[i] = 0; tri[i] = -1; t[i] = INFINITY;
        loc[3 * i] = loc[3 * i + 1] = loc[3 * i + 2] = 0.f;
        uv[2 * i] = uv[2 * i + 1] = 0.f;
        if (cnt > 0) {
            const int32_t f = best.face;
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            hit[i] = 1; tri[i] = f; t[i] = best.t;
            front[i] = tr_hit_outputs(r, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], loc + 3 * i, uv + 2 * i) ? 1 : 0;
        }
    }
}

// the walk on (nodes, links, tris) of nf triangles; stack_entries: 0 = all, 1 .. TR_RANGE_STACK.  lost[i]: the first walk of
// ray i (of the closest query) overflowed its stack (the result then comes from the second, stackless walk)
void sim_range_walk(const void* nodes, const void* links, const void* tris, int64_t nf, const float* origins, const float* dirs,
                    const float* tmin, const float* tmax, int64_t n, int stack_entries, uint8_t* any, uint8_t* hit, uint8_t* front,
                    int32_t* tri, float* t, float* loc, float* uv, uint8_t* lost_any, uint8_t* lost) {
    tr_bvh_view v;
    memset(&v, 0, sizeof(v));
    v.nodes = (const tr_node*)nodes; v.links = (const tr_link*)links; v.tris = (const tr_tri*)tris; v.num_tris = nf;
    int32_t mem[2 * TR_RANGE_STACK];
    const tr_ring stack = {mem, 1, nullptr};
    for (int64_t i = 0; i < n; i++) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        const float lo = tmin ? tmin[i] : 0.0f, hi = tmax ? tmax[i] : TR_TMAX;
        tr_range_query<TR_Q_ANY>(v, o[0], o[1], o[2], d[0], d[1], d[2], lo, hi, stack, stack_entries, any + i, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, lost_any + i);
        tr_range_query<TR_Q_CLOSEST>(v, o[0], o[1], o[2], d[0], d[1], d[2], lo, hi, stack, stack_entries, hit + i, front + i, tri + i,
                                     t + i, loc + 3 * i, uv + 2 * i, lost + i);
    }
}

}  // extern "C"

#ifdef RANGE_SIM_MAIN
// a stand-alone program around the same routines (for a sanitizer build of host code: g++ -fsanitize=... -DRANGE_SIM_MAIN):
// the brute force on an octahedron with known answers, and the walk -- every stack limit, the second walk included -- on a
// complete binary hierarchy put together by hand over the same eight triangles, against the brute force
#include <cstdio>
int main() {
    const float vs[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const int32_t fs[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    const int nf = 8;
    std::vector<float> org, dir, lo, hi;
    // from (-3, .2, .1) along +x the octahedron is entered at t = 2.3 and left at t = 3.7
    const float bounds[6][2] = {{0.f, 1e7f}, {0.f, 3.0f}, {3.0f, 1e7f}, {3.8f, 9.f}, {0.f, 2.0f}, {NAN, 1.f}};
    for (int k = 0; k < 6; k++) { org.insert(org.end(), {-3.f, .2f, .1f}); dir.insert(dir.end(), {1.f, 0.f, 0.f}); lo.push_back(bounds[k][0]); hi.push_back(bounds[k][1]); }
    for (int x = -3; x <= 3; x++) for (int y = -3; y <= 3; y++) for (int z = -3; z <= 3; z++) {
        org.insert(org.end(), {0.3f * x, 0.3f * y, 0.3f * z});
        dir.insert(dir.end(), {0.37f * y - 0.2f, 0.41f * z + 0.1f, 0.29f * x + 0.05f});
        lo.push_back(0.1f * (x + 3)); hi.push_back(0.1f * (x + 3) + 0.4f * (y + 3));
    }
    const int64_t n = (int64_t)lo.size();
    std::vector<uint8_t> any(n), hit(n), front(n), any2(n), hit2(n), front2(n), la(n), lc(n);
    std::vector<int32_t> tri(n), tri2(n), cnt(n);
    std::vector<float> t(n), loc(3 * n), uv(2 * n), t2(n), loc2(3 * n), uv2(2 * n);
    sim_range_brute(vs, fs, nf, org.data(), dir.data(), lo.data(), hi.data(), n, any.data(), hit.data(), front.data(), tri.data(), t.data(),
                    loc.data(), uv.data(), cnt.data(), nullptr, 0);
    printf("full: t %.9g count %d; [0, 3]: t %.9g; [3, 1e7]: t %.9g front %d; [3.8, 9]: hit %d; [0, 2]: hit %d; NaN: hit %d\n", t[0], cnt[0],
           t[1], t[2], front[2], hit[3], hit[4], hit[5]);
    bool ok = cnt[0] == 2 && cnt[1] == 1 && cnt[2] == 1 && front[1] == 1 && front[2] == 0 && !hit[3] && !hit[4] && !hit[5] && t[1] < 3.f && t[2] > 3.f;
    std::vector<tr_tri> tris(nf);
    std::vector<tr_node> nodes(nf - 1);
    std::vector<tr_link> links(nf - 1);
    float blo[15][3], bhi[15][3];      // boxes of the nodes 0 .. 6 and of the leaves (7 + slot)
    for (int k = 0; k < nf; k++) {
        const float *a = vs + 3 * fs[3 * k], *b = vs + 3 * fs[3 * k + 1], *c = vs + 3 * fs[3 * k + 2];
        memset(&tris[k], 0, sizeof(tr_tri));
        tris[k].ax = a[0]; tris[k].ay = a[1]; tris[k].az = a[2]; tris[k].bx = b[0]; tris[k].by = b[1]; tris[k].bz = b[2];
        tris[k].cx = c[0]; tris[k].cy = c[1]; tris[k].cz = c[2]; tris[k].face = k;
        tris[k].esum = tr_tri_scale(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
        tr_tri_box(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], blo[7 + k], bhi[7 + k]);
    }
    for (int i = nf - 2; i >= 0; i--) {
        const int l = 2 * i + 1, r = 2 * i + 2;      // (heap numbering: 7 .. 14 are the leaves)
        memset(&nodes[i], 0, sizeof(tr_node));
        tr_node_set_box(nodes[i].box0, blo[l], bhi[l]);
        tr_node_set_box(nodes[i].box1, blo[r], bhi[r]);
        nodes[i].c0 = l < 7 ? l : ~(l - 7); nodes[i].c1 = r < 7 ? r : ~(r - 7);
        nodes[i].parent = i ? (i - 1) / 2 : -1; nodes[i].sibling = i ? ((i & 1) ? i + 1 : i - 1) : 0;
        links[i].parent = nodes[i].parent; links[i].sibling = nodes[i].sibling;
        for (int a = 0; a < 3; a++) { blo[i][a] = fminf(blo[l][a], blo[r][a]); bhi[i][a] = fmaxf(bhi[l][a], bhi[r][a]); }
    }
    int nlost = 0, nhit = 0;
    for (int entries = 0; entries <= TR_RANGE_STACK; entries++) {
        sim_range_walk(nodes.data(), links.data(), tris.data(), nf, org.data(), dir.data(), lo.data(), hi.data(), n, entries, any2.data(),
                       hit2.data(), front2.data(), tri2.data(), t2.data(), loc2.data(), uv2.data(), la.data(), lc.data());
        if (entries == 1) for (int64_t i = 0; i < n; i++) { nlost += lc[i]; nhit += hit[i]; }
        ok = ok && memcmp(any.data(), any2.data(), n) == 0 && memcmp(hit.data(), hit2.data(), n) == 0 && memcmp(front.data(), front2.data(), n) == 0 &&
             memcmp(tri.data(), tri2.data(), n * 4) == 0 && memcmp(t.data(), t2.data(), n * 4) == 0 &&
             memcmp(loc.data(), loc2.data(), n * 12) == 0 && memcmp(uv.data(), uv2.data(), n * 8) == 0;
    }
    printf("rays with a hit in range: %d of %lld; walks that overflowed a stack of one entry: %d\n", nhit, (long long)n, nlost);
    printf("walk on the hand-made hierarchy at every stack limit: %s\n", ok ? "same bits as the brute force" : "DIFFERENT");
    return ok && nhit > 0 ? 0 : 1;
}
#endif
