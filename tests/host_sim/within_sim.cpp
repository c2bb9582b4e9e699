// within_sim.cpp -- TEST-ONLY: csrc/tr_within.h built for the host (libwithin_sim.so, tests/host_sim/within_sim.py).
// The brute force: the per-triangle function tr_near_tri over every active triangle of a mesh, in face order, kept where
// d2 <= R2 -- counts, lists with their optional rows, and the bounded nearest (the lexicographic minimum (d2, face index) of
// the kept ones): the oracle of the GPU tests.  And the walks (tr_within_query, tr_within_rows, tr_within_closest_query) over
// the arrays of a hierarchy (sim.SimBVH: built on the host, or downloaded from the GPU builder), point by point.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_within.h"

extern "C" {

int sim_within_stack_capacity(void) { return TR_WITHIN_STACK; }

// pass 1 (face == null): count [n].  pass 2: the rows of point i at offsets[i] ..: face, and distance / closest where given.
// vertices [nv, 3], faces [nf, 3], radii [n]
void sim_within_brute(const float* verts, const int32_t* faces, int64_t nf, const float* points, int64_t n, const float* radii,
                      int32_t* count, const int64_t* offsets, int32_t* face, float* distance, float* closest) {
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        const bool valid = tr_within_valid(p[0], p[1], p[2], radii[i]);
        const double R2 = tr_within_r2(radii[i]);
        int32_t k = 0;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            if (!tr_near_active(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2])) continue;
            const tr_near_pt q = tr_near_tri(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
            if (!(q.d2 <= R2)) continue;
            if (face) {
                const int64_t row = offsets[i] + k;
                face[row] = (int32_t)f;
                if (distance) distance[row] = tr_near_distance(q.d2);
                if (closest) { closest[3 * row] = (float)q.x; closest[3 * row + 1] = (float)q.y; closest[3 * row + 2] = (float)q.z; }
            }
            k++;
        }
        if (count) count[i] = k;
    }
}

// the bounded nearest by brute force; d2 [n] (may be null): the winner's float64 squared distance, +Inf for none
void sim_within_brute_closest(const float* verts, const int32_t* faces, int64_t nf, const float* points, int64_t n, const float* radii,
                              float* closest, float* distance, int32_t* tri, double* d2) {
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        const bool valid = tr_within_valid(p[0], p[1], p[2], radii[i]);
        const double R2 = tr_within_r2(radii[i]);
        tr_near_pt bp = {INFINITY, 0, 0, 0};
        int32_t bf = -1;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            if (!tr_near_active(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2])) continue;
            const tr_near_pt q = tr_near_tri(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
            if (!(q.d2 <= R2)) continue;
            if (bf < 0 || q.d2 < bp.d2) { bp = q; bf = (int32_t)f; }      // (ascending f: the first of equals is the smallest index)
        }
        if (bf >= 0) {
            closest[3 * i] = (float)bp.x; closest[3 * i + 1] = (float)bp.y; closest[3 * i + 2] = (float)bp.z;
            distance[i] = tr_near_distance(bp.d2);
        } else {
            closest[3 * i] = closest[3 * i + 1] = closest[3 * i + 2] = tr_u2f(0x7fc00000u);
            distance[i] = INFINITY;
        }
        tri[i] = bf;
        if (d2) d2[i] = bf >= 0 ? bp.d2 : INFINITY;
    }
}

static tr_bvh_view sim_view(const void* nodes, const void* links, const void* tris, int64_t nf) {
    tr_bvh_view v;
    memset(&v, 0, sizeof(v));
    v.nodes = (const tr_node*)nodes; v.links = (const tr_link*)links; v.tris = (const tr_tri*)tris; v.num_tris = nf;
    return v;
}

// the set walk on (nodes, links, tris) of nf triangles; stack_entries: 0 = all, 1 .. TR_WITHIN_STACK.
// mode 0: any [n] (as 0 / 1 in out); 1: count [n] in out; 2: the fill -- count / offsets / total as tr_within_fill takes them,
// rows into face (slot: scratch of `total`, required with distance / closest).  lost [n] (may be null): the first walk of point
// i overflowed its stack.
void sim_within_walk(const void* nodes, const void* links, const void* tris, int64_t nf, const float* points, int64_t n,
                     const float* radii, int stack_entries, int mode, int32_t* out, const int32_t* count, const int64_t* offsets,
                     int64_t total, int32_t* face, int32_t* slot, float* distance, float* closest, uint8_t* lost) {
    const tr_bvh_view v = sim_view(nodes, links, tris, nf);
    int32_t mem[TR_WITHIN_STACK];
    const tr_ring stack = {mem, 1};
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        tr_within_acc acc;
        acc.count = 0; acc.limit = 0; acc.face = nullptr; acc.slot = nullptr;
        bool l = false;
        if (mode == TR_WITHIN_ANY) {
            out[i] = tr_within_query<TR_WITHIN_ANY>(v, p[0], p[1], p[2], radii[i], stack, stack_entries, acc, &l) > 0 ? 1 : 0;
        } else if (mode == TR_WITHIN_COUNT) {
            out[i] = tr_within_query<TR_WITHIN_COUNT>(v, p[0], p[1], p[2], radii[i], stack, stack_entries, acc, &l);
        } else {
            const int64_t off = offsets[i];
            acc.limit = tr_within_limit(count[i], off, total);
            if (acc.limit > 0) {
                acc.face = face + off; acc.slot = slot ? slot + off : nullptr;
                tr_within_query<TR_WITHIN_FILL>(v, p[0], p[1], p[2], radii[i], stack, stack_entries, acc, &l);
                tr_within_rows(v, p[0], p[1], p[2], face + off, slot ? slot + off : nullptr, acc.limit, distance ? distance + off : nullptr,
                               closest ? closest + 3 * off : nullptr);
            }
        }
        if (lost) lost[i] = l ? 1 : 0;
    }
}

// the bounded nearest walk; stack_entries: 0 = all, 1 .. TR_NEAR_STACK
void sim_within_walk_closest(const void* nodes, const void* links, const void* tris, int64_t nf, const float* points, int64_t n,
                             const float* radii, int stack_entries, float* closest, float* distance, int32_t* tri) {
    const tr_bvh_view v = sim_view(nodes, links, tris, nf);
    int32_t mem[2 * TR_NEAR_STACK];
    const tr_ring stack = {mem, 1};
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        tr_within_closest_query(v, p[0], p[1], p[2], radii[i], stack, stack_entries, closest + 3 * i, distance + i, tri + i);
    }
}

}  // extern "C"

#ifdef WITHIN_SIM_MAIN
// a stand-alone program around the same routines (for a sanitizer build of host code: g++ -fsanitize=... -DWITHIN_SIM_MAIN):
// every walk at every stack limit, the second walk included, on a complete binary hierarchy put together by hand over the
// eight triangles of an octahedron, against the brute force; then a fill handed the counts of a smaller radius and a total
// cut short, into buffers of exactly that many rows (the sanitizer is the guard)
#include <cstdio>
int main() {
    const float vs[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const int32_t fs[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    const int nf = 8;
    std::vector<float> pts = {0, 0, 0, 3, 0, 0, NAN, 0, 0, 1, 0, 0};
    for (int x = -3; x <= 3; x++) for (int y = -3; y <= 3; y++) for (int z = -3; z <= 3; z++) { pts.push_back(0.4f * x); pts.push_back(0.4f * y); pts.push_back(0.4f * z); }
    const int64_t n = (int64_t)pts.size() / 3;
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
    bool ok = true;
    int nlost = 0;
    const float radii_of[6] = {0.0f, 0.25f, 0.6f, 1.0f, INFINITY, -1.0f};
    std::vector<int32_t> small_count;
    std::vector<int64_t> small_off;
    for (int k = 0; k < 6; k++) {
        std::vector<float> rad(n, radii_of[k]);
        std::vector<int32_t> cnt(n), any(n), wcnt(n);
        sim_within_brute(vs, fs, nf, pts.data(), n, rad.data(), cnt.data(), nullptr, nullptr, nullptr, nullptr);
        std::vector<int64_t> off(n + 1, 0);
        for (int64_t i = 0; i < n; i++) off[i + 1] = off[i] + cnt[i];
        const int64_t total = off[n];
        std::vector<int32_t> face(total + 1), wface(total + 1), wslot(total + 1), bt(n), wt(n);
        std::vector<float> dist(total + 1), clo(3 * total + 3), wdist(total + 1), wclo(3 * total + 3), bc(3 * n), bd(n), wc(3 * n), wd(n);
        sim_within_brute(vs, fs, nf, pts.data(), n, rad.data(), nullptr, off.data(), face.data(), dist.data(), clo.data());
        sim_within_brute_closest(vs, fs, nf, pts.data(), n, rad.data(), bc.data(), bd.data(), bt.data(), nullptr);
        if (k == 1) { small_count = cnt; small_off = off; }
        for (int entries = 0; entries <= TR_WITHIN_STACK; entries++) {
            std::vector<uint8_t> lost(n);
            sim_within_walk(nodes.data(), links.data(), tris.data(), nf, pts.data(), n, rad.data(), entries, 0, any.data(), nullptr, nullptr, 0,
                            nullptr, nullptr, nullptr, nullptr, nullptr);
            sim_within_walk(nodes.data(), links.data(), tris.data(), nf, pts.data(), n, rad.data(), entries, 1, wcnt.data(), nullptr, nullptr, 0,
                            nullptr, nullptr, nullptr, nullptr, lost.data());
            sim_within_walk(nodes.data(), links.data(), tris.data(), nf, pts.data(), n, rad.data(), entries, 2, nullptr, cnt.data(), off.data(), total,
                            wface.data(), wslot.data(), wdist.data(), wclo.data(), nullptr);
            sim_within_walk_closest(nodes.data(), links.data(), tris.data(), nf, pts.data(), n, rad.data(), entries, wc.data(), wd.data(), wt.data());
            for (int64_t i = 0; i < n; i++) { ok = ok && wcnt[i] == cnt[i] && any[i] == (cnt[i] > 0); if (entries == 1) nlost += lost[i]; }
            ok = ok && memcmp(face.data(), wface.data(), total * sizeof(int32_t)) == 0 && memcmp(dist.data(), wdist.data(), total * sizeof(float)) == 0 &&
                 memcmp(clo.data(), wclo.data(), 3 * total * sizeof(float)) == 0 && memcmp(bt.data(), wt.data(), n * sizeof(int32_t)) == 0 &&
                 memcmp(bd.data(), wd.data(), n * sizeof(float)) == 0 && memcmp(bc.data(), wc.data(), 3 * n * sizeof(float)) == 0;
        }
        printf("r = %g: %lld rows; every walk at every stack limit: %s\n", radii_of[k], (long long)total, ok ? "same bits as the brute force" : "DIFFERENT");
    }
    printf("count walks that overflowed a stack of one entry: %d\n", nlost);
    ok = ok && nlost > 0;
    {   // misuse: counts of r = 0.25 handed to a fill at r = +Inf, the total cut short by three rows, exact-size heap buffers
        const int64_t total = small_off[n] - 3;
        std::vector<float> rad(n, INFINITY);
        std::vector<int32_t> face(total), slot(total);
        std::vector<float> dist(total), clo(3 * total);
        for (int entries = 0; entries <= 2; entries++)
            sim_within_walk(nodes.data(), links.data(), tris.data(), nf, pts.data(), n, rad.data(), entries, 2, nullptr, small_count.data(),
                            small_off.data(), total, face.data(), slot.data(), dist.data(), clo.data(), nullptr);
        for (int64_t i = 0; i < n; i++)
            for (int64_t row = small_off[i] + 1; row < small_off[i + 1] && row < total; row++) ok = ok && face[row - 1] < face[row];
        printf("fill with the counts of a smaller radius (%lld rows): %s\n", (long long)total, ok ? "inside its rows, ascending" : "WRONG");
    }
    return ok ? 0 : 1;
}
#endif
