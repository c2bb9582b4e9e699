// tris_sim.cpp -- TEST-ONLY: csrc/tr_tris.h built for the host (libtris_sim.so, tests/host_sim/tris_sim.py).
// The brute force: the predicate tr_tris_meets over every active triangle of a mesh, in face order -- counts and lists: the
// oracle of the GPU tests.  And the walk (tr_tris_query, tr_tris_rows) over the arrays of a hierarchy (sim.SimBVH: built on
// the host, or downloaded from the GPU builder), query by query.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_tris.h"

static tr_tris_q sim_tri(const float* t) {
    tr_tris_q q;
    q.px = t[0]; q.py = t[1]; q.pz = t[2]; q.qx = t[3]; q.qy = t[4]; q.qz = t[5]; q.rx = t[6]; q.ry = t[7]; q.rz = t[8];
    return q;
}

extern "C" {

int sim_tris_stack_capacity(void) { return TR_TRIS_STACK; }

// pass 1 (face == null): count [n].  pass 2: the rows of query i at offsets[i] ...  vertices [nv, 3], faces [nf, 3], tri [n, 9]
void sim_tris_brute(const float* verts, const int32_t* faces, int64_t nf, const float* tri, int64_t n, int32_t* count, const int64_t* offsets,
                    int32_t* face) {
    for (int64_t i = 0; i < n; i++) {
        const tr_tris_q q = sim_tri(tri + 9 * i);
        const bool valid = tr_tris_valid(q);
        const tr_box qb = tr_tris_box(q);
        int32_t k = 0;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            if (!tr_near_active(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2])) continue;
            if (!tr_tris_meets(q, qb, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2])) continue;
            if (face) face[offsets[i] + k] = (int32_t)f;
            k++;
        }
        if (count) count[i] = k;
    }
}

static tr_bvh_view sim_view(const void* nodes, const void* links, const void* tris, int64_t nf) {
    tr_bvh_view v;
    memset(&v, 0, sizeof(v));
    v.nodes = (const tr_node*)nodes; v.links = (const tr_link*)links; v.tris = (const tr_tri*)tris; v.num_tris = nf;
    return v;
}

// the walk on (nodes, links, tris) of nf triangles; stack_entries: 0 = all, 1 .. TR_TRIS_STACK.
// mode 0: any [n] (as 0 / 1 in out); 1: count [n] in out; 2: the fill -- count / offsets / total as tr_tris_fill takes them,
// rows into face.  lost [n] (may be null): the first walk of query i overflowed its stack.
void sim_tris_walk(const void* nodes, const void* links, const void* tris, int64_t nf, const float* tri, int64_t n, int stack_entries,
                   int mode, int32_t* out, const int32_t* count, const int64_t* offsets, int64_t total, int32_t* face, uint8_t* lost) {
    const tr_bvh_view v = sim_view(nodes, links, tris, nf);
    int32_t mem[TR_TRIS_STACK];
    const tr_ring stack = {mem, 1};
    for (int64_t i = 0; i < n; i++) {
        const tr_tris_q q = sim_tri(tri + 9 * i);
        tr_boxes_acc acc;
        acc.count = 0; acc.limit = 0; acc.key = nullptr;
        bool l = false;
        if (mode == TR_TRIS_ANY) {
            out[i] = tr_tris_query<TR_TRIS_ANY>(v, q, stack, stack_entries, acc, &l) > 0 ? 1 : 0;
        } else if (mode == TR_TRIS_COUNT) {
            out[i] = tr_tris_query<TR_TRIS_COUNT>(v, q, stack, stack_entries, acc, &l);
        } else {
            const int64_t off = offsets[i];
            acc.limit = tr_within_limit(count[i], off, total);
            if (acc.limit > 0) {
                acc.key = face + off;
                tr_tris_query<TR_TRIS_FILL>(v, q, stack, stack_entries, acc, &l);
                tr_tris_rows(face + off, acc.limit);
            }
        }
        if (lost) lost[i] = l ? 1 : 0;
    }
}

}  // extern "C"

#ifdef TRIS_SIM_MAIN
// a stand-alone program around the same routines (for a sanitizer build of host code: g++ -fsanitize=... -DTRIS_SIM_MAIN):
// the walk at every stack limit, the second walk included, on a complete binary hierarchy put together by hand over the eight
// triangles of an octahedron, against the brute force; then a fill handed the counts of smaller queries and a total cut
// short, into a buffer of exactly that many rows (the sanitizer is the guard)
#include <cstdio>
int main() {
    const float vs[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const int32_t fs[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    const int nf = 8;
    std::vector<tr_tri> tris(nf);
    std::vector<tr_node> nodes(nf - 1);
    std::vector<tr_link> links(nf - 1);
    float blo[15][3], bhi[15][3];      // boxes of the nodes 0 .. 6 and of the leaves (7 + slot)
    for (int k = 0; k < nf; k++) {
        const float *a = vs + 3 * fs[3 * k], *b = vs + 3 * fs[3 * k + 1], *cc = vs + 3 * fs[3 * k + 2];
        memset(&tris[k], 0, sizeof(tr_tri));
        tris[k].ax = a[0]; tris[k].ay = a[1]; tris[k].az = a[2]; tris[k].bx = b[0]; tris[k].by = b[1]; tris[k].bz = b[2];
        tris[k].cx = cc[0]; tris[k].cy = cc[1]; tris[k].cz = cc[2]; tris[k].face = k;
        tr_tri_box(a[0], a[1], a[2], b[0], b[1], b[2], cc[0], cc[1], cc[2], blo[7 + k], bhi[7 + k]);
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
    bool ok = true;
    int nlost = 0;
    const float sizes[5] = {0.05f, 0.125f, 0.3f, 0.75f, 3.0f};
    std::vector<int32_t> small_count;
    std::vector<int64_t> small_off;
    std::vector<float> big;
    int64_t n = 0;
    for (int k = 0; k < 5; k++) {
        std::vector<float> tri;      // one triangle per grid point, in a plane that turns with the point
        for (int x = -3; x <= 3; x++) for (int y = -3; y <= 3; y++) for (int z = -3; z <= 3; z++) {
            const float c[3] = {0.4f * x, 0.4f * y, 0.4f * z}, s = sizes[k];
            const float p[9] = {c[0] - s, c[1] - s * (float)(x & 1), c[2], c[0] + s, c[1], c[2] - s * (float)(y & 1), c[0], c[1] + s, c[2] + s * (float)(1 + (z & 1))};
            tri.insert(tri.end(), p, p + 9);
        }
        tri[0] = NAN; tri[9 + 4] = INFINITY;                                       // two invalid queries
        for (int a = 0; a < 9; a++) tri[18 + a] = tri[18 + a % 3];                  // a point: degenerate
        for (int a = 0; a < 3; a++) tri[27 + 6 + a] = tri[27 + 3 + a];              // p, q, q: a segment
        n = (int64_t)tri.size() / 9;
        std::vector<int32_t> cnt(n), any(n), wcnt(n);
        sim_tris_brute(vs, fs, nf, tri.data(), n, cnt.data(), nullptr, nullptr);
        for (int i = 0; i < 4; i++)
            if (cnt[i] != 0) { printf("size %g: query %d is invalid or degenerate and meets %d faces\n", sizes[k], i, cnt[i]); ok = false; }
        std::vector<int64_t> off(n + 1, 0);
        for (int64_t i = 0; i < n; i++) off[i + 1] = off[i] + cnt[i];
        const int64_t total = off[n];
        std::vector<int32_t> face(total + 1), wface(total + 1);
        sim_tris_brute(vs, fs, nf, tri.data(), n, nullptr, off.data(), face.data());
        if (k == 2) { small_count = cnt; small_off = off; }
        if (k == 4) big = tri;
        for (int entries = 0; entries <= TR_TRIS_STACK; entries++) {
            std::vector<uint8_t> lost(n);
            sim_tris_walk(nodes.data(), links.data(), tris.data(), nf, tri.data(), n, entries, 0, any.data(), nullptr, nullptr, 0, nullptr, nullptr);
            sim_tris_walk(nodes.data(), links.data(), tris.data(), nf, tri.data(), n, entries, 1, wcnt.data(), nullptr, nullptr, 0, nullptr, lost.data());
            sim_tris_walk(nodes.data(), links.data(), tris.data(), nf, tri.data(), n, entries, 2, nullptr, cnt.data(), off.data(), total, wface.data(), nullptr);
            for (int64_t i = 0; i < n; i++) { ok = ok && wcnt[i] == cnt[i] && any[i] == (cnt[i] > 0); if (entries == 1) nlost += lost[i]; }
            ok = ok && memcmp(face.data(), wface.data(), total * sizeof(int32_t)) == 0;
        }
        printf("size %g: %lld rows; the walk at every stack limit: %s\n", sizes[k], (long long)total, ok ? "same as the brute force" : "DIFFERENT");
        ok = ok && (k == 0 || total > 0);
    }
    printf("count walks that overflowed a stack of one entry: %d\n", nlost);
    ok = ok && nlost > 0;
    {   // misuse: counts of the queries of size 0.3 handed to a fill with those of size 3, the total cut short by three rows
        const int64_t total = small_off[n] - 3;
        // (a large triangle need not meet what a small one met: a query writes min(its own count, the count handed in) rows
        // and the ordering pass sorts the whole segment, rows that were never written -- here -1 -- included: they come first)
        std::vector<int32_t> face(total, -1);
        for (int entries = 0; entries <= 2; entries++)
            sim_tris_walk(nodes.data(), links.data(), tris.data(), nf, big.data(), n, entries, 2, nullptr, small_count.data(), small_off.data(), total,
                          face.data(), nullptr);
        int64_t written = 0;
        for (int64_t i = 0; i < n; i++)
            for (int64_t row = small_off[i]; row < small_off[i + 1] && row < total; row++) {
                written += face[row] >= 0;
                if (row > small_off[i]) ok = ok && (face[row - 1] < face[row] || (face[row - 1] == -1 && face[row] == -1));
            }
        ok = ok && written > 0;
        printf("fill with the counts of smaller queries (%lld rows, %lld written): %s\n", (long long)total, (long long)written,
               ok ? "inside its rows, ascending" : "WRONG");
    }
    return ok ? 0 : 1;
}
#endif
