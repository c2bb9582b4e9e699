// scene_sim.cpp -- TEST-ONLY: csrc/tr_scene.h built for the host (libscene_sim.so, tests/host_sim/scene_sim.py).
// The inverse and the flags of a placement (tr_scene_record: the function tr_scene_commit runs), the ray of an instance's
// frame (tr_scene_ray), the brute force -- tr_range_tri on every triangle of every instance, reduced by (t, instance, face):
// the oracle of the GPU tests -- and the walk (tr_scene_query) over the arrays of the members' hierarchies (sim.SimBVH).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_scene.h"

namespace {

std::vector<tr_scene_inst> records(const int32_t* mesh_of, const float* M, int64_t ninst, const int64_t* nf) {
    std::vector<tr_scene_inst> recs((size_t)ninst);
    for (int64_t k = 0; k < ninst; k++) {
        tr_scene_record(M + 12 * k, recs[(size_t)k]);
        recs[(size_t)k].mesh = mesh_of[k];
        if (nf[mesh_of[k]] <= 0) recs[(size_t)k].flags &= ~TR_SCENE_VALID;
    }
    return recs;
}

}  // namespace

extern "C" {

// M [n, 12] -> W [n, 12], flags [n] (TR_SCENE_VALID | TR_SCENE_FLIP, without the member's share)
void sim_scene_record(const float* M, int64_t n, float* W, int32_t* flags) {
    for (int64_t k = 0; k < n; k++) {
        tr_scene_inst rec;
        tr_scene_record(M + 12 * k, rec);
        memcpy(W + 12 * k, rec.W, sizeof(rec.W));
        flags[k] = rec.flags;
    }
}

// rays [n, 3] + [n, 3] in the frame of the placement M [12]: o2, d2 [n, 3], ok [n] (tr_ray_setup of the transformed ray)
void sim_scene_transform(const float* M, const float* origins, const float* dirs, int64_t n, float* o2, float* d2, uint8_t* ok) {
    tr_scene_inst rec;
    tr_scene_record(M, rec);
    for (int64_t i = 0; i < n; i++) {
        tr_ray r;
        ok[i] = tr_scene_ray(rec, origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], r) ? 1 : 0;
        o2[3 * i] = r.ox; o2[3 * i + 1] = r.oy; o2[3 * i + 2] = r.oz;
        d2[3 * i] = r.dx; d2[3 * i + 1] = r.dy; d2[3 * i + 2] = r.dz;
    }
}

// points [n, 3] through the 3 x 4 map A [12] (the fmaf order of the contract)
void sim_scene_points(const float* A, const float* p, int64_t n, float* out) {
    for (int64_t i = 0; i < n; i++) tr_scene_point(A, p[3 * i], p[3 * i + 1], p[3 * i + 2], out[3 * i], out[3 * i + 1], out[3 * i + 2]);
}

// members: verts[m] -> [nv, 3], faces[m] -> [nf[m], 3]; instances: mesh_of [ninst], M [ninst, 12]; rays dense; tmin / tmax [n] or
// null.  Outputs [n] (loc [n, 3], uv [n, 2]): any, then the closest query's hit, front, instance, tri, t, loc, uv;
// count[n] = accepted (instance, triangle) pairs of the ray
void sim_scene_brute(const float* const* verts, const int32_t* const* faces, const int64_t* nf, int64_t nmesh, const int32_t* mesh_of,
                     const float* M, int64_t ninst, const float* origins, const float* dirs, const float* tmin, const float* tmax, int64_t n,
                     uint8_t* any, uint8_t* hit, uint8_t* front, int32_t* inst, int32_t* tri, float* t, float* loc, float* uv, int32_t* count) {
    (void)nmesh;
    const std::vector<tr_scene_inst> recs = records(mesh_of, M, ninst, nf);
    for (int64_t i = 0; i < n; i++) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        tr_ray rw;
        float lo, hi;
        bool valid = tr_ray_setup(rw, o[0], o[1], o[2], d[0], d[1], d[2]);
        valid = tr_range_bounds(tmin ? tmin[i] : 0.0f, tmax ? tmax[i] : TR_TMAX, lo, hi) && valid;
        float bt = INFINITY;
        int32_t bk = -1, bf = -1, cnt = 0;
        for (int64_t k = 0; valid && k < ninst; k++) {
            const tr_scene_inst& rec = recs[(size_t)k];
            if (!(rec.flags & TR_SCENE_VALID)) continue;
            tr_ray r;
            if (!tr_scene_ray(rec, o[0], o[1], o[2], d[0], d[1], d[2], r)) continue;
            const float* v = verts[rec.mesh];
            const int32_t* fs = faces[rec.mesh];
            for (int64_t f = 0; f < nf[rec.mesh]; f++) {
                const float *a = v + 3 * fs[3 * f], *b = v + 3 * fs[3 * f + 1], *c = v + 3 * fs[3 * f + 2];
                float tt;
                if (!tr_range_tri(r, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], lo, hi, tt)) continue;
                cnt++;
                // instances and faces come in ascending order: only a strictly smaller distance displaces
                if (bk < 0 || tt < bt) { bt = tt; bk = (int32_t)k; bf = (int32_t)f; }
            }
        }
        count[i] = cnt;
        any[i] = cnt > 0 ? 1 : 0;
        hit[i] = 0; front[i] = 0; inst[i] = -1; tri[i] = -1; t[i] = INFINITY;
        loc[3 * i] = loc[3 * i + 1] = loc[3 * i + 2] = 0.f;
        uv[2 * i] = uv[2 * i + 1] = 0.f;
        if (cnt > 0) {
            const tr_scene_inst& rec = recs[(size_t)bk];
            const float* v = verts[rec.mesh];
            const int32_t* fs = faces[rec.mesh] + 3 * bf;
            const float *a = v + 3 * fs[0], *b = v + 3 * fs[1], *c = v + 3 * fs[2];
            tr_ray r;
            (void)tr_scene_ray(rec, o[0], o[1], o[2], d[0], d[1], d[2], r);
            float ol[3];
            const bool fr = tr_hit_outputs(r, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], ol, uv + 2 * i);
            hit[i] = 1; inst[i] = bk; tri[i] = bf; t[i] = bt;
            front[i] = (fr != ((rec.flags & TR_SCENE_FLIP) != 0)) ? 1 : 0;
            tr_scene_point(rec.M, ol[0], ol[1], ol[2], loc[3 * i], loc[3 * i + 1], loc[3 * i + 2]);
        }
    }
}

// the walk: members as (nodes, links, tris, nf) of their hierarchies; order: the order the instances are visited in (null:
// ascending); stack_entries: 0 = all.  lost_any / lost [n]: some instance's first walk of the ray overflowed its stack
void sim_scene_walk(const void* const* nodes, const void* const* links, const void* const* tris, const int64_t* nf, int64_t nmesh,
                    const int32_t* mesh_of, const float* M, int64_t ninst, const int32_t* order, const float* origins, const float* dirs,
                    const float* tmin, const float* tmax, int64_t n, int stack_entries, uint8_t* any, uint8_t* hit, uint8_t* front,
                    int32_t* inst, int32_t* tri, float* t, float* loc, float* uv, uint8_t* lost_any, uint8_t* lost) {
    std::vector<tr_scene_member> members((size_t)nmesh);
    for (int64_t m = 0; m < nmesh; m++) {
        members[(size_t)m].nodes = (const tr_node*)nodes[m]; members[(size_t)m].links = (const tr_link*)links[m];
        members[(size_t)m].tris = (const tr_tri*)tris[m]; members[(size_t)m].num_tris = nf[m];
    }
    const std::vector<tr_scene_inst> recs = records(mesh_of, M, ninst, nf);
    int32_t mem[2 * TR_RANGE_STACK];
    const tr_ring stack = {mem, 1, nullptr};
    for (int64_t i = 0; i < n; i++) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        const float lo = tmin ? tmin[i] : 0.0f, hi = tmax ? tmax[i] : TR_TMAX;
        tr_scene_query<TR_Q_ANY>(members.data(), recs.data(), (int32_t)ninst, order, o[0], o[1], o[2], d[0], d[1], d[2], lo, hi, stack,
                                 stack_entries, any + i, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, lost_any + i);
        tr_scene_query<TR_Q_CLOSEST>(members.data(), recs.data(), (int32_t)ninst, order, o[0], o[1], o[2], d[0], d[1], d[2], lo, hi, stack,
                                     stack_entries, hit + i, front + i, inst + i, tri + i, t + i, loc + 3 * i, uv + 2 * i, lost + i);
    }
}

}  // extern "C"

#ifdef SCENE_SIM_MAIN
// a stand-alone program around the same routines (for a sanitizer build of host code: g++ -fsanitize=... -DSCENE_SIM_MAIN):
// an octahedron and a single triangle placed five times -- a translation, a mirror, a general affine map, a singular map and
// the triangle -- with known answers along one ray, and the walk on a complete binary hierarchy put together by hand, at every
// stack limit and in both visiting orders, against the brute force
#include <cstdio>
int main() {
    const float vs[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const int32_t fs[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    const float tv[9] = {8, -1, -1, 8, 1, -1, 8, 0, 1.5f};
    const int32_t tf[3] = {0, 1, 2};
    const int nf = 8;
    const float M[5 * 12] = {1, 0, 0, 4, 0, 1, 0, 0, 0, 0, 1, 0,                          // the octahedron around (4, 0, 0)
                             -2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0,                         // mirrored and doubled around the origin
                             0.5f, 0.25f, 0, 12, -0.25f, 0.5f, 0.125f, 0, 0, 0, 1, 0,     // a general map around (12, 0, 0)
                             1, 2, 3, 0, 2, 4, 6, 0, 1, 1, 1, 0,                          // singular: hit by nothing
                             1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};                         // the triangle at x = 8
    const int32_t mesh_of[5] = {0, 0, 0, 0, 1};
    const int64_t nfs[2] = {nf, 1};
    float W[60];
    int32_t flags[5];
    sim_scene_record(M, 5, W, flags);
    bool ok = flags[0] == 1 && flags[1] == 3 && flags[2] == 1 && flags[3] == 0 && flags[4] == 1 && W[3] == -4.f && W[12] == -0.5f && W[17] == 0.5f;
    std::vector<float> org, dir, lo, hi;
    // from (-5, .1, .05) along +x: the doubled octahedron is entered at x = -1.85 (t = 3.15) and left at 1.85, the first one at x = 3.15 (t = 8.15)
    const float bounds[6][2] = {{0.f, 1e7f}, {4.f, 1e7f}, {7.f, 1e7f}, {9.5f, 1e7f}, {13.5f, 14.f}, {NAN, 1.f}};
    for (int k = 0; k < 6; k++) { org.insert(org.end(), {-5.f, .1f, .05f}); dir.insert(dir.end(), {1.f, 0.f, 0.f}); lo.push_back(bounds[k][0]); hi.push_back(bounds[k][1]); }
    for (int x = -3; x <= 3; x++) for (int y = -3; y <= 3; y++) for (int z = -3; z <= 3; z++) {
        org.insert(org.end(), {4.f + 2.5f * x, 0.4f * y, 0.4f * z});
        dir.insert(dir.end(), {0.9f * y - 0.2f, 0.21f * z + 0.1f, 0.19f * x + 0.05f});
        lo.push_back(0.2f * (x + 3)); hi.push_back(0.2f * (x + 3) + 1.5f * (y + 3));
    }
    const int64_t n = (int64_t)lo.size();
    std::vector<uint8_t> any(n), hit(n), front(n), any2(n), hit2(n), front2(n), la(n), lc(n);
    std::vector<int32_t> inst(n), tri(n), inst2(n), tri2(n), cnt(n);
    std::vector<float> t(n), loc(3 * n), uv(2 * n), t2(n), loc2(3 * n), uv2(2 * n);
    const float* verts[2] = {vs, tv};
    const int32_t* faces[2] = {fs, tf};
    sim_scene_brute(verts, faces, nfs, 2, mesh_of, M, 5, org.data(), dir.data(), lo.data(), hi.data(), n, any.data(), hit.data(), front.data(),
                    inst.data(), tri.data(), t.data(), loc.data(), uv.data(), cnt.data());
    printf("full: instance %d t %.9g front %d count %d; from 4: instance %d front %d; from 7: instance %d t %.9g; from 9.5: instance %d; [13.5, 14]: hit %d; NaN: hit %d\n",
           inst[0], t[0], front[0], cnt[0], inst[1], front[1], inst[2], t[2], inst[3], hit[4], hit[5]);
    // (under the mirror the placed triangles are wound the other way: entering shows their back, leaving their front)
    ok = ok && inst[0] == 1 && front[0] == 0 && cnt[0] == 7 && inst[1] == 1 && front[1] == 1 && inst[2] == 0 && front[2] == 1 && inst[3] == 0 && t[3] > 9.5f && inst[4] == -1 &&
         !hit[4] && !hit[5] && inst[5] == -1 && t[0] > 3.1f && t[0] < 3.2f && t[2] > 8.1f && t[2] < 8.2f;
    std::vector<tr_tri> tris(nf), one(1);
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
    memset(&one[0], 0, sizeof(tr_tri));
    one[0].ax = tv[0]; one[0].ay = tv[1]; one[0].az = tv[2]; one[0].bx = tv[3]; one[0].by = tv[4]; one[0].bz = tv[5];
    one[0].cx = tv[6]; one[0].cy = tv[7]; one[0].cz = tv[8]; one[0].face = 0;
    one[0].esum = tr_tri_scale(tv[0], tv[1], tv[2], tv[3], tv[4], tv[5], tv[6], tv[7], tv[8]);
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
    const void* pn[2] = {nodes.data(), nullptr};
    const void* pl[2] = {links.data(), nullptr};
    const void* pt[2] = {tris.data(), one.data()};
    const int32_t reversed[5] = {4, 3, 2, 1, 0};
    int nlost = 0, nhit = 0;
    for (int entries = 0; entries <= TR_RANGE_STACK; entries++)
        for (int rev = 0; rev < 2; rev++) {
            sim_scene_walk(pn, pl, pt, nfs, 2, mesh_of, M, 5, rev ? reversed : nullptr, org.data(), dir.data(), lo.data(), hi.data(), n, entries,
                           any2.data(), hit2.data(), front2.data(), inst2.data(), tri2.data(), t2.data(), loc2.data(), uv2.data(), la.data(), lc.data());
            if (entries == 1 && !rev) for (int64_t i = 0; i < n; i++) { nlost += lc[i]; nhit += hit[i]; }
            ok = ok && memcmp(any.data(), any2.data(), n) == 0 && memcmp(hit.data(), hit2.data(), n) == 0 && memcmp(front.data(), front2.data(), n) == 0 &&
                 memcmp(inst.data(), inst2.data(), n * 4) == 0 && memcmp(tri.data(), tri2.data(), n * 4) == 0 && memcmp(t.data(), t2.data(), n * 4) == 0 &&
                 memcmp(loc.data(), loc2.data(), n * 12) == 0 && memcmp(uv.data(), uv2.data(), n * 8) == 0;
        }
    printf("rays with a hit in range: %d of %lld; rays with a walk that overflowed a stack of one entry: %d\n", nhit, (long long)n, nlost);
    printf("walk on the hand-made hierarchies at every stack limit, both visiting orders: %s\n", ok ? "same bits as the brute force" : "DIFFERENT");
    return ok && nhit > 0 ? 0 : 1;
}
#endif
