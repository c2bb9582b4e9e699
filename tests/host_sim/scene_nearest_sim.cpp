// scene_nearest_sim.cpp -- TEST-ONLY: csrc/tr_scene_nearest.h built for the host (libscene_nearest_sim.so,
// tests/host_sim/scene_nearest_sim.py).  The per-lane query (tr_scene_near_query) over the arrays of the members' hierarchies
// (sim.SimBVH), point by point, in any visiting order, at any stack limit; and the placed box and its bound on their own
// (tr_scene_near_place, tr_scene_near_bound) for the checks of the culling proof.
// The brute force it is compared with is NOT here: scene_nearest_sim.py bakes the placed copies with scene_sim.points and
// runs the brute forces of nearest_sim and within_sim on the baked mesh.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_scene_nearest.h"

namespace {

struct Scene {
    std::vector<tr_scene_member> members;
    std::vector<tr_scene_inst> recs;
};

Scene scene_of(const void* const* nodes, const void* const* links, const void* const* tris, const int64_t* nf, int64_t nmesh,
               const int32_t* mesh_of, const float* M, int64_t ninst) {
    Scene s;
    s.members.resize((size_t)nmesh);
    for (int64_t m = 0; m < nmesh; m++) {
        s.members[(size_t)m].nodes = (const tr_node*)nodes[m]; s.members[(size_t)m].links = (const tr_link*)links[m];
        s.members[(size_t)m].tris = (const tr_tri*)tris[m]; s.members[(size_t)m].num_tris = nf[m];
    }
    s.recs.resize((size_t)ninst);
    for (int64_t k = 0; k < ninst; k++) {      // (what tr_scene_commit does)
        tr_scene_record(M + 12 * k, s.recs[(size_t)k]);
        s.recs[(size_t)k].mesh = mesh_of[k];
        if (nf[mesh_of[k]] <= 0) s.recs[(size_t)k].flags &= ~TR_SCENE_VALID;
    }
    return s;
}

}  // namespace

extern "C" {

int sim_scene_nearest_stack_capacity(void) { return TR_NEAR_STACK; }

// members as (nodes, links, tris, nf) of their hierarchies; instances: mesh_of [ninst], M [ninst, 12]; order: the order the
// instances are visited in (null: ascending); points dense [n, 3]; max_distance [n]; stack_entries: 0 = all.  closest [n, 3],
// distance [n], inst [n], tri [n]; lost [n] (may be null): some instance's first walk of point i overflowed its stack.
void sim_scene_nearest_walk(const void* const* nodes, const void* const* links, const void* const* tris, const int64_t* nf, int64_t nmesh,
                            const int32_t* mesh_of, const float* M, int64_t ninst, const int32_t* order, const float* points,
                            const float* max_distance, int64_t n, int stack_entries, float* closest, float* distance, int32_t* inst,
                            int32_t* tri, uint8_t* lost) {
    const Scene s = scene_of(nodes, links, tris, nf, nmesh, mesh_of, M, ninst);
    int32_t mem[2 * TR_NEAR_STACK];
    const tr_ring stack = {mem, 1, nullptr};
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        tr_scene_near_query(s.members.data(), s.recs.data(), (int32_t)ninst, order, p[0], p[1], p[2], max_distance[i], stack, stack_entries,
                            closest ? closest + 3 * i : nullptr, distance ? distance + i : nullptr, inst + i, tri + i, lost ? lost + i : nullptr);
    }
}

// THE BOUND on its own: boxes lo, hi [n, 3] placed by M [12] -> LO, HI [n, 3]; and, for points [n, 3], bound [n]
void sim_scene_nearest_place(const float* M, const float* lo, const float* hi, int64_t n, float* LO, float* HI) {
    tr_scene_near_map A;
    tr_scene_near_map_make(M, A);
    for (int64_t i = 0; i < n; i++)
        tr_scene_near_place(A, lo[3 * i], lo[3 * i + 1], lo[3 * i + 2], hi[3 * i], hi[3 * i + 1], hi[3 * i + 2], LO + 3 * i, HI + 3 * i);
}
void sim_scene_nearest_bound(const float* M, const float* points, const float* lo, const float* hi, int64_t n, double* bound) {
    tr_scene_near_map A;
    tr_scene_near_map_make(M, A);
    for (int64_t i = 0; i < n; i++)
        bound[i] = tr_scene_near_bound(A, points[3 * i], points[3 * i + 1], points[3 * i + 2], lo[3 * i], lo[3 * i + 1], lo[3 * i + 2], hi[3 * i],
                                       hi[3 * i + 1], hi[3 * i + 2]);
}
// the float64 squared distance of points [n, 3] to the triangles abc [n, 9] (tr_near_tri), +Inf for an inactive one
void sim_scene_nearest_d2(const float* points, const float* abc, int64_t n, double* d2) {
    for (int64_t i = 0; i < n; i++) {
        const float *p = points + 3 * i, *t = abc + 9 * i;
        d2[i] = tr_near_active(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8])
                    ? tr_near_tri(p[0], p[1], p[2], t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]).d2 : (double)INFINITY;
    }
}

}  // extern "C"

#ifdef SCENE_NEAREST_SIM_MAIN
// a stand-alone program around the same routine (for a sanitizer build of host code: g++ -fsanitize=... -DSCENE_NEAREST_SIM_MAIN).
// argv[1]: a file of int64 {nmesh, ninst, n}, then per member int64 {nn, nf}, nodes [nn] (64 B), links [nn] (8 B), tris [nf]
// (48 B); mesh_of i32 [ninst], M f32 [ninst, 12], points f32 [n, 3], max_distance f32 [n]; what a brute force expects:
// closest f32 [n, 3], distance f32 [n], instance i32 [n], tri i32 [n].  The query at argv[2] stack entries and at the whole
// stack, in both visiting orders, with every output and with the optional ones left out, into heap buffers of exactly n
// elements against the expected ones.
#include <cstdio>
#include <cstdlib>
template <typename T>
static std::vector<T> take(FILE* fp, size_t count) {
    std::vector<T> x(count);
    if (count && fread(x.data(), sizeof(T), count, fp) != count) { fprintf(stderr, "short read\n"); exit(2); }
    return x;
}
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    const int entries = atoi(argv[2]);
    const std::vector<int64_t> hd = take<int64_t>(fp, 3);
    const int64_t nmesh = hd[0], ninst = hd[1], n = hd[2];
    static_assert(sizeof(tr_node) == 64 && sizeof(tr_link) == 8 && sizeof(tr_tri) == 48, "record sizes");
    std::vector<std::vector<tr_node>> nodes((size_t)nmesh);
    std::vector<std::vector<tr_link>> links((size_t)nmesh);
    std::vector<std::vector<tr_tri>> tris((size_t)nmesh);
    std::vector<int64_t> nf((size_t)nmesh + 1, 0);
    std::vector<const void*> pn, pl, pt;
    for (int64_t m = 0; m < nmesh; m++) {
        const std::vector<int64_t> sz = take<int64_t>(fp, 2);
        nodes[(size_t)m] = take<tr_node>(fp, (size_t)sz[0]);
        links[(size_t)m] = take<tr_link>(fp, (size_t)sz[0]);
        tris[(size_t)m] = take<tr_tri>(fp, (size_t)sz[1]);
        nf[(size_t)m] = sz[1];
        pn.push_back(nodes[(size_t)m].data()); pl.push_back(links[(size_t)m].data()); pt.push_back(tris[(size_t)m].data());
    }
    const auto mesh_of = take<int32_t>(fp, ninst);
    const auto M = take<float>(fp, 12 * ninst);
    const auto pts = take<float>(fp, 3 * n), maxd = take<float>(fp, n);
    const auto closest = take<float>(fp, 3 * n), distance = take<float>(fp, n);
    const auto inst = take<int32_t>(fp, n), tri = take<int32_t>(fp, n);
    fclose(fp);
    bool ok = true;
    std::vector<int32_t> reversed((size_t)ninst);
    for (int64_t k = 0; k < ninst; k++) reversed[(size_t)k] = (int32_t)(ninst - 1 - k);
    int64_t nlost = 0, nfound = 0;
    for (int variant = 0; variant < 8; variant++) {
        const int32_t* order = (variant & 1) ? reversed.data() : nullptr;
        const int e = (variant & 2) ? 0 : entries;
        const bool all = !(variant & 4);
        std::vector<float> wc(3 * n), wd(n);
        std::vector<int32_t> wi(n), wt(n);
        std::vector<uint8_t> lost(n);
        sim_scene_nearest_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, order, pts.data(), maxd.data(), n,
                               e, all ? wc.data() : nullptr, all ? wd.data() : nullptr, wi.data(), wt.data(), lost.data());
        ok = ok && memcmp(wi.data(), inst.data(), 4 * n) == 0 && memcmp(wt.data(), tri.data(), 4 * n) == 0;
        if (all) ok = ok && memcmp(wc.data(), closest.data(), 12 * n) == 0 && memcmp(wd.data(), distance.data(), 4 * n) == 0;
        if (!variant)
            for (int64_t i = 0; i < n; i++) { nlost += lost[i]; nfound += inst[i] >= 0; }
    }
    printf("%lld points, %lld instances, %lld with a nearest triangle, stack_entries %d: %lld points overflowed a stack; closest, distance, "
           "instance and tri in both visiting orders: %s\n",
           (long long)n, (long long)ninst, (long long)nfound, entries, (long long)nlost, ok ? "same bits as the brute force" : "DIFFERENT");
    return ok ? 0 : 1;
}
#endif
