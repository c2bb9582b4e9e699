// scene_tris_sim.cpp -- TEST-ONLY: csrc/tr_scene_tris.h built for the host (libscene_tris_sim.so,
// tests/host_sim/scene_tris_sim.py).  The per-lane query (tr_scene_tris_query, tr_scene_tris_rows) over the arrays of the
// members' hierarchies (sim.SimBVH), triangle by triangle, in any visiting order, at any stack limit; and the culling test and
// the predicate on placed vertices on their own (tr_scene_tris_apart, tr_tris_meets) for the checks of the culling proof.
// The brute force it is compared with is NOT here: scene_tris_sim.py bakes the placed copies with scene_nearest_sim.bake and
// runs tris_sim.brute on the baked mesh.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_scene_tris.h"

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

tr_tris_q sim_tri(const float* t) {
    tr_tris_q q;
    q.px = t[0]; q.py = t[1]; q.pz = t[2]; q.qx = t[3]; q.qy = t[4]; q.qz = t[5]; q.rx = t[6]; q.ry = t[7]; q.rz = t[8];
    return q;
}

}  // namespace

extern "C" {

int sim_scene_tris_stack_capacity(void) { return TR_TRIS_STACK; }

// members as (nodes, links, tris, nf) of their hierarchies; instances: mesh_of [ninst], M [ninst, 12]; order: the order the
// instances are visited in (null: ascending); tri dense [n, 9]; stack_entries: 0 = all.
// mode 0: any [n] (as 0 / 1 in out); 1: count [n] in out; 2: the fill -- count / offsets / total as tr_scene_tris_fill takes
// them, rows into inst and face.  lost [n] (may be null): some instance's first walk of query i overflowed its stack.
void sim_scene_tris_walk(const void* const* nodes, const void* const* links, const void* const* tris, const int64_t* nf, int64_t nmesh,
                         const int32_t* mesh_of, const float* M, int64_t ninst, const int32_t* order, const float* tri, int64_t n,
                         int stack_entries, int mode, int32_t* out, const int32_t* count, const int64_t* offsets, int64_t total, int32_t* inst,
                         int32_t* face, uint8_t* lost) {
    const Scene s = scene_of(nodes, links, tris, nf, nmesh, mesh_of, M, ninst);
    int32_t mem[TR_TRIS_STACK];
    const tr_ring stack = {mem, 1};
    for (int64_t i = 0; i < n; i++) {
        const tr_tris_q q = sim_tri(tri + 9 * i);
        tr_boxes_acc acc;
        acc.count = 0; acc.limit = 0; acc.key = nullptr;
        uint8_t l = 0;
        if (mode == TR_TRIS_ANY) {
            out[i] = tr_scene_tris_query<TR_TRIS_ANY>(s.members.data(), s.recs.data(), (int32_t)ninst, order, q, stack, stack_entries, acc, nullptr, &l) > 0 ? 1 : 0;
        } else if (mode == TR_TRIS_COUNT) {
            out[i] = tr_scene_tris_query<TR_TRIS_COUNT>(s.members.data(), s.recs.data(), (int32_t)ninst, order, q, stack, stack_entries, acc, nullptr, &l);
        } else {
            const int64_t off = offsets[i];
            acc.limit = tr_rows_limit(count[i], off, total);
            if (acc.limit > 0) {
                acc.key = face + off;
                tr_scene_tris_query<TR_TRIS_FILL>(s.members.data(), s.recs.data(), (int32_t)ninst, order, q, stack, stack_entries, acc, inst + off, &l);
                tr_scene_tris_rows(inst + off, face + off, acc.limit);
            }
        }
        if (lost) lost[i] = l;
    }
}

// CULLING on its own: the object-space boxes lo, hi [n, 3] placed by M [12] against the box of query triangle i -> apart [n]
void sim_scene_tris_apart(const float* M, const float* tri, const float* lo, const float* hi, int64_t n, uint8_t* apart) {
    tr_scene_near_map A;
    tr_scene_near_map_make(M, A);
    for (int64_t i = 0; i < n; i++) {
        const tr_box qb = tr_tris_box(sim_tri(tri + 9 * i));
        apart[i] = tr_scene_tris_apart(A, qb, lo[3 * i], lo[3 * i + 1], lo[3 * i + 2], hi[3 * i], hi[3 * i + 1], hi[3 * i + 2]) ? 1 : 0;
    }
}
// contract 2 on its own: does query triangle i meet the member triangle abc [n, 9] placed by M [12] (live, active, tr_tris_meets)
void sim_scene_tris_meets(const float* M, const float* tri, const float* abc, int64_t n, uint8_t* meets) {
    for (int64_t i = 0; i < n; i++) {
        const tr_tris_q q = sim_tri(tri + 9 * i);
        const float* t = abc + 9 * i;
        float w[9];
        for (int v = 0; v < 3; v++) tr_scene_point(M, t[3 * v], t[3 * v + 1], t[3 * v + 2], w[3 * v], w[3 * v + 1], w[3 * v + 2]);
        meets[i] = tr_tris_live(q) && tr_near_active(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]) &&
                   tr_tris_meets(q, tr_tris_box(q), w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]) ? 1 : 0;
    }
}

}  // extern "C"

#ifdef SCENE_TRIS_SIM_MAIN
// a stand-alone program around the same routine (for a sanitizer build of host code: g++ -fsanitize=... -DSCENE_TRIS_SIM_MAIN).
// argv[1]: a file of int64 {nmesh, ninst, n, total}, then per member int64 {nn, nf}, nodes [nn] (64 B), links [nn] (8 B), tris
// [nf] (48 B); mesh_of i32 [ninst], M f32 [ninst, 12], tri f32 [n, 9]; what a brute force expects: count i32 [n], instance i32
// [total], face i32 [total].  any, count and the fill at argv[2] stack entries and at the whole stack, in both visiting orders,
// into heap buffers of exactly n and total elements against the expected ones; then a fill whose total is cut short by three
// rows into buffers of exactly that many (the sanitizer is the guard).
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
    const std::vector<int64_t> hd = take<int64_t>(fp, 4);
    const int64_t nmesh = hd[0], ninst = hd[1], n = hd[2], total = hd[3];
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
    const auto tri = take<float>(fp, 9 * n);
    const auto count = take<int32_t>(fp, n), inst = take<int32_t>(fp, total), face = take<int32_t>(fp, total);
    fclose(fp);
    std::vector<int64_t> off(n + 1, 0);
    for (int64_t i = 0; i < n; i++) off[i + 1] = off[i] + count[i];
    bool ok = off[n] == total;
    std::vector<int32_t> reversed((size_t)ninst);
    for (int64_t k = 0; k < ninst; k++) reversed[(size_t)k] = (int32_t)(ninst - 1 - k);
    int64_t nlost = 0, nmet = 0;
    for (int variant = 0; variant < 4; variant++) {
        const int32_t* order = (variant & 1) ? reversed.data() : nullptr;
        const int e = (variant & 2) ? 0 : entries;
        std::vector<int32_t> any(n), wc(n), wi(total), wf(total);
        std::vector<uint8_t> lost(n);
        for (int mode = 0; mode < 3; mode++)
            sim_scene_tris_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, order, tri.data(), n, e, mode,
                                mode == 0 ? any.data() : (mode == 1 ? wc.data() : nullptr), count.data(), off.data(), total, wi.data(), wf.data(),
                                mode == 1 ? lost.data() : nullptr);
        ok = ok && memcmp(wc.data(), count.data(), 4 * n) == 0 && memcmp(wi.data(), inst.data(), 4 * total) == 0 &&
             memcmp(wf.data(), face.data(), 4 * total) == 0;
        for (int64_t i = 0; i < n; i++) ok = ok && any[i] == (count[i] > 0);
        if (!variant)
            for (int64_t i = 0; i < n; i++) { nlost += lost[i]; nmet += count[i] > 0; }
    }
    {   // a total cut short: nothing beyond it is written, and what is written are pairs of the query
        const int64_t cut = total > 3 ? total - 3 : 0;
        std::vector<int32_t> wi(cut), wf(cut);
        sim_scene_tris_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, nullptr, tri.data(), n, entries, 2,
                            nullptr, count.data(), off.data(), cut, wi.data(), wf.data(), nullptr);
        for (int64_t i = 0; i < n; i++)
            if (off[i + 1] <= cut) ok = ok && memcmp(wi.data() + off[i], inst.data() + off[i], 4 * count[i]) == 0 &&
                                         memcmp(wf.data() + off[i], face.data() + off[i], 4 * count[i]) == 0;
    }
    printf("%lld triangles, %lld instances, %lld that meet something, %lld rows, stack_entries %d: %lld triangles overflowed a stack; any, count, "
           "instance and face in both visiting orders: %s\n",
           (long long)n, (long long)ninst, (long long)nmet, (long long)total, entries, (long long)nlost, ok ? "same as the brute force" : "DIFFERENT");
    return ok ? 0 : 1;
}
#endif
