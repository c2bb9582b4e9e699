// scene_points_sim.cpp -- TEST-ONLY: csrc/tr_scene_points.h built for the host (libscene_points_sim.so,
// tests/host_sim/scene_points_sim.py).  The per-lane query (tr_scene_points_query: any, count, fill) over the arrays of the
// members' hierarchies (sim.SimBVH), point by point, in any visiting order, at any stack limit, with or without the shortcut.
// The brute force it is compared with is NOT here: scene_points_sim.py composes it in numpy from cross_sim.brute and
// scene_sim.transform, two brute forces that share no code with the instance loop or the parity rule.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_scene_points.h"

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

int sim_scene_points_stack_capacity(void) { return TR_CROSS_STACK; }

// members as (nodes, links, tris, nf) of their hierarchies; instances: mesh_of [ninst], M [ninst, 12]; order: the order the
// instances are visited in (null: ascending); points dense [n, 3]; dir3 [3]; stack_entries: 0 = all; both: the second pass
// is walked whatever the first count.  mode 0: any [n] into out8; 1: count [n] into out32; 2: the fill -- count / offsets /
// total as tr_scene_points_fill takes them, rows into inst.  lost_inst [n] (may be null): the last instance visited in
// which a pass of point i overflowed its stack, -1: none.
void sim_scene_points_walk(const void* const* nodes, const void* const* links, const void* const* tris, const int64_t* nf, int64_t nmesh,
                           const int32_t* mesh_of, const float* M, int64_t ninst, const int32_t* order, const float* points,
                           const float* dir3, int64_t n, int stack_entries, int both, int mode, uint8_t* out8, int32_t* out32,
                           const int32_t* count, const int64_t* offsets, int64_t total, int32_t* inst, int32_t* lost_inst) {
    const Scene s = scene_of(nodes, links, tris, nf, nmesh, mesh_of, M, ninst);
    int32_t mem[TR_CROSS_STACK];
    const tr_ring stack = {mem, 1, nullptr};
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        tr_scene_points_acc acc;
        acc.count = 0; acc.limit = 0; acc.inst = nullptr;
        int32_t l = -1;
        if (mode == TR_SCENE_POINTS_ANY) {
            out8[i] = tr_scene_points_query<TR_SCENE_POINTS_ANY>(s.members.data(), s.recs.data(), (int32_t)ninst, order, p[0], p[1], p[2], dir3[0],
                                                                 dir3[1], dir3[2], stack, stack_entries, both != 0, acc, &l) > 0 ? 1 : 0;
        } else if (mode == TR_SCENE_POINTS_COUNT) {
            out32[i] = tr_scene_points_query<TR_SCENE_POINTS_COUNT>(s.members.data(), s.recs.data(), (int32_t)ninst, order, p[0], p[1], p[2],
                                                                    dir3[0], dir3[1], dir3[2], stack, stack_entries, both != 0, acc, &l);
        } else {
            const int64_t off = offsets[i];
            acc.limit = tr_cross_limit(count[i], off, total);
            if (acc.limit > 0) {
                acc.inst = inst + off;
                tr_scene_points_query<TR_SCENE_POINTS_FILL>(s.members.data(), s.recs.data(), (int32_t)ninst, order, p[0], p[1], p[2], dir3[0],
                                                            dir3[1], dir3[2], stack, stack_entries, both != 0, acc, &l);
            }
        }
        if (lost_inst) lost_inst[i] = l;
    }
}

}  // extern "C"

#ifdef SCENE_POINTS_SIM_MAIN
// a stand-alone program around the same routine (for a sanitizer build of host code: g++ -fsanitize=... -DSCENE_POINTS_SIM_MAIN).
// argv[1]: a file of int64 {nmesh, ninst, n, total}, then per member int64 {nn, nf}, nodes [nn] (64 B), links [nn] (8 B),
// tris [nf] (48 B); mesh_of i32 [ninst], M f32 [ninst, 12], points f32 [n, 3], direction f32 [3]; what a brute force expects:
// any u8 [n], count i32 [n], instance i32 [total]; and the counts of ANOTHER query (misdirected ones), count2 i32 [n].
// The three queries at argv[2] stack entries, in both visiting orders, with and without the shortcut, into heap buffers of
// exactly n / total elements against the expected ones; then a fill with those other counts and a total cut
// short, into a buffer of exactly that many rows (the sanitizer is the guard).
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
    const auto pts = take<float>(fp, 3 * n), dir = take<float>(fp, 3);
    const auto any = take<uint8_t>(fp, n);
    const auto cnt = take<int32_t>(fp, n);
    const auto inst = take<int32_t>(fp, total);
    const auto cnt2 = take<int32_t>(fp, n);
    fclose(fp);
    bool ok = true;
    auto scan = [&](const std::vector<int32_t>& c) {
        std::vector<int64_t> off(n + 1, 0);
        for (int64_t i = 0; i < n; i++) off[i + 1] = off[i] + c[i];
        return off;
    };
    const std::vector<int64_t> off = scan(cnt), off2 = scan(cnt2);
    ok = ok && off[n] == total;
    std::vector<int32_t> reversed((size_t)ninst);
    for (int64_t k = 0; k < ninst; k++) reversed[(size_t)k] = (int32_t)(ninst - 1 - k);
    int64_t nlost = 0, most = 0;
    for (int variant = 0; variant < 4; variant++) {
        const int32_t* order = (variant & 1) ? reversed.data() : nullptr;
        const int both = variant >> 1;
        std::vector<uint8_t> wany(n);
        std::vector<int32_t> wcnt(n), winst(total), lost(n);
        sim_scene_points_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, order, pts.data(), dir.data(), n,
                              entries, both, 0, wany.data(), nullptr, nullptr, nullptr, 0, nullptr, nullptr);
        sim_scene_points_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, order, pts.data(), dir.data(), n,
                              entries, both, 1, nullptr, wcnt.data(), nullptr, nullptr, 0, nullptr, lost.data());
        sim_scene_points_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, order, pts.data(), dir.data(), n,
                              entries, both, 2, nullptr, nullptr, cnt.data(), off.data(), total, winst.data(), nullptr);
        for (int64_t i = 0; i < n; i++) {
            ok = ok && wany[i] == any[i] && wcnt[i] == cnt[i];
            if (!variant) { nlost += lost[i] >= 0; if (cnt[i] > most) most = cnt[i]; }
        }
        ok = ok && memcmp(winst.data(), inst.data(), 4 * total) == 0;
    }
    printf("%lld points, %lld instances, %lld rows, longest list %lld, stack_entries %d: %lld points overflowed a stack; any, count and list "
           "in both visiting orders, with and without the shortcut: %s\n",
           (long long)n, (long long)ninst, (long long)total, (long long)most, entries, (long long)nlost,
           ok ? "same bits as the brute force" : "DIFFERENT");
    {   // misuse: the counts of another query handed to a fill on this one, the total cut short by three rows
        const int64_t total2 = off2[n] > 3 ? off2[n] - 3 : off2[n];
        for (int rev = 0; rev < 2; rev++) {
            std::vector<int32_t> i2(total2, -7);
            sim_scene_points_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, rev ? reversed.data() : nullptr,
                                  pts.data(), dir.data(), n, entries, 0, 2, nullptr, nullptr, cnt2.data(), off2.data(), total2, i2.data(), nullptr);
            for (int64_t i = 0; i < n; i++) {
                const int64_t end = off2[i + 1] < total2 ? off2[i + 1] : total2;
                const int64_t written = off2[i] + (cnt[i] < cnt2[i] ? cnt[i] : cnt2[i]);
                for (int64_t row = off2[i]; row < end; row++) {
                    if (row >= written) { ok = ok && i2[row] == -7; continue; }      // (rows the point has no instance for stay untouched)
                    ok = ok && i2[row] >= 0 && i2[row] < ninst;
                    if (row > off2[i]) ok = ok && i2[row - 1] < i2[row];
                }
            }
        }
        printf("fill with the counts of another query (%lld rows): %s\n", (long long)total2, ok ? "inside its rows, ascending" : "WRONG");
    }
    return ok ? 0 : 1;
}
#endif
