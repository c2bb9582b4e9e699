// scene_cross_sim.cpp -- TEST-ONLY: csrc/tr_scene_cross.h built for the host (libscene_cross_sim.so,
// tests/host_sim/scene_cross_sim.py).  The walk (tr_scene_cross_query: the count, then the fill; tr_scene_cross_rows) over the
// arrays of the members' hierarchies (sim.SimBVH), ray by ray, in any visiting order and at any stack limit; and
// tr_scene_cross_sort on rows handed in.  The brute force it is compared with is NOT here: scene_cross_sim.py composes it in
// numpy from cross_sim.brute and scene_sim.transform, two brute forces that share no code with the instance loop.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_scene_cross.h"

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

int sim_scene_cross_stack_capacity(void) { return TR_CROSS_STACK; }

// members as (nodes, links, tris, nf) of their hierarchies; instances: mesh_of [ninst], M [ninst, 12]; order: the order the
// instances are visited in (null: ascending); rays dense [n, 3] + [n, 3]; tmin / tmax [n] or null; stack_entries: 0 = all.
// mode 0: count [n] in out; 1: the fill -- count / offsets / total as tr_scene_cross_fill takes them, rows into inst, face and
// t (slot: scratch of `total`, required with front / loc / uv), then the ordering and the optional rows (ray: i + ray_base).
// lost [n] (may be null): some instance's first walk of ray i overflowed its stack.
void sim_scene_cross_walk(const void* const* nodes, const void* const* links, const void* const* tris, const int64_t* nf, int64_t nmesh,
                          const int32_t* mesh_of, const float* M, int64_t ninst, const int32_t* order, const float* origins,
                          const float* dirs, const float* tmin, const float* tmax, int64_t n, int stack_entries, int mode, int32_t* out,
                          const int32_t* count, const int64_t* offsets, int64_t total, int32_t* inst, int32_t* face, float* t, int32_t* slot,
                          uint8_t* front, float* loc, float* uv, int64_t* ray, int64_t ray_base, uint8_t* lost) {
    const Scene s = scene_of(nodes, links, tris, nf, nmesh, mesh_of, M, ninst);
    int32_t mem[TR_CROSS_STACK];
    const tr_ring stack = {mem, 1, nullptr};
    for (int64_t i = 0; i < n; i++) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        const float lo = tmin ? tmin[i] : 0.0f, hi = tmax ? tmax[i] : TR_TMAX;
        tr_cross_acc acc;
        acc.count = 0; acc.limit = 0; acc.face = nullptr; acc.t = nullptr; acc.slot = nullptr;
        uint8_t l = 0;
        if (mode == TR_CROSS_COUNT) {
            out[i] = tr_scene_cross_query<TR_CROSS_COUNT>(s.members.data(), s.recs.data(), (int32_t)ninst, order, o[0], o[1], o[2], d[0], d[1],
                                                          d[2], lo, hi, stack, stack_entries, acc, nullptr, &l);
        } else {
            const int64_t off = offsets[i];
            acc.limit = tr_cross_limit(count[i], off, total);
            if (acc.limit > 0) {
                acc.face = face + off; acc.t = t + off; acc.slot = slot ? slot + off : nullptr;
                tr_scene_cross_query<TR_CROSS_FILL>(s.members.data(), s.recs.data(), (int32_t)ninst, order, o[0], o[1], o[2], d[0], d[1], d[2],
                                                    lo, hi, stack, stack_entries, acc, inst + off, &l);
                tr_scene_cross_rows(s.members.data(), s.recs.data(), (int32_t)ninst, o[0], o[1], o[2], d[0], d[1], d[2], inst + off, face + off,
                                    t + off, slot ? slot + off : nullptr, acc.limit, front ? front + off : nullptr,
                                    loc ? loc + 3 * off : nullptr, uv ? uv + 2 * off : nullptr, ray ? ray + off : nullptr, i + ray_base);
            }
        }
        if (lost) lost[i] = l;
    }
}

// tr_scene_cross_sort on m rows handed in (slot may be null)
void sim_scene_cross_sort(float* t, int32_t* inst, int32_t* face, int32_t* slot, int32_t m) { tr_scene_cross_sort(t, inst, face, slot, m); }

}  // extern "C"

#ifdef SCENE_CROSS_SIM_MAIN
// a stand-alone program around the same routines (for a sanitizer build of host code: g++ -fsanitize=... -DSCENE_CROSS_SIM_MAIN).
// argv[1]: a file of int64 {nmesh, ninst, n, total}, then per member int64 {nn, nf}, nodes [nn] (64 B), links [nn] (8 B),
// tris [nf] (48 B); mesh_of i32 [ninst], M f32 [ninst, 12], origins, directions f32 [n, 3], tmin, tmax f32 [n]; the rows a
// brute force expects: count i32 [n], instance, face i32 [total], t f32 [total], front u8 [total], loc f32 [total, 3], uv f32
// [total, 2]; and the counts of a narrower interval, count2 i32 [n].
// The count walk and the fill + rows at argv[2] stack entries, in both visiting orders, into heap buffers of exactly `total`
// rows against the expected rows; then a fill with the counts of the narrower interval and a total cut short, into buffers of
// exactly that many rows (the sanitizer is the guard); and the sort on rows full of NaN.
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
    const auto org = take<float>(fp, 3 * n), dir = take<float>(fp, 3 * n);
    const auto lo = take<float>(fp, n), hi = take<float>(fp, n);
    const auto cnt = take<int32_t>(fp, n);
    const auto inst = take<int32_t>(fp, total), face = take<int32_t>(fp, total);
    const auto t = take<float>(fp, total);
    const auto front = take<uint8_t>(fp, total);
    const auto loc = take<float>(fp, 3 * total), uv = take<float>(fp, 2 * total);
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
    int64_t nlost = 0, longest = 0;
    for (int rev = 0; rev < 2; rev++) {
        std::vector<int32_t> wcnt(n), winst(total), wface(total), wslot(total);
        std::vector<float> wt(total), wloc(3 * total), wuv(2 * total);
        std::vector<uint8_t> wfront(total), lost(n);
        std::vector<int64_t> wray(total);
        const int32_t* order = rev ? reversed.data() : nullptr;
        sim_scene_cross_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, order, org.data(), dir.data(),
                             lo.data(), hi.data(), n, entries, 0, wcnt.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr, 0, lost.data());
        sim_scene_cross_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, order, org.data(), dir.data(),
                             lo.data(), hi.data(), n, entries, 1, nullptr, cnt.data(), off.data(), total, winst.data(), wface.data(), wt.data(),
                             wslot.data(), wfront.data(), wloc.data(), wuv.data(), wray.data(), 7, nullptr);
        for (int64_t i = 0; i < n; i++) {
            ok = ok && wcnt[i] == cnt[i];
            if (!rev) { nlost += lost[i]; if (cnt[i] > longest) longest = cnt[i]; }
            for (int64_t w = off[i]; w < off[i + 1]; w++) ok = ok && wray[w] == i + 7;
        }
        ok = ok && memcmp(winst.data(), inst.data(), 4 * total) == 0 && memcmp(wface.data(), face.data(), 4 * total) == 0 &&
             memcmp(wt.data(), t.data(), 4 * total) == 0 && memcmp(wfront.data(), front.data(), total) == 0 &&
             memcmp(wloc.data(), loc.data(), 12 * total) == 0 && memcmp(wuv.data(), uv.data(), 8 * total) == 0;
    }
    printf("%lld rays, %lld instances, %lld rows, longest list %lld, stack_entries %d: %lld rays overflowed a stack; walk and rows in both visiting orders: %s\n",
           (long long)n, (long long)ninst, (long long)total, (long long)longest, entries, (long long)nlost,
           ok ? "same bits as the brute force" : "DIFFERENT");
    {   // misuse: the counts of the narrower interval handed to a fill on the wider one, the total cut short by three rows
        const int64_t total2 = off2[n] > 3 ? off2[n] - 3 : off2[n];
        std::vector<int32_t> i2(total2), f2(total2), s2(total2);
        std::vector<float> t2(total2), l2(3 * total2), u2(2 * total2);
        std::vector<uint8_t> fr2(total2);
        std::vector<int64_t> r2(total2);
        sim_scene_cross_walk(pn.data(), pl.data(), pt.data(), nf.data(), nmesh, mesh_of.data(), M.data(), ninst, nullptr, org.data(), dir.data(),
                             lo.data(), hi.data(), n, entries, 1, nullptr, cnt2.data(), off2.data(), total2, i2.data(), f2.data(), t2.data(),
                             s2.data(), fr2.data(), l2.data(), u2.data(), r2.data(), 0, nullptr);
        for (int64_t i = 0; i < n; i++)
            for (int64_t row = off2[i]; row < off2[i + 1] && row < total2; row++) {
                ok = ok && r2[row] == i && i2[row] >= 0 && i2[row] < ninst;
                if (row > off2[i])
                    ok = ok && (t2[row - 1] < t2[row] || (t2[row - 1] == t2[row] && (i2[row - 1] < i2[row] || (i2[row - 1] == i2[row] && f2[row - 1] < f2[row]))));
            }
        printf("fill with the counts of a narrower interval (%lld rows): %s\n", (long long)total2, ok ? "inside its rows, ordered" : "WRONG");
    }
    for (int32_t m : {0, 1, 2, 3, 33, 3000}) {   // the sort on keys that compare false both ways: exact-size buffers
        std::vector<float> kt(m, NAN);
        std::vector<int32_t> ki(m), kf(m), ks(m);
        for (int32_t k = 0; k < m; k++) { kf[k] = (k * 7919) % (m ? m : 1); ks[k] = kf[k]; ki[k] = kf[k] % 3; if (k % 3 == 0) kt[k] = (float)(k % 5); }
        sim_scene_cross_sort(kt.data(), ki.data(), kf.data(), ks.data(), m);
        for (int32_t k = 0; k < m; k++) ok = ok && kf[k] == ks[k] && ki[k] == kf[k] % 3;
    }
    return ok ? 0 : 1;
}
#endif
