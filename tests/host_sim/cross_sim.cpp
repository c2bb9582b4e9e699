// cross_sim.cpp -- TEST-ONLY: csrc/tr_cross.h built for the host (libcross_sim.so, tests/host_sim/cross_sim.py).
// The brute force: the per-triangle predicate tr_range_tri over every triangle of a mesh, kept where it accepts, IN FACE ORDER
// with all the outputs of a row (cross_sim.py orders the rows with numpy.lexsort: no code shared with tr_cross_sort) -- the
// oracle of the GPU tests.  And the walk (tr_cross_query, tr_cross_rows) over the arrays of a hierarchy (sim.SimBVH: built on
// the host, or downloaded from the GPU builder), ray by ray; and tr_cross_sort on rows handed in.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_cross.h"

extern "C" {

int sim_cross_stack_capacity(void) { return TR_CROSS_STACK; }

// pass 1 (face == null): count [n].  pass 2: the rows of ray i at offsets[i] .., in face order: face, t, front, loc, uv.
// vertices [nv, 3], faces [nf, 3]; rays dense [n, 3] + [n, 3]; tmin / tmax [n] or null
void sim_cross_brute(const float* verts, const int32_t* faces, int64_t nf, const float* origins, const float* dirs, const float* tmin,
                     const float* tmax, int64_t n, int32_t* count, const int64_t* offsets, int32_t* face, float* t, uint8_t* front,
                     float* loc, float* uv) {
    for (int64_t i = 0; i < n; i++) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        tr_ray r;
        float lo, hi;
        bool valid = tr_ray_setup(r, o[0], o[1], o[2], d[0], d[1], d[2]);
        valid = tr_range_bounds(tmin ? tmin[i] : 0.0f, tmax ? tmax[i] : TR_TMAX, lo, hi) && valid;
        int32_t k = 0;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            float tt;
            if (!tr_range_tri(r, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], lo, hi, tt)) continue;
            if (face) {
                const int64_t row = offsets[i] + k;
                face[row] = (int32_t)f;
                t[row] = tt;
                front[row] = tr_hit_outputs(r, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], loc + 3 * row, uv + 2 * row) ? 1 : 0;
            }
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

// the walk on (nodes, links, tris) of nf triangles; stack_entries: 0 = all, 1 .. TR_CROSS_STACK.
// mode 0: count [n] in out; 1: the fill -- count / offsets / total as tr_cross_fill takes them, rows into face and t (slot:
// scratch of `total`, required with front / loc / uv), then the ordering and the optional rows (ray: i + ray_base).
// lost [n] (may be null): the first walk of ray i overflowed its stack.
void sim_cross_walk(const void* nodes, const void* links, const void* tris, int64_t nf, const float* origins, const float* dirs,
                    const float* tmin, const float* tmax, int64_t n, int stack_entries, int mode, int32_t* out, const int32_t* count,
                    const int64_t* offsets, int64_t total, int32_t* face, float* t, int32_t* slot, uint8_t* front, float* loc, float* uv,
                    int64_t* ray, int64_t ray_base, uint8_t* lost) {
    const tr_bvh_view v = sim_view(nodes, links, tris, nf);
    int32_t mem[TR_CROSS_STACK];
    const tr_ring stack = {mem, 1, nullptr};
    for (int64_t i = 0; i < n; i++) {
        const float *o = origins + 3 * i, *d = dirs + 3 * i;
        const float lo = tmin ? tmin[i] : 0.0f, hi = tmax ? tmax[i] : TR_TMAX;
        tr_cross_acc acc;
        acc.count = 0; acc.limit = 0; acc.face = nullptr; acc.t = nullptr; acc.slot = nullptr;
        uint8_t l = 0;
        if (mode == TR_CROSS_COUNT) {
            out[i] = tr_cross_query<TR_CROSS_COUNT>(v, o[0], o[1], o[2], d[0], d[1], d[2], lo, hi, stack, stack_entries, acc, &l);
        } else {
            const int64_t off = offsets[i];
            acc.limit = tr_cross_limit(count[i], off, total);
            if (acc.limit > 0) {
                acc.face = face + off; acc.t = t + off; acc.slot = slot ? slot + off : nullptr;
                tr_cross_query<TR_CROSS_FILL>(v, o[0], o[1], o[2], d[0], d[1], d[2], lo, hi, stack, stack_entries, acc, &l);
                tr_ray r;
                tr_ray_setup(r, o[0], o[1], o[2], d[0], d[1], d[2]);
                tr_cross_rows(v, r, face + off, t + off, slot ? slot + off : nullptr, acc.limit, front ? front + off : nullptr,
                              loc ? loc + 3 * off : nullptr, uv ? uv + 2 * off : nullptr, ray ? ray + off : nullptr, i + ray_base);
            }
        }
        if (lost) lost[i] = l;
    }
}

// tr_cross_sort on m rows handed in (slot may be null)
void sim_cross_sort(float* t, int32_t* face, int32_t* slot, int32_t m) { tr_cross_sort(t, face, slot, m); }

}  // extern "C"

#ifdef CROSS_SIM_MAIN
// a stand-alone program around the same routines (for a sanitizer build of host code: g++ -fsanitize=... -DCROSS_SIM_MAIN).
// argv[1]: a file of int64 {nv, nf, nn, n}, then vertices f32 [nv, 3], faces i32 [nf, 3], nodes [nn] (64 B), links [nn] (8 B),
// tris [nf] (48 B), origins, directions f32 [n, 3], tmin, tmax f32 [n], and the narrower bounds tmin2, tmax2 f32 [n].
// The brute force, the count walk and the fill + rows at argv[2] stack entries against each other (the brute-force rows
// ordered by a std::stable_sort on (t, face)), then a fill with the counts of the narrower interval and a total cut short,
// into heap buffers of exactly that many rows (the sanitizer is the guard), and the sort on rows full of NaN.
#include <algorithm>
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
    const int64_t nv = hd[0], nf = hd[1], nn = hd[2], n = hd[3];
    static_assert(sizeof(tr_node) == 64 && sizeof(tr_link) == 8 && sizeof(tr_tri) == 48, "record sizes");
    const auto vs = take<float>(fp, 3 * nv);
    const auto fs = take<int32_t>(fp, 3 * nf);
    const auto nodes = take<tr_node>(fp, nn);
    const auto links = take<tr_link>(fp, nn);
    const auto tris = take<tr_tri>(fp, nf);
    const auto org = take<float>(fp, 3 * n), dir = take<float>(fp, 3 * n);
    const auto lo = take<float>(fp, n), hi = take<float>(fp, n), lo2 = take<float>(fp, n), hi2 = take<float>(fp, n);
    fclose(fp);
    bool ok = true;
    auto scan = [&](const std::vector<int32_t>& c) {
        std::vector<int64_t> off(n + 1, 0);
        for (int64_t i = 0; i < n; i++) off[i + 1] = off[i] + c[i];
        return off;
    };
    // the brute force, ordered
    std::vector<int32_t> cnt(n), cnt2(n), wcnt(n);
    sim_cross_brute(vs.data(), fs.data(), nf, org.data(), dir.data(), lo.data(), hi.data(), n, cnt.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    sim_cross_brute(vs.data(), fs.data(), nf, org.data(), dir.data(), lo2.data(), hi2.data(), n, cnt2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    const std::vector<int64_t> off = scan(cnt), off2 = scan(cnt2);
    const int64_t total = off[n];
    std::vector<int32_t> face(total), wface(total), wslot(total);
    std::vector<float> t(total), loc(3 * total), uv(2 * total), wt(total), wloc(3 * total), wuv(2 * total);
    std::vector<uint8_t> front(total), wfront(total), lost(n);
    std::vector<int64_t> wray(total);
    sim_cross_brute(vs.data(), fs.data(), nf, org.data(), dir.data(), lo.data(), hi.data(), n, nullptr, off.data(), face.data(), t.data(), front.data(),
                    loc.data(), uv.data());
    sim_cross_walk(nodes.data(), links.data(), tris.data(), nf, org.data(), dir.data(), lo.data(), hi.data(), n, entries, 0, wcnt.data(), nullptr, nullptr,
                   0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, lost.data());
    sim_cross_walk(nodes.data(), links.data(), tris.data(), nf, org.data(), dir.data(), lo.data(), hi.data(), n, entries, 1, nullptr, cnt.data(), off.data(),
                   total, wface.data(), wt.data(), wslot.data(), wfront.data(), wloc.data(), wuv.data(), wray.data(), 7, nullptr);
    int64_t nlost = 0, longest = 0;
    for (int64_t i = 0; i < n; i++) {
        ok = ok && wcnt[i] == cnt[i];
        nlost += lost[i];
        longest = std::max<int64_t>(longest, cnt[i]);
        std::vector<int64_t> order(cnt[i]);
        for (int64_t k = 0; k < cnt[i]; k++) order[k] = off[i] + k;
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return t[a] < t[b]; });      // (face order within equal t)
        for (int64_t k = 0; k < cnt[i]; k++) {
            const int64_t w = off[i] + k, b = order[k];
            ok = ok && wface[w] == face[b] && memcmp(&wt[w], &t[b], 4) == 0 && wfront[w] == front[b] && memcmp(&wloc[3 * w], &loc[3 * b], 12) == 0 &&
                 memcmp(&wuv[2 * w], &uv[2 * b], 8) == 0 && wray[w] == i + 7;
        }
    }
    printf("%lld rays, %lld rows, longest list %lld, stack_entries %d: %lld count walks overflowed; walk and rows: %s\n", (long long)n,
           (long long)total, (long long)longest, entries, (long long)nlost, ok ? "same bits as the brute force" : "DIFFERENT");
    {   // misuse: the counts of the narrower interval handed to a fill on the wider one, the total cut short by three rows
        const int64_t total2 = off2[n] > 3 ? off2[n] - 3 : off2[n];
        std::vector<int32_t> f2(total2), s2(total2);
        std::vector<float> t2(total2), l2(3 * total2), u2(2 * total2);
        std::vector<uint8_t> fr2(total2);
        std::vector<int64_t> r2(total2);
        sim_cross_walk(nodes.data(), links.data(), tris.data(), nf, org.data(), dir.data(), lo.data(), hi.data(), n, entries, 1, nullptr, cnt2.data(),
                       off2.data(), total2, f2.data(), t2.data(), s2.data(), fr2.data(), l2.data(), u2.data(), r2.data(), 0, nullptr);
        for (int64_t i = 0; i < n; i++)
            for (int64_t row = off2[i] + 1; row < off2[i + 1] && row < total2; row++)
                ok = ok && (t2[row - 1] < t2[row] || (t2[row - 1] == t2[row] && f2[row - 1] < f2[row])) && r2[row] == i;
        printf("fill with the counts of a narrower interval (%lld rows): %s\n", (long long)total2, ok ? "inside its rows, ordered" : "WRONG");
    }
    for (int32_t m : {0, 1, 2, 3, 33, 3000}) {   // the sort on keys that compare false both ways: exact-size buffers
        std::vector<float> kt(m, NAN);
        std::vector<int32_t> kf(m), ks(m);
        for (int32_t k = 0; k < m; k++) { kf[k] = (k * 7919) % (m ? m : 1); ks[k] = kf[k]; if (k % 3 == 0) kt[k] = (float)(k % 5); }
        sim_cross_sort(kt.data(), kf.data(), ks.data(), m);
        for (int32_t k = 0; k < m; k++) ok = ok && kf[k] == ks[k];
    }
    return ok ? 0 : 1;
}
#endif
