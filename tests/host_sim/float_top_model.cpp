// float_top_model.cpp -- TEST-ONLY: uniform_top_model.cpp (included whole and unchanged) plus the FLOAT TOP: the table loop
// that walks the wave-uniform top of the tree from the per-octant tables of pre-selected float planes (tr_bvh.h: tr_top_rec,
// tr_top_fill, tr_top_test, tr_top_build_slot), in front of the generic uniform loop, the descent phase and the general loop.
// The table loop runs while the wave's node has a heap slot in the table; it leaves on exactly the generic loop's conditions
// and hands over what that loop would have left, or -- the next node lies below the table -- lets the generic loop go on
// at that arena index with the same lanes, trip count and stack pointers.
//   variant 4: table loop + uniform top + descent phase + general loop;
// and three deliberately WRONG forms:
//   variant 5: octant 0's table is used for every octant;
//   variant 6: the table is not the hierarchy's (the caller hands in one built before a refit; the loop itself is variant 4's);
//   variant 7: the table loop does not leave when no lane has a child to go to, and walks on into slot 2i + 2, absent or not.
// Variants 0 to 3 are uniform_top_model.cpp's.  Per group a seventh figure: the trips of the table loop (they are trips of
// the uniform top as well).  A library of its own (libfloat_top_model.so, tests/host_sim/float_top_sim.py).
#include "uniform_top_model.cpp"

namespace {
template <int Q>
void ft_wave_run(const tr_bvh_view& v, const tr_top_rec* top, uint32_t slots, dm_lane* L, int m, int variant, uint32_t steal_min,
                 dm_wave& w, ut_wave& u, int32_t& table_trips) {
    if (variant < 4) {
        ut_wave_run<Q>(v, L, m, variant, steal_min, w, u);
        return;
    }
    uint32_t trip = 0, k0 = 0;
    bool l0[64], l1[64], go[64];
    int32_t c0[64], c1[64];
    for (int k = 0; k < m; k++) { l0[k] = l1[k] = false; c0[k] = c1[k] = 0; go[k] = L[k].fs.node >= 0; }
    bool stop = false;
    int first = -1;
    uint64_t act = 0;
    for (int k = 0; k < m; k++) {
        if (go[k]) { if (first < 0) first = k; act |= 1ull << k; }
    }
    if (first >= 0 && trip < steal_min) {
        const uint32_t sn = L[first].r.sel_n, sf = L[first].r.sel_f, sz = L[first].r.sel_z;
        bool same = true;
        for (int k = 0; k < m; k++) same = same && !(go[k] && (L[k].r.sel_n != sn || L[k].r.sel_f != sf || L[k].r.sel_z != sz));
        u.octant_fail = !same;
        if (same) {
            const tr_uoctant oct = tr_uniform_octant(sn, sz);
            const tr_top_rec* tab = top ? top + (size_t)(variant == 5 ? 0u : tr_octant_index(sn, sz)) * slots : nullptr;
            int32_t nu = 0;
            uint32_t slot = 0;
            for (;;) {
                dm_before(L, m, w);
                const bool in_table = tab && slot < slots;
                int32_t ch0, ch1;
                uint64_t b0 = 0, b1 = 0, blt = 0;
                if (in_table) {
                    const tr_top_rec& t = tab[slot];
                    for (int k = 0; k < m; k++) {
                        bool a0, a1, lt;
                        tr_top_test<Q>(L[k].r, t.p, L[k].res, a0, a1, lt);
                        b0 |= (uint64_t)a0 << k; b1 |= (uint64_t)a1 << k; blt |= (uint64_t)lt << k;
                    }
                    ch0 = t.c0; ch1 = t.c1;
                    table_trips++;
                } else {
                    const tr_i4* np = tr_qnode_ptr<true>(v, nu);
                    const tr_i4 w0 = np[0], w1 = np[1];
                    for (int k = 0; k < m; k++) {
                        bool a0, a1, lt;
                        tr_uniform_test<Q>(L[k].r, w0, w1, oct, L[k].res, a0, a1, lt);
                        b0 |= (uint64_t)a0 << k; b1 |= (uint64_t)a1 << k; blt |= (uint64_t)lt << k;
                    }
                    ch0 = w1.z; ch1 = w1.w;
                }
                for (int k = 0; k < m; k++) if (go[k]) L[k].cnt.nodes++;
                const tr_uwave uw = tr_uniform_wave(act, b0, b1, blt, ch0, ch1);
                for (int k = 0; k < m; k++) {
                    const bool was = tr_addr_lost(L[k].fs.sa);
                    if (tr_lane_in(uw.both, k)) tr_addr_push(tr_aring_of(L[k].ring), L[k].fs.sa, tr_lane_in(uw.sw, k) ? ch0 : ch1);
                    if (!was && tr_addr_lost(L[k].fs.sa)) w.lost_in_phase++;
                }
                trip++;
                u.loop++;
                const bool leaf = (uw.l0 | uw.l1) != 0;
                const uint64_t sw = uw.sw;
                const bool differ = sw != 0 && sw != act;
                const bool pop = uw.pop != 0 && !(variant == 7 && in_table && !leaf && !differ && 2 * slot + 2 < slots);
                if (leaf || pop || differ || trip >= steal_min) {
                    bool any_node = false;
                    for (int k = 0; k < m; k++) {
                        c0[k] = ch0; c1[k] = ch1;
                        l0[k] = tr_lane_in(uw.l0, k); l1[k] = tr_lane_in(uw.l1, k);
                        if (go[k]) L[k].fs.node = tr_lane_in(uw.sw, k) ? ch1 : ch0;
                        if (tr_lane_in(uw.pop, k)) L[k].fs.node = tr_addr_pop(tr_aring_of(L[k].ring), L[k].fs.sa);
                        any_node = any_node || L[k].fs.node >= 0;
                    }
                    dm_after(L, m, w);
                    stop = leaf || !any_node;
                    break;
                }
                dm_after(L, m, w);
                nu = sw ? ch1 : ch0;
                slot = 2 * slot + (sw ? 2u : 1u);      // (past the table from here on: slot >= slots stays so)
                if (nu < 0) nu = 0;                    // variant 7 alone: a leaf's slot; the generic loop needs an arena node
            }
        }
    }
    // ---- the descent phase and the general loop, as in ut_wave_run
    if (!stop) {
        while (trip < steal_min) {
            dm_before(L, m, w);
            bool any_leaf = false, any_node = false;
            for (int k = 0; k < m; k++) {
                l0[k] = false; l1[k] = false;
                if (L[k].fs.node >= 0) {
                    const bool was = tr_addr_lost(L[k].fs.sa);
                    tr_descent_step<Q, true, true>(v, L[k].r, L[k].fs, L[k].res, &L[k].cnt, L[k].ring, l0[k], l1[k], c0[k], c1[k]);
                    if (!was && tr_addr_lost(L[k].fs.sa)) w.lost_in_phase++;
                }
                any_leaf = any_leaf || l0[k] || l1[k];
                any_node = any_node || L[k].fs.node >= 0;
            }
            trip++;
            w.phase++;
            dm_after(L, m, w);
            if (any_leaf || !any_node) break;
        }
    }
    for (int k = 0; k < m; k++) {
        L[k].fs.p0 = l0[k] ? ~c0[k] : (l1[k] ? ~c1[k] : -1);
        L[k].fs.p1 = (l0[k] && l1[k]) ? ~c1[k] : -1;
    }
    if (w.phase || u.loop) dm_after(L, m, w);
    if (trip & 1u) {
        dm_general<Q, false>(v, L, m, w);
        trip++;
    }
    k0 = trip == 0u ? 0u : ((trip - 1u) & 3u) + 1u;
    trip -= k0;
    for (;;) {
        for (uint32_t k = k0; k <= 3u; k += 2) {
            dm_general<Q, true>(v, L, m, w);
            dm_general<Q, false>(v, L, m, w);
        }
        k0 = 0;
        trip += 4;
        bool all = true;
        for (int k = 0; k < m; k++) all = all && tr_done(L[k].fs);
        if (all) break;
    }
}

int64_t g_ft_lost;

// ut_run with ft_wave_run in the place of ut_wave_run and seven figures per group
template <int Q>
void ft_run(const tr_bvh_view& v, const tr_top_rec* top, uint32_t slots, int variant, uint32_t steal_min, const float* o, const float* d,
            int64_t n, uint8_t* hit, uint8_t* front, int32_t* tri, float* loc, float* uv, uint64_t* stats, int32_t* per_ray,
            int32_t* per_group) {
    static dm_lane L[64];
    uint64_t tn = 0, tt = 0;
    g_ft_lost = 0;
    for (int64_t g0 = 0; g0 < n; g0 += 64) {
        const int m = (int)(n - g0 < 64 ? n - g0 : 64);
        for (int k = 0; k < m; k++) {
            const int64_t i = g0 + k;
            dm_lane& l = L[k];
            l.valid = tr_ray_setup_q(l.r, v.frame, o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2]);
            l.cnt.nodes = l.cnt.tris = l.cnt.climbs = 0;
            l.ring = tr_ring{l.ring_mem + 2, 4, l.ring_mem};
            l.lost_trip = 0;
            tr_result_init(l.res);
            tr_state_init(l.fs, tr_addr_start(l.ring));
            if (!(l.valid && v.num_tris >= 2)) l.fs.node = -1;
        }
        dm_wave w;
        ut_wave u;
        int32_t table_trips = 0;
        if (v.num_tris >= 2) ft_wave_run<Q>(v, top, slots, L, m, variant, steal_min, w, u, table_trips);
        if (per_group) {
            int32_t* p = per_group + 7 * (g0 / 64);
            p[0] = w.first_leaf; p[1] = w.uniform; p[2] = w.longest; p[3] = w.phase; p[4] = u.loop; p[5] = u.octant_fail;
            p[6] = table_trips;
        }
        for (int k = 0; k < m; k++) {
            const int64_t i = g0 + k;
            dm_lane& l = L[k];
            const bool lost = tr_addr_lost(l.fs.sa);
            if (per_ray) { per_ray[3 * i] = (int32_t)l.cnt.nodes; per_ray[3 * i + 1] = (int32_t)l.cnt.tris; per_ray[3 * i + 2] = lost; }
            tn += l.cnt.nodes; tt += l.cnt.tris;
            if (lost) {
                g_ft_lost++;
                tr_topk<1> tk;
                tr_traverse_more<Q, 1, true>(v, l.r, l.res, tk, &l.cnt);
            }
            const tr_result& res = l.res;
            if (Q == TR_Q_ANY) hit[i] = res.best_face >= 0;
            if (Q == TR_Q_FIRST) tri[i] = res.best_face;
            if (Q == TR_Q_CLOSEST) {
                float l3[3] = {0, 0, 0}, u2[2] = {0, 0};
                hit[i] = res.best_face >= 0; front[i] = 0; tri[i] = res.best_face;
                if (res.best_face >= 0) {
                    const tr_tri& t = v.tris[res.best_slot];
                    front[i] = tr_hit_outputs(l.r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, l3, u2);
                }
                memcpy(loc + 3 * i, l3, 12); memcpy(uv + 2 * i, u2, 8);
            }
        }
    }
    stats[0] = (uint64_t)n; stats[1] = tn; stats[2] = tt; stats[3] = 0;
}
}  // namespace

extern "C" {
// the eight tables of `levels` levels of the grid nodes `qnodes` (nf >= 2 triangles), slot by slot as tr_top_build_slot defines
// them: out = 8 * (2^levels - 1) records of 64 bytes
void sim_float_top_build(const void* qnodes, int64_t num_nodes, int levels, void* out) {
    const uint32_t slots = (1u << levels) - 1u;
    for (uint32_t s = 0; s < slots; s++) tr_top_build_slot((tr_top_rec*)out, (const tr_qnode*)qnodes, num_nodes, s, slots);
}
// one record, and the two box tests on it, for the plane test: rays = n x (origin, direction) of octant `o` in the frame f6
// (base, scale); out3 = n x {a0, a1, lt} of tr_uniform_test and then of tr_top_test
void sim_float_top_record(const void* qnode, uint32_t o, void* rec) { tr_top_fill(*(tr_top_rec*)rec, *(const tr_qnode*)qnode, o); }
int sim_float_top_tests(const void* qnode, const float* f6, const float* od, int64_t n, float best_t, float* planes, uint8_t* out) {
    tr_qframe f;
    for (int k = 0; k < 3; k++) { f.base[k] = f6[k]; f.scale[k] = f6[3 + k]; }
    const tr_qnode& q = *(const tr_qnode*)qnode;
    const tr_i4 w0 = {(int32_t)q.q[0], (int32_t)q.q[1], (int32_t)q.q[2], (int32_t)q.q[3]};
    const tr_i4 w1 = {(int32_t)q.q[4], (int32_t)q.q[5], q.c0, q.c1};
    for (int64_t i = 0; i < n; i++) {
        tr_ray r;
        if (!tr_ray_setup_q(r, f, od[6 * i], od[6 * i + 1], od[6 * i + 2], od[6 * i + 3], od[6 * i + 4], od[6 * i + 5])) return -1;
        tr_result res;
        tr_result_init(res);
        tr_set_best_t(res, best_t);
        const uint32_t o = tr_octant_index(r.sel_n, r.sel_z);
        tr_top_rec t;
        tr_top_fill(t, q, o);
        bool a[6];
        tr_uniform_test<TR_Q_CLOSEST>(r, w0, w1, tr_uniform_octant(r.sel_n, r.sel_z), res, a[0], a[1], a[2]);
        tr_top_test<TR_Q_CLOSEST>(r, t.p, res, a[3], a[4], a[5]);
        for (int k = 0; k < 6; k++) out[6 * i + k] = a[k];
        if (planes) memcpy(planes + 13 * i, t.p, 48), planes[13 * i + 12] = (float)o;
    }
    return 0;
}
// sim_uniform_top_query's arguments with the table (8 x `slots` records; NULL: none), the variants above and SEVEN int32 per
// group: uniform_top_model.cpp's six and the trips of the table loop
int sim_float_top_query(int q, int variant, uint32_t steal_min, const void* nodes, const void* links, const void* tris, int64_t nf,
                        const void* top, uint32_t slots, const float* o, const float* d, int64_t n, uint8_t* hit, uint8_t* front,
                        int32_t* tri, float* loc, float* uv, uint64_t* stats, int32_t* per_ray, int32_t* per_group) {
    const tr_bvh_view v = view_of((const tr_node*)nodes, (const tr_link*)links, (const tr_tri*)tris, nf);
    const tr_top_rec* t = (const tr_top_rec*)top;
    switch (q) {
        case TR_Q_ANY: ft_run<TR_Q_ANY>(v, t, slots, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
        case TR_Q_FIRST: ft_run<TR_Q_FIRST>(v, t, slots, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
        case TR_Q_CLOSEST: ft_run<TR_Q_CLOSEST>(v, t, slots, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
    }
    return -1;
}
int64_t sim_float_top_lost(void) { return g_ft_lost; }
}
