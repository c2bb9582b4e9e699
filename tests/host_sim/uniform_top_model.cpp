// uniform_top_model.cpp -- TEST-ONLY: descent_model.cpp (included whole and unchanged) plus the UNIFORM TOP of the stealing
// grid-node launch: the loop that wave_traverse_steal (kernels_direct.inc) runs in front of its descent phase while every
// visiting lane of the wave is at one node and all its rays point into one octant, driven through the product's own
// tr_uniform_test, tr_uniform_wave and tr_lane_in (tr_bvh.h).  The entry test, the loop and its exits are written out here
// as the kernel has them, statement by statement; the phase and the general loop behind it are those of descent_model.cpp.
//   variant 0: descent phase + general loop (descent_model.cpp's variant 1: what the kernels ran before the loop);
//   variant 1: uniform top + descent phase + general loop, as the kernels run it;
// and two deliberately WRONG forms, so that the test that compares the variants can show that it has bite:
//   variant 2: the entry test is left out -- a wave of mixed octants walks with its first lane's octant;
//   variant 3: the loop goes on, at the first lane's next node, after the lanes' next nodes differ.
// Per ray: outputs, node visits, leaf tests, the lost flag.  Per group: descent_model.cpp's four figures, the trips of the
// uniform top, and whether the group failed the octant test.  A library of its own (libuniform_top_model.so,
// tests/host_sim/uniform_top_sim.py).
#include "descent_model.cpp"

namespace {
struct ut_wave {
    int32_t loop = 0;                   // trips of the uniform top
    int32_t octant_fail = 0;            // the wave has a valid ray and its valid rays do not share one octant
};

template <int Q>
void ut_wave_run(const tr_bvh_view& v, dm_lane* L, int m, int variant, uint32_t steal_min, dm_wave& w, ut_wave& u) {
    if (variant == 0) {
        dm_wave_run<Q>(v, L, m, 1, steal_min, w);
        return;
    }
    uint32_t trip = 0, k0 = 0;
    bool l0[64], l1[64], go[64];
    int32_t c0[64], c1[64];
    for (int k = 0; k < m; k++) { l0[k] = l1[k] = false; c0[k] = c1[k] = 0; go[k] = L[k].fs.node >= 0; }
    bool stop = false;                  // the uniform top ended where the phase's loop ends
    // ---- the uniform top: entry test, once per wave, against the first ACTIVE lane
    int first = -1;
    uint64_t act = 0;                   // the lanes with a node
    for (int k = 0; k < m; k++) {
        if (go[k]) { if (first < 0) first = k; act |= 1ull << k; }
    }
    if (first >= 0 && trip < steal_min) {
        const uint32_t sn = L[first].r.sel_n, sf = L[first].r.sel_f, sz = L[first].r.sel_z;
        bool same = true;
        for (int k = 0; k < m; k++) same = same && !(go[k] && (L[k].r.sel_n != sn || L[k].r.sel_f != sf || L[k].r.sel_z != sz));
        u.octant_fail = !same;
        if (same || variant == 2) {
            const tr_uoctant oct = tr_uniform_octant(sn, sz);
            int32_t nu = 0;
            for (;;) {
                dm_before(L, m, w);
                const tr_i4* np = tr_qnode_ptr<true>(v, nu);
                const tr_i4 w0 = np[0], w1 = np[1];
                uint64_t b0 = 0, b1 = 0, blt = 0;      // the three compares of EVERY lane, as the kernel's ballots collect them
                for (int k = 0; k < m; k++) {
                    bool a0, a1, lt;
                    tr_uniform_test<Q>(L[k].r, w0, w1, oct, L[k].res, a0, a1, lt);
                    if (go[k]) L[k].cnt.nodes++;
                    b0 |= (uint64_t)a0 << k; b1 |= (uint64_t)a1 << k; blt |= (uint64_t)lt << k;
                }
                const tr_uwave uw = tr_uniform_wave(act, b0, b1, blt, w1.z, w1.w);
                for (int k = 0; k < m; k++) {
                    const bool was = tr_addr_lost(L[k].fs.sa);
                    if (tr_lane_in(uw.both, k)) tr_addr_push(tr_aring_of(L[k].ring), L[k].fs.sa, tr_lane_in(uw.sw, k) ? w1.z : w1.w);
                    if (!was && tr_addr_lost(L[k].fs.sa)) w.lost_in_phase++;
                }
                trip++;
                u.loop++;
                const bool leaf = (uw.l0 | uw.l1) != 0;
                uint64_t sw = uw.sw;
                bool differ = sw != 0 && sw != act;
                if (variant == 3 && differ && !leaf && !uw.pop && trip < steal_min) { differ = false; sw = tr_lane_in(sw, first) ? act : 0; }
                if (leaf || uw.pop != 0 || differ || trip >= steal_min) {
                    bool any_node = false;
                    for (int k = 0; k < m; k++) {
                        c0[k] = w1.z; c1[k] = w1.w;
                        l0[k] = tr_lane_in(uw.l0, k); l1[k] = tr_lane_in(uw.l1, k);
                        if (go[k]) L[k].fs.node = tr_lane_in(uw.sw, k) ? w1.w : w1.z;
                        if (tr_lane_in(uw.pop, k)) L[k].fs.node = tr_addr_pop(tr_aring_of(L[k].ring), L[k].fs.sa);
                        any_node = any_node || L[k].fs.node >= 0;
                    }
                    dm_after(L, m, w);
                    stop = leaf || !any_node;
                    break;
                }
                dm_after(L, m, w);
                nu = sw ? w1.w : w1.z;
            }
        }
    }
    // ---- the descent phase and the general loop: descent_model.cpp's dm_wave_run from here on
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

int64_t g_ut_lost;

// dm_run with ut_wave_run in the place of dm_wave_run and six figures per group
template <int Q>
void ut_run(const tr_bvh_view& v, int variant, uint32_t steal_min, const float* o, const float* d, int64_t n, uint8_t* hit,
            uint8_t* front, int32_t* tri, float* loc, float* uv, uint64_t* stats, int32_t* per_ray, int32_t* per_group) {
    static dm_lane L[64];
    uint64_t tn = 0, tt = 0;
    g_ut_lost = 0;
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
        if (v.num_tris >= 2) ut_wave_run<Q>(v, L, m, variant, steal_min, w, u);
        if (per_group) {
            int32_t* p = per_group + 6 * (g0 / 64);
            p[0] = w.first_leaf; p[1] = w.uniform; p[2] = w.longest; p[3] = w.phase; p[4] = u.loop; p[5] = u.octant_fail;
        }
        for (int k = 0; k < m; k++) {
            const int64_t i = g0 + k;
            dm_lane& l = L[k];
            const bool lost = tr_addr_lost(l.fs.sa);
            if (per_ray) { per_ray[3 * i] = (int32_t)l.cnt.nodes; per_ray[3 * i + 1] = (int32_t)l.cnt.tris; per_ray[3 * i + 2] = lost; }
            tn += l.cnt.nodes; tt += l.cnt.tris;
            if (lost) {
                g_ut_lost++;
                tr_topk<1> top;
                tr_traverse_more<Q, 1, true>(v, l.r, l.res, top, &l.cnt);
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
// sim_descent_query's arguments with the variants above and `per_group` of SIX int32 per group of 64 rays: first-leaf trip,
// uniform leading trips, trips of the longest lane, trips of the descent phase, trips of the uniform top, octant test failed.
int sim_uniform_top_query(int q, int variant, uint32_t steal_min, const void* nodes, const void* links, const void* tris, int64_t nf,
                          const float* o, const float* d, int64_t n, uint8_t* hit, uint8_t* front, int32_t* tri, float* loc, float* uv,
                          uint64_t* stats, int32_t* per_ray, int32_t* per_group) {
    const tr_bvh_view v = view_of((const tr_node*)nodes, (const tr_link*)links, (const tr_tri*)tris, nf);
    switch (q) {
        case TR_Q_ANY: ut_run<TR_Q_ANY>(v, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
        case TR_Q_FIRST: ut_run<TR_Q_FIRST>(v, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
        case TR_Q_CLOSEST: ut_run<TR_Q_CLOSEST>(v, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
    }
    return -1;
}
// of the last query: rays whose stack lost a child
int64_t sim_uniform_top_lost(void) { return g_ut_lost; }
}
