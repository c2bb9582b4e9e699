// descent_model.cpp -- TEST-ONLY: plain_sim.cpp (included whole and unchanged: same builder, same views, same entry points)
// plus the stealing grid-node launch WAVE BY WAVE, below the give-away threshold: rays in groups of 64, the wave's loop
// and exit rule as wave_traverse_steal has them (kernels_direct.inc), driven through the product's own tr_descent_step and
// tr_fused_step (tr_bvh.h: the plain stack by LDS byte address over the grid nodes).  Two forms of the same wave:
//   variant 0: the general loop alone -- rounds of four trips, with and without the leaf block in turn;
//   variant 1: the descent phase in front of it, as the kernels run it: tr_descent_step until some lane of the wave accepts
//              a leaf child (or no lane has a node, or the trip reaches `steal_min`), that trip's leaves entered into the
//              empty FIFOs, then the general loop from where the schedule stands;
// and two deliberately WRONG forms, so that the test that compares the variants can show that it has bite:
//   variant 2: the second leaf of the phase's last trip is dropped;
//   variant 3: the general loop is entered with the wrong flavour of trip after a phase that ended on an odd trip.
// Per ray: outputs, node visits, leaf tests, the lost flag.  Per group: the trip that accepted the wave's first leaf, the
// leading trips on which every visiting lane was at the same node, the trips of the longest lane, the phase's trips.
// A library of its own (libdescent_model.so, tests/host_sim/descent_sim.py).
#include "plain_sim.cpp"

namespace {
struct dm_lane {
    tr_ray r;
    bool valid;
    tr_result res;
    tr_astate fs;
    tr_counters cnt;
    int32_t ring_mem[TR_RING * 4];      // four lanes' worth of interleaved slots; the ray walks as lane 2 (trip_model.cpp)
    tr_ring ring;
    int32_t lost_trip;                  // the trip (from 1) whose push found the stack full, 0 = none
};

struct dm_wave {
    int32_t trips = 0;                  // trips run so far
    int32_t first_leaf = 0;             // the trip after which some lane held a leaf for the first time, 0 = none
    int32_t uniform = 0;                // leading leaf-free trips on which all visiting lanes were at one node
    bool uniform_on = true;
    int32_t longest = 0;                // the last trip some lane took part in
    int32_t phase = 0;                  // trips of the descent phase
    int32_t lost_in_phase = 0;          // rays whose stack lost a child inside the phase
};

// bookkeeping in front of a trip: does anybody take part, and are the visiting lanes at one node?
void dm_before(dm_lane* L, int m, dm_wave& w) {
    bool busy = false, same = true;
    int32_t at = -1;
    for (int k = 0; k < m; k++) {
        if (!tr_done(L[k].fs)) busy = true;
        if (L[k].fs.node >= 0) {
            if (at < 0) at = L[k].fs.node;
            else if (at != L[k].fs.node) same = false;
        }
    }
    w.trips++;
    if (busy) w.longest = w.trips;
    if (w.uniform_on && w.first_leaf == 0 && same && at >= 0) w.uniform++;
    else w.uniform_on = false;
}
void dm_after(dm_lane* L, int m, dm_wave& w) {
    for (int k = 0; k < m; k++) {
        if (!L[k].lost_trip && tr_addr_lost(L[k].fs.sa)) L[k].lost_trip = w.trips;
        if (!w.first_leaf && L[k].fs.p0 >= 0) w.first_leaf = w.trips;
    }
}

template <int Q, bool TEST>
void dm_general(const tr_bvh_view& v, dm_lane* L, int m, dm_wave& w) {
    dm_before(L, m, w);
    for (int k = 0; k < m; k++) {
        tr_topk<1> top;
        if (!tr_done(L[k].fs)) tr_fused_step<Q, 1, true, true, tr_plaina_w, false, TEST, true>(v, L[k].r, L[k].fs, L[k].res, top, &L[k].cnt, L[k].ring);
    }
    dm_after(L, m, w);
}

// wave_traverse_steal below the give-away threshold, statement by statement
template <int Q>
void dm_wave_run(const tr_bvh_view& v, dm_lane* L, int m, int variant, uint32_t steal_min, dm_wave& w) {
    uint32_t trip = 0, k0 = 0;
    if (variant >= 1) {
        bool l0[64], l1[64];
        int32_t c0[64], c1[64];
        for (int k = 0; k < m; k++) { l0[k] = l1[k] = false; c0[k] = c1[k] = 0; }
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
        for (int k = 0; k < m; k++) {
            L[k].fs.p0 = l0[k] ? ~c0[k] : (l1[k] ? ~c1[k] : -1);
            L[k].fs.p1 = (l0[k] && l1[k] && variant != 2) ? ~c1[k] : -1;
        }
        if (w.phase) dm_after(L, m, w);      // (the last trip's first leaf, now that the FIFOs are written)
        if (trip & 1u) {
            if (variant != 3) dm_general<Q, false>(v, L, m, w);
            trip++;
        }
        k0 = trip == 0u ? 0u : ((trip - 1u) & 3u) + 1u;
        trip -= k0;
    }
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

int64_t g_dm_extra[3];

template <int Q>
void dm_run(const tr_bvh_view& v, int variant, uint32_t steal_min, const float* o, const float* d, int64_t n, uint8_t* hit,
            uint8_t* front, int32_t* tri, float* loc, float* uv, uint64_t* stats, int32_t* per_ray, int32_t* per_group) {
    static dm_lane L[64];
    uint64_t tn = 0, tt = 0;
    g_dm_extra[0] = g_dm_extra[1] = g_dm_extra[2] = 0;
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
        if (v.num_tris >= 2) dm_wave_run<Q>(v, L, m, variant, steal_min, w);
        if (per_group) {
            int32_t* p = per_group + 4 * (g0 / 64);
            p[0] = w.first_leaf; p[1] = w.uniform; p[2] = w.longest; p[3] = w.phase;
        }
        g_dm_extra[2] += w.lost_in_phase;
        for (int k = 0; k < m; k++) {
            const int64_t i = g0 + k;
            dm_lane& l = L[k];
            const bool lost = tr_addr_lost(l.fs.sa);
            if (per_ray) { per_ray[3 * i] = (int32_t)l.cnt.nodes; per_ray[3 * i + 1] = (int32_t)l.cnt.tris; per_ray[3 * i + 2] = lost; }
            tn += l.cnt.nodes; tt += l.cnt.tris;
            if (lost) {
                g_dm_extra[0]++;
                if (l.lost_trip && (w.first_leaf == 0 || l.lost_trip < w.first_leaf)) g_dm_extra[1]++;
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
// sim_plain_query's arguments plus the variant (above), the give-away threshold, `per_ray` (3 int32 per ray: node visits,
// leaf tests, lost; or null) and `per_group` (4 int32 per group of 64 rays: first-leaf trip, uniform leading trips, trips
// of the longest lane, trips of the descent phase; or null).  stats = rays, node visits, leaf tests of the walk itself (the
// second traversal of a lost ray is not counted).
int sim_descent_query(int q, int variant, uint32_t steal_min, const void* nodes, const void* links, const void* tris, int64_t nf,
                      const float* o, const float* d, int64_t n, uint8_t* hit, uint8_t* front, int32_t* tri, float* loc, float* uv,
                      uint64_t* stats, int32_t* per_ray, int32_t* per_group) {
    const tr_bvh_view v = view_of((const tr_node*)nodes, (const tr_link*)links, (const tr_tri*)tris, nf);
    switch (q) {
        case TR_Q_ANY: dm_run<TR_Q_ANY>(v, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
        case TR_Q_FIRST: dm_run<TR_Q_FIRST>(v, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
        case TR_Q_CLOSEST: dm_run<TR_Q_CLOSEST>(v, variant, steal_min, o, d, n, hit, front, tri, loc, uv, stats, per_ray, per_group); return 0;
    }
    return -1;
}
// of the last query: rays whose stack lost a child; of those, the ones that lost it before the trip that gave their group
// its first leaf; and (variants >= 1) the ones that lost it inside the descent phase
void sim_descent_extra(int64_t* out3) { out3[0] = g_dm_extra[0]; out3[1] = g_dm_extra[1]; out3[2] = g_dm_extra[2]; }
}
