// trip_model.cpp -- TEST-ONLY: plain_sim.cpp (included whole and unchanged: same builder, same views, same entry points)
// plus the walk the stealing kernels run since round 10 -- the fused trip over the grid nodes with the plain far-child
// stack BY LDS BYTE ADDRESS (tr_bvh.h: tr_plaina_w) -- ray by ray, with per-ray TRIP COUNTERS: the schedule of a lane
// of wave_traverse_steal below the give-away threshold (trips with and without the leaf block alternate, one leaf test
// per trip, a node visit only when the leaf FIFO has room).  A lane's trips do not depend on its neighbours there, so the
// trips of a wave are those of its longest lane: scripts/trip_model.py folds the per-ray counters into 8x8 tiles.
// A library of its own (libtrip_model.so, tests/host_sim/trip_sim.py).
#include "plain_sim.cpp"

static int64_t g_addr_lost = 0;

// per ray, 6 counters: trips, node visits, trips lost to a full FIFO / the alternation rule (a node was waiting and the
// trip could not visit it), trips with only queued leaves left, the trip at which the first hit was found (0 = none), far
// children on the stack at that moment
template <int Q>
static void run_addr(const tr_bvh_view& v, const float* o, const float* d, int64_t n, uint8_t* hit, uint8_t* front,
                     int32_t* tri, float* loc, float* uv, uint64_t* stats, int32_t* per_ray) {
    tr_counters cnt = {0, 0, 0};
    uint64_t tn = 0, tt = 0, tc = 0;
    for (int64_t i = 0; i < n; i++) {
        tr_ray r;
        const bool valid = tr_ray_setup_q(r, v.frame, o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        tr_result res;
        tr_topk<1> top;
        cnt.nodes = cnt.tris = cnt.climbs = 0;
        // four lanes' worth of interleaved slots; the ray walks as lane 2 (its slots are every fourth word)
        int32_t ring_mem[TR_RING * 4];
        const tr_ring ring = {ring_mem + 2, 4, ring_mem};
        const tr_aring ar = tr_aring_of(ring);
        int32_t trips = 0, stalls = 0, leaf_only = 0, first_hit = 0, entries = 0;
        tr_result_init(res);
        if (valid && v.num_tris >= 2) {
            tr_astate fs;
            tr_state_init(fs, tr_addr_start(ring));
            while (!tr_done(fs)) {
                const bool test = (trips & 1) == 0;
                const int32_t room = test ? fs.p2 : fs.p1;
                if (fs.node >= 0 && room >= 0) stalls++;
                if (fs.node < 0) leaf_only++;
                if (test) tr_fused_step<Q, 1, true, true, tr_plaina_w, false, true, true>(v, r, fs, res, top, &cnt, ring);
                else tr_fused_step<Q, 1, true, true, tr_plaina_w, false, false, true>(v, r, fs, res, top, &cnt, ring);
                trips++;
                if (!first_hit && res.best_face >= 0) { first_hit = trips; entries = (int32_t)tr_addr_slots(ar, fs.sa); }
            }
            if (tr_addr_lost(fs.sa)) {
                g_addr_lost++;
                tr_traverse_more<Q, 1, true>(v, r, res, top, &cnt);
            }
        }
        if (per_ray) {
            int32_t* p = per_ray + 6 * i;
            p[0] = trips; p[1] = (int32_t)cnt.nodes; p[2] = stalls; p[3] = leaf_only; p[4] = first_hit; p[5] = entries;
        }
        tn += cnt.nodes; tt += cnt.tris; tc += cnt.climbs;
        if (Q == TR_Q_ANY) hit[i] = res.best_face >= 0;
        if (Q == TR_Q_FIRST) tri[i] = res.best_face;
        if (Q == TR_Q_CLOSEST) {
            float l3[3] = {0, 0, 0}, u2[2] = {0, 0};
            hit[i] = res.best_face >= 0; front[i] = 0; tri[i] = res.best_face;
            if (res.best_face >= 0) {
                const tr_tri& t = v.tris[res.best_slot];
                front[i] = tr_hit_outputs(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, l3, u2);
            }
            memcpy(loc + 3 * i, l3, 12); memcpy(uv + 2 * i, u2, 8);
        }
    }
    stats[0] = (uint64_t)n; stats[1] = tn; stats[2] = tt; stats[3] = tc;
}

extern "C" {
// sim_plain_query's arguments plus `per_ray` (6 int32 per ray, or null): closest / first / any through the address form
int sim_addr_query(int q, const void* nodes, const void* links, const void* tris, int64_t nf, const float* o, const float* d,
                   int64_t n, uint8_t* hit, uint8_t* front, int32_t* tri, float* loc, float* uv, uint64_t* stats, int32_t* per_ray) {
    const tr_bvh_view v = view_of((const tr_node*)nodes, (const tr_link*)links, (const tr_tri*)tris, nf);
    g_addr_lost = 0;
    switch (q) {
        case TR_Q_ANY: run_addr<TR_Q_ANY>(v, o, d, n, hit, front, tri, loc, uv, stats, per_ray); return 0;
        case TR_Q_FIRST: run_addr<TR_Q_FIRST>(v, o, d, n, hit, front, tri, loc, uv, stats, per_ray); return 0;
        case TR_Q_CLOSEST: run_addr<TR_Q_CLOSEST>(v, o, d, n, hit, front, tri, loc, uv, stats, per_ray); return 0;
    }
    return -1;
}
int64_t sim_addr_lost() { return g_addr_lost; }
}
