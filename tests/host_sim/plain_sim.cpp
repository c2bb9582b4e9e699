// plain_sim.cpp -- TEST-ONLY: the host simulation (host_sim.cpp, included whole: same builder, same views, same entry points)
// plus ONE more schedule: the fused trip over the 32-byte grid nodes with the PLAIN far-child stack (tr_bvh.h: tr_plain_w),
// as the stealing closest / first / any launch runs it, ray by ray -- and, for a ray whose stack lost a far child, the
// second, stackless traversal from its best hit so far (tr_traverse_more).  A library of its own (libplain_sim.so,
// tests/host_sim/plain_sim.py) so that host_sim.cpp and its modes stay exactly what they are.
#include "host_sim.cpp"

static int64_t g_plain_lost = 0;   // rays of the last sim_plain_query whose stack lost a far child

template <int Q>
static void run_plain(const tr_bvh_view& v, const float* o, const float* d, int64_t n, uint8_t* hit, uint8_t* front,
                      int32_t* tri, float* loc, float* uv, uint64_t* stats) {
    tr_counters cnt = {0, 0, 0};
    uint64_t tn = 0, tt = 0, tc = 0;
    for (int64_t i = 0; i < n; i++) {
        tr_ray r;
        const bool valid = tr_ray_setup_q(r, v.frame, o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        tr_result res;
        tr_topk<1> top;
        cnt.nodes = cnt.tris = cnt.climbs = 0;
        int32_t ring_mem[TR_RING];
        const tr_ring ring = {ring_mem, 1};
        tr_result_init(res);
        if (valid && v.num_tris >= 2) {
            tr_pstate fs;
            tr_state_init(fs);
            // as the kernels run it: trips with and without the leaf block alternate
            while (!tr_done(fs)) {
                tr_fused_step<Q, 1, true, true, tr_plain_w, false, true, true>(v, r, fs, res, top, &cnt, ring);
                if (!tr_done(fs)) tr_fused_step<Q, 1, true, true, tr_plain_w, false, false, true>(v, r, fs, res, top, &cnt, ring);
            }
            if (tr_plain_lost(fs.sp)) {
                g_plain_lost++;
                tr_traverse_more<Q, 1, true>(v, r, res, top, &cnt);
            }
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
// closest / first / any (q = TR_Q_*) of a hierarchy of at least two triangles; the grid nodes come from sim_set_qnodes.
// stats = rays, node visits, leaf tests, climbs (the climbs are the second traversals': the plain walk has none)
int sim_plain_query(int q, const void* nodes, const void* links, const void* tris, int64_t nf, const float* o, const float* d,
                    int64_t n, uint8_t* hit, uint8_t* front, int32_t* tri, float* loc, float* uv, uint64_t* stats) {
    const tr_bvh_view v = view_of((const tr_node*)nodes, (const tr_link*)links, (const tr_tri*)tris, nf);
    g_plain_lost = 0;
    switch (q) {
        case TR_Q_ANY: run_plain<TR_Q_ANY>(v, o, d, n, hit, front, tri, loc, uv, stats); return 0;
        case TR_Q_FIRST: run_plain<TR_Q_FIRST>(v, o, d, n, hit, front, tri, loc, uv, stats); return 0;
        case TR_Q_CLOSEST: run_plain<TR_Q_CLOSEST>(v, o, d, n, hit, front, tri, loc, uv, stats); return 0;
    }
    return -1;
}
int64_t sim_plain_lost() { return g_plain_lost; }
}
