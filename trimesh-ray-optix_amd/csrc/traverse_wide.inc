// traverse_wide.inc -- included by traverse.hip inside its anonymous namespace: construction of the 8-wide
// compressed nodes (tr_wide.h) from the binary hierarchy, and the streaming launch that walks them.
//
// ---- construction (on the first streaming query after a build / refit / load; derived data) --------------
// 1. k_wide_mark, one launch per three tree levels: the roots of the wide nodes (binary nodes at depth 0, 3, 6 ...
//    reached through internal nodes only) are flagged round by round from the root.
// 2. exclusive scan of the flags (the library's own scan kernels) = wide index of every root, in the order of the
//    binary node array -- the treelet layout, so the wide nodes are stored depth first as well.
// 3. k_wide_emit: one thread per root gathers its exits (tr_wexits) and writes the 96-byte record.

__global__ __launch_bounds__(256) void k_wide_mark(const tr_node* __restrict__ nodes, int64_t n, uint8_t* __restrict__ flag,
                                                   int round) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (round == 0) { flag[i] = i == 0 ? 1 : 0; return; }
    if (flag[i] != (uint8_t)round) return;
    const tr_node n0 = nodes[i];
    for (int s0 = 0; s0 < 2; s0++) {
        const int32_t c0 = s0 ? n0.c1 : n0.c0;
        if (c0 < 0) continue;
        const tr_node n1 = nodes[c0];
        for (int s1 = 0; s1 < 2; s1++) {
            const int32_t c1 = s1 ? n1.c1 : n1.c0;
            if (c1 < 0) continue;
            const tr_node n2 = nodes[c1];
            if (n2.c0 >= 0) flag[n2.c0] = (uint8_t)(round + 1);
            if (n2.c1 >= 0) flag[n2.c1] = (uint8_t)(round + 1);
        }
    }
}

__global__ __launch_bounds__(256) void k_wide_emit(const tr_node* __restrict__ nodes, int64_t n, const uint8_t* __restrict__ flag,
                                                   const int64_t* __restrict__ widx, tr_wnode* __restrict__ wnodes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || flag[i] == 0) return;
    tr_wexit ex[8];
    const int ne = tr_wexits(nodes, (int32_t)i, ex);
    tr_wnode w;
    tr_wnode_make(ex, ne, widx, &w);
    wnodes[widx[i]] = w;
}

// ---- traversal --------------------------------------------------------------------------------------------
// One ray per lane, persistent waves with ballot / mbcnt refill exactly as k_query_stream; the per-ray state is two
// STACKS of 32-bit items instead of trail word + far-child ring: wide nodes still to visit (TR_WNODES entries per
// lane in LDS -- entry k of lane t at [k * BS + t]: conflict free -- the rest, 7 per wide level is the bound, in a
// per-lane spill row in global memory that ordinary rays never touch; option wide_stack lowers the LDS part so that
// tests reach it) and leaves still to test (TR_WLEAVES entries in LDS; a lane visits a node only while eight more
// leaves fit, so this one never overflows).  A FUSED trip like the binary kernels': every lane that has a leaf
// tests one (full predicate, tr_tri_hit) and every lane that has a node and room visits one -- six 16-byte gathers,
// the <= 8 child boxes decoded and tested, hit leaves pushed, hit internal children pushed with the nearest of
// them last (it is popped first).
// Child box test: the planes a ray ENTERS through (lo where its direction is positive, hi where negative) and the
// ones it leaves through are selected per ray before anything is decoded (min(t1, t2) IS the entry plane's t when the
// reciprocal's sign is known), so that a child costs 6 conversions, 6 fma (the fused form below), one max3 and one
// min3, pairs of children in packed FP32.
constexpr int TR_WNODES = 12;
constexpr int TR_WLEAVES = 12;
constexpr int TR_WSTACK = TR_WNODES;     // (host: LDS part of the node stack)

// one fused trip of one lane (all 64 lanes of the wave call it together): test one queued leaf, visit one node
typedef __attribute__((address_space(3))) int32_t tr_wlds_i32;
template <int Q, int K, bool STATS, int BS>
__device__ __forceinline__ void wide_trip(const tr_bvh_view& b, const tr_wnode* __restrict__ wn, tr_ray& r, int& sn, int& nl,
                                          tr_result& res, tr_topk<K>& top, tr_counters& cnt, tr_wlds_i32* const nstk,
                                          tr_wlds_i32* const lstk, int32_t* const myspill, const int lds_cap) {
    typedef float tr_v2 __attribute__((ext_vector_type(2)));
    auto push_node = [&](int32_t v) {
        if (sn < lds_cap) nstk[sn * BS] = v;
        else myspill[sn - lds_cap] = v;
        sn++;
    };
    // ---- leaf block: one queued leaf per lane
    const bool is_leaf = nl > 0;
    int32_t pe = -1;      // a test the float32 part leaves undecided: decided at the end of the trip (tr_fold_leaf, tr_bvh.h)
    if (__ballot(is_leaf) != 0ull) {
        int32_t slot = 0;
        if (is_leaf) { nl--; slot = lstk[nl * BS]; }
        tr_counters* nc = nullptr;
        const tr_tri t = tr_load_tri<false, true>(b, slot, nc);
        if (STATS && is_leaf) cnt.tris++;
        if (tr_fold_leaf<Q, K>(is_leaf, r, t, slot, res, top, pe) && Q == TR_Q_ANY) { sn = 0; nl = 0; }     // the first accepted hit ends the ray
    }
    // ---- node block: one node per lane that has one and room for eight more leaves
    const bool is_node = sn > 0 && nl <= TR_WLEAVES - 8;
    if (__ballot(is_node) != 0ull) {
        int32_t item = 0;
        if (is_node) {
            sn--;
            item = sn < lds_cap ? nstk[sn * BS] : myspill[sn - lds_cap];
        }
        if (STATS && is_node) cnt.nodes++;
        const uint32_t off = (uint32_t)item * (uint32_t)sizeof(tr_wnode);
        const tr_i4* p = reinterpret_cast<const tr_i4*>(reinterpret_cast<const char*>(wn) + off);
        const tr_i4 h = p[0], q0 = p[1], q1 = p[2], q2 = p[3], ia = p[4], ib = p[5];
        const uint32_t ew = (uint32_t)h.w;
        const int nch = (int)(ew >> 24);
        const float lim = tr_cull_limit<Q>(res);
        // entry / exit plane bytes per axis (two dwords = children 0-3, 4-7 each)
        const uint32_t lo[3][2] = {{(uint32_t)q0.x, (uint32_t)q0.y}, {(uint32_t)q0.z, (uint32_t)q0.w}, {(uint32_t)q1.x, (uint32_t)q1.y}};
        const uint32_t hi[3][2] = {{(uint32_t)q1.z, (uint32_t)q1.w}, {(uint32_t)q2.x, (uint32_t)q2.y}, {(uint32_t)q2.z, (uint32_t)q2.w}};
        const bool ng[3] = {r.ix < 0.f, r.iy < 0.f, r.iz < 0.f};      // towards -x / -y / -z: the ray enters a box through its hi plane
        const float sc[3] = {tr_wscale(ew & 0xffu), tr_wscale((ew >> 8) & 0xffu), tr_wscale((ew >> 16) & 0xffu)};
        const float bs[3] = {__int_as_float(h.x), __int_as_float(h.y), __int_as_float(h.z)};
        const float ro[3] = {r.ox, r.oy, r.oz};
        // Round 5, the fused conservative form (tr_ray_fuse, tr_bvh.h): the node's frame is folded into per-visit
        // constants -- A = scale * k, B = (base - o) * k -+ e: four instructions per axis -- and a plane costs ONE fma
        // instead of decode, subtract, multiply: 24 packed fma per visit instead of 72 packed instructions, no pad
        // multiplies.  e is the ray's margin for the whole mesh (every plane of every node lies within the mesh's box
        // grown by one extent, which M accounts for), so the fused interval contains the contract's.
        const float rk[3] = {r.kx, r.ky, r.kz}, re[3] = {r.ex, r.ey, r.ez};
        float fA[3], fN[3], fF[3];
#pragma unroll
        for (int k = 0; k < 3; k++) tr_wfuse_axis(bs[k], sc[k], ro[k], rk[k], re[k], fA[k], fN[k], fF[k]);
        const int32_t ids[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
        // the entry- and exit-plane dwords of the three axes (selected once per visit)
        uint32_t en[3][2], ex[3][2];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int dw = 0; dw < 2; dw++) { en[k][dw] = ng[k] ? hi[k][dw] : lo[k][dw]; ex[k][dw] = ng[k] ? lo[k][dw] : hi[k][dw]; }
        uint32_t hits = 0;
        float near_t = INFINITY;
        int near_c = -1;
        int32_t near_id = -1;
        // two children at a time (packed FP32), all three axes of the pair before the next pair: few live values
#pragma unroll
        for (int pair = 0; pair < 4; pair++) {
            const int dw = pair >> 1, sh = 16 * (pair & 1);
            tr_v2 tn2 = {-INFINITY, -INFINITY}, tf2 = {INFINITY, INFINITY};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const tr_v2 qn = {(float)((en[k][dw] >> sh) & 0xffu), (float)((en[k][dw] >> (sh + 8)) & 0xffu)};
                const tr_v2 qx = {(float)((ex[k][dw] >> sh) & 0xffu), (float)((ex[k][dw] >> (sh + 8)) & 0xffu)};
                const tr_v2 a2 = {fA[k], fA[k]}, n2 = {fN[k], fN[k]}, f2 = {fF[k], fF[k]};
                const tr_v2 a = __builtin_elementwise_fma(qn, a2, n2);
                const tr_v2 z = __builtin_elementwise_fma(qx, a2, f2);
                tn2.x = fmaxf(tn2.x, a.x); tn2.y = fmaxf(tn2.y, a.y);
                tf2.x = fminf(tf2.x, z.x); tf2.y = fminf(tf2.y, z.y);
            }
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int c = 2 * pair + e;
                const float tn = e ? tn2.y : tn2.x;
                const float tf = e ? tf2.y : tf2.x;                      // (the exit margin is in fF)
                const bool hc = tr_slab_hit(tn, tf, lim) && is_node && c < nch;
                hits |= hc ? (1u << c) : 0u;
                if (hc && ids[c] >= 0 && tn < near_t) { near_t = tn; near_id = ids[c]; near_c = c; }
            }
        }
        // hit leaves -> leaf stack; hit internal children -> node stack, the nearest of them last
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (((hits >> c) & 1u) && ids[c] < 0) { lstk[nl * BS] = ~ids[c]; nl++; }
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (((hits >> c) & 1u) && ids[c] >= 0 && c != near_c) push_node(ids[c]);
        if (near_c >= 0) push_node(near_id);
    }
    if (tr_drain_exact<Q, K, true>(b, r, pe, res, top) && Q == TR_Q_ANY) { sn = 0; nl = 0; }
}

template <int Q, int BS, bool STATS>
__device__ __forceinline__ void query_wide_body(const tr_bvh_view& b, const tr_wnode* __restrict__ wn, const RayFetch& rf,
                                                const QueryOut& out, int rays_per_wave, int refill_min,
                                                const int* __restrict__ sel, unsigned long long* work,
                                                int32_t* __restrict__ spill, int spill_cap, int lds_cap,
                                                unsigned long long* stats) {
    if (sel && *sel != 1) return;      // dual launch: this is the shape for incoherent batches (id 1)
    __shared__ int32_t stack_lds[(TR_WNODES + TR_WLEAVES) * BS];
    tr_wlds_i32* const nstk = (tr_wlds_i32*)stack_lds + threadIdx.x;
    tr_wlds_i32* const lstk = (tr_wlds_i32*)stack_lds + TR_WNODES * BS + threadIdx.x;
    int32_t* const myspill = spill ? spill + ((size_t)blockIdx.x * BS + threadIdx.x) * (size_t)spill_cap : nullptr;
    const int64_t wave = (int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
    int64_t next = wave * rays_per_wave;                 // wave-uniform cursor into the wave's range
    int64_t end = next + rays_per_wave;
    if (end > rf.n) end = rf.n;
    bool exhausted = work == nullptr;
    const unsigned long long first_dynamic = (unsigned long long)gridDim.x * (BS / 64) * (unsigned long long)rays_per_wave;
    if (next >= rf.n) { next = 0; end = 0; }
    int64_t rid = -1;          // ray this lane holds (-1 none); its result is stored when the lane is refilled
    int sn = 0, nl = 0;        // fill of the node stack / the leaf stack; busy <=> sn + nl > 0
    tr_ray r;
    tr_result res;
    tr_counters cnt = {0, 0, 0};
    constexpr int K = 1;
    tr_topk<1> top;
    tr_result_init(res);
    tr_ray_setup_q(r, b.frame, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
    auto push_node = [&](int32_t v) {
        if (sn < lds_cap) nstk[sn * BS] = v;
        else myspill[sn - lds_cap] = v;
        sn++;
    };
    for (;;) {
        if (!exhausted && next >= end) {
            unsigned long long base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(work, (unsigned long long)rays_per_wave) + first_dynamic;
            base = __shfl(base, 0);
            if (base >= (unsigned long long)rf.n) {
                exhausted = true;
            } else {
                next = (int64_t)base;
                end = next + rays_per_wave;
                if (end > rf.n) end = rf.n;
            }
        }
        const unsigned long long idle = __ballot(sn + nl == 0);
        const int nidle = __popcll(idle);
        const bool more = next < end;
        if (!more && nidle == 64) break;
        if (more && (nidle >= refill_min || nidle == 64)) {
            if (sn + nl == 0) {
                if (rid >= 0) write_result<Q>(b, out, rid, r, res);      // the finished ray of this lane
                const int64_t cand = next + lane_rank(idle);
                rid = -1;
                if (cand < end) {
                    rid = cand;
                    float o[3], d[3];
                    fetch_ray(rf, cand, o, d);
                    const bool valid = tr_ray_setup_q(r, b.frame, o[0], o[1], o[2], d[0], d[1], d[2]);
                    tr_result_init(res);
                    if (b.num_tris >= 2) { if (valid) push_node(0); }
                    else brute_one<Q>(b, r, valid, res);                 // no hierarchy below two triangles
                }
            }
            next += nidle;     // lanes past `end` took nothing; the cursor only has to reach `end`
        }
        const int stop = (next < end || !exhausted) ? refill_min : 64;
        int idle_now;
        do {
            wide_trip<Q, K, STATS, BS>(b, wn, r, sn, nl, res, top, cnt, nstk, lstk, myspill, lds_cap);
            TR_CONVERGE();
            idle_now = __popcll(__ballot(sn + nl == 0));
        } while (idle_now < stop);
    }
    if (rid >= 0) write_result<Q>(b, out, rid, r, res);
    flush_stats<STATS>(cnt, stats);
}

// Round 5: five waves per SIMD (96 registers) where the compiler's own budget is 101-106 (four waves): the fused box
// test's per-visit constants sit on top of two stacks' worth of state; as with the streaming launch on the binary nodes
// the values that go to scratch are kernel-lifetime ones (prologue / refill path, none inside the trips:
// tests/test_round4_cpu.py) -- C5(ii) shard on wide nodes 1.814 -> 1.786 ms, shard count 2.419 -> 2.242, 5.2 M triangles
// 2.255 -> 2.246 (profiles/r05_ab_wide_waves.txt).  (The instrumented launches walk the binary nodes.)
#ifndef TR_WIDE_WAVES
#define TR_WIDE_WAVES 5
#endif
#if TR_WIDE_WAVES > 0
#define TR_WIDE_OCC __attribute__((amdgpu_waves_per_eu(TR_WIDE_WAVES, TR_WIDE_WAVES)))
#else
#define TR_WIDE_OCC
#endif
template <int Q>
__global__ __launch_bounds__(128) TR_WIDE_OCC void k_query_wide(tr_bvh_view b, const tr_wnode* __restrict__ wn, RayFetch rf, QueryOut out,
                                                    int rays_per_wave, int refill_min, const int* __restrict__ sel,
                                                    unsigned long long* work, int32_t* __restrict__ spill, int spill_cap,
                                                    int lds_cap, unsigned long long* stats) {
    TR_VIEW_LIVE(b);
    query_wide_body<Q, 128, false>(b, wn, rf, out, rays_per_wave, refill_min, sel, work, spill, spill_cap, lds_cap, stats);
}
// ---- the same walk for the DIRECT launch (one ray per lane for the life of the wave; query_direct_body MODE 4) ----
// The unordered queries on image tiles are bound by VALU issue (C4 count: 19 687 VALU instructions per wave, the host
// model of profiles/r04_packet_count_model.jsonl to 2 %): 148 visits of 32-byte nodes per ray at ~100 instructions
// each.  The 8-wide walk visits a third as many records -- the same exits, three levels at a time.
struct tr_wide_args {
    const tr_wnode* wn;
    int32_t* spill;
    int spill_cap, lds_cap;
};
template <int Q, int K, bool STATS, int BS>
__device__ __forceinline__ void wave_traverse_wide(const tr_bvh_view& b, const tr_wide_args& wa, tr_ray& r, bool go,
                                                   tr_result& res, tr_topk<K>& top, tr_counters& cnt, int32_t* stack_lds) {
    tr_wlds_i32* const nstk = (tr_wlds_i32*)stack_lds + threadIdx.x;
    tr_wlds_i32* const lstk = (tr_wlds_i32*)stack_lds + TR_WNODES * BS + threadIdx.x;
    int32_t* const myspill = wa.spill ? wa.spill + ((size_t)blockIdx.x * BS + threadIdx.x) * (size_t)wa.spill_cap : nullptr;
    tr_result_init(res);
    if (Q == TR_Q_LOCATION) top.init();
    int sn = 0, nl = 0;
    if (go) { nstk[0] = 0; sn = 1; }
    while (__ballot(sn + nl > 0) != 0ull) {
        wide_trip<Q, K, STATS, BS>(b, wa.wn, r, sn, nl, res, top, cnt, nstk, lstk, myspill, wa.lds_cap);
        TR_CONVERGE();
    }
}
