// kernels_direct.inc -- included by traverse.hip inside its anonymous namespace: the DIRECT launch (one workgroup per
// 128 rays): the wave-level drivers of the per-lane state machine (tr_bvh.h) -- plain, with intra-wave work stealing,
// the unordered two-phase schedule with and without stealing --, the block -> ray map (XCD chunks, tiles, learned
// order, split slots), k_query_direct / k_query_direct_wide and the kernels that learn the launch order.
// Wave-level traversal of one ray per lane with the fused, software-pipelined trip
// (tr_fused_step): every lane advances on every trip; results do not depend on the schedule
// (the hit predicate is order-independent, tr_math.h).
template <bool C, bool DEEP = false> struct tr_word { typedef uint64_t T; };
template <> struct tr_word<true, false> { typedef uint32_t T; };

// COMPACT = both arrays are below 4 GiB: SGPR-base + 32-bit-offset loads; and, unless DEEP (the
// hierarchy is more than 32 levels high), 32-bit trail / owned words.  Chosen on the host per BVH.
// COMPACT + DEEP is what meshes of a few million triangles and more get (5.2 M-triangle sphere: 34
// levels): 80 instead of 82 VGPRs in the stealing closest kernel, i.e. 6 instead of 5 waves/SIMD.
constexpr bool TR_STREAM_QN = true;     // the streaming launch walks the 32-byte grid nodes (tr_rec_q)
// the drain of parked leaf tests as a cold branch (tr_drain_exact): everywhere but in the streaming closest kernel on the
// binary nodes, which answers the hint with ten spills (C3 closest +6 %: profiles/r06_ab_cold_drain.txt)
template <int Q> constexpr bool TR_STREAM_COLD = Q != TR_Q_CLOSEST;
template <int Q, int K, bool STATS, bool COMPACT = false, bool UNI = false, bool DEEP = false>
__device__ __forceinline__ void wave_traverse(const tr_bvh_view& b, tr_ray& r, bool go,
                                              tr_result& res, tr_topk<K>& top, tr_counters* cnt,
                                              const tr_ring ring) {
    tr_result_init(res);
    if (Q == TR_Q_LOCATION) top.init();
    // fused, software-pipelined schedule: every lane advances on every trip
    typedef typename tr_word<COMPACT, DEEP>::T W;
    tr_state_t<W> fs;
    tr_state_init(fs);
    if (!go) fs.node = -1;
    while (!tr_done(fs)) {
        tr_fused_step<Q, K, STATS, COMPACT, W, UNI, true>(b, r, fs, res, top, cnt, ring);
        TR_CONVERGE();
        tr_fused_step<Q, K, STATS, COMPACT, W, UNI, false>(b, r, fs, res, top, cnt, ring);   // no-op for a finished lane
        TR_CONVERGE();
    }
}

// ---- intra-wave work stealing ------------------------------------------------------------------
// A wave runs until its slowest ray is done; on the headline batch that is 334 trips for one
// grazing ray while the other 63 lanes finished after 30-60.  Here an idle lane takes the
// SHALLOWEST owed far child (the biggest untouched subtree) of a busy lane together with that
// lane's ray and traverses it as an independent sub-traversal (empty trail: it ends when the
// subtree is exhausted); the per-ray results are merged at the end of the wave by the same
// (t_key, face) minimum (closest / first) or by summation (count).  Any partition of the tree
// among lanes examines the same set of candidate triangles except for culling, so results are
// bit-identical.  Donors are rays that are still busy at their `steal_min`-th trip (64): by then a
// primary ray has normally found its hit (the thief inherits that bound), and what is left are
// the grazing rays that make the long waves.  Splitting earlier costs culling (-6 % at 48, -15 %
// at 32 on the headline).  wl = 6*64 ints of LDS scratch per wave.
constexpr uint32_t TR_STEAL_EVERY = 3u;     // hand-overs are attempted on every (TR_STEAL_EVERY+1)-th trip ...
constexpr uint32_t TR_STEAL_EARLY = 4u;     // ... and the trip from which a wave of UNRELATED rays gives subtrees away (wave_traverse_steal): its first look
constexpr int TR_STEAL_IDLE = 1;            // ... when at least this many lanes are idle
__device__ __forceinline__ int lane_rank(unsigned long long mask) {   // set bits of mask below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// (Round 3's LDS-staged table of the top levels -- a lockstep descent through 4 KiB of LDS -- and its slim hand-over
// for an eighth wave per SIMD measured slower or equal on every config and were retired in round 5 with their options
// lds_top / occ8: profiles/r03_ab_lds_top.jsonl, r03_ab_occ8.txt, r04_ab_qsign.txt.)
template <int Q, bool STATS, bool COMPACT, bool DEEP = false, bool QN = false>
__device__ __forceinline__ bool wave_traverse_steal(const tr_bvh_view& b, tr_ray& r, bool go,
                                                    tr_result& res, tr_counters* cnt,
                                                    const tr_ring ring, int32_t* wl, int lane,
                                                    uint32_t steal_min, bool& lost) {
    // the grid-node launch walks with the plain far-child stack, its stack pointer an LDS byte address (tr_plaina_w,
    // tr_bvh.h: no trail words, so DEEP is the same code); the launch on the exact nodes (option grid_nodes = 0) keeps the
    // dense stack and never loses a child
    constexpr bool PLAIN = QN;
    typedef typename std::conditional<PLAIN, tr_plaina_w, typename tr_word<COMPACT, DEEP>::T>::type W;
    lost = false;
    tr_result_init(res);
    tr_topk<1> top;
    tr_state_t<W> fs;
    const tr_aring ar = tr_aring_of(ring);
    (void)ar;
    if constexpr (PLAIN) tr_state_init(fs, tr_addr_start(ring));
    else tr_state_init(fs);
    if (!go) fs.node = -1;
    auto trip_step = [&](auto test_tag) {
        constexpr bool TEST = decltype(test_tag)::value;
        if (!tr_done(fs)) tr_fused_step<Q, 1, STATS, COMPACT, W, false, TEST, QN>(b, r, fs, res, top, cnt, ring);
    };
    int owner = lane;          // lane whose ray this lane is working on
    bool split = false;        // wave-uniform: some ray is (or was) traversed by more than one lane
    uint32_t trip = 0;
    // Bit 15 of the threshold: ADAPTIVE (the automatic policy).  A wave of unrelated rays -- a flat batch of shadow or secondary
    // rays below the streaming launch's sizes -- gives subtrees away from trip TR_STEAL_EARLY on instead, i.e. from its first
    // look: its rays are short (12-14 node visits on average), lanes run dry from the start, and waiting for trip 64 leaves them
    // idle (1 M hash rays, trip 64 / 16 / 8 / 4: closest 0.218 / 0.177 / 0.163 / 0.160 ms on the 82 k-triangle mesh, any-hit
    // 0.198 / 0.155 / 0.139 / 0.134; headline mesh closest 0.270 / 0.213 / 0.203 / 0.200: profiles/r05_ab_steal_incoherent.txt),
    // while the waves of an image keep the late threshold that protects their culling (headline at 32: -15 %).  The wave decides for itself, once, with k_probe_coherence's test against its first ray: at
    // least three quarters of its rays within ~2.5 degrees and 1 % of the grid's diagonal of it.
    if (steal_min & 0x8000u) {
        steal_min &= 0x7fffu;
        const unsigned long long act = __ballot(go);
        if (act != 0ull) {
            const int l0 = (int)__builtin_ctzll(act);
            const float ax = __shfl(r.dx, l0), ay = __shfl(r.dy, l0), az = __shfl(r.dz, l0);
            const float bx = __shfl(r.ox, l0) - r.ox, by = __shfl(r.oy, l0) - r.oy, bz = __shfl(r.oz, l0) - r.oz;
            const float dd = ax * r.dx + ay * r.dy + az * r.dz;
            const float n0 = ax * ax + ay * ay + az * az, n1 = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
            const float ex = 65535.f * b.frame.scale[0], ey = 65535.f * b.frame.scale[1], ez = 65535.f * b.frame.scale[2];
            const bool alike = dd > 0.f && dd * dd >= 0.998f * n0 * n1 && bx * bx + by * by + bz * bz <= 1e-4f * (ex * ex + ey * ey + ez * ez);
            if (4 * __popcll(__ballot(go && alike)) < 3 * __popcll(act) && steal_min > TR_STEAL_EARLY) steal_min = TR_STEAL_EARLY;
        }
    }
    // explicit LDS pointers: volatile accesses through generic pointers would compile to flat
    // loads/stores with 64-bit addresses held in VGPRs for the whole loop
    typedef __attribute__((address_space(3))) volatile int32_t lds_i32;
    typedef __attribute__((address_space(3))) volatile unsigned long long lds_u64;
    lds_i32* const lw = (lds_i32*)wl;
    lds_i32* const list = lw;                    // [64] donor lane of pair k
    lds_i32* const xnode = lw + 64;              // [64] node handed over by donor lane
    // [64] dense stack: the depth of the node handed over.  Plain stack: per lane, bits 0-7 = entries this lane has given
    // away since its stack was last empty (`bot`, tr_addr_give), bit 8 = a lane that worked on THIS lane's ray lost a
    // far child (set by that lane when it hands its results in)
    lds_i32* const xdepth = lw + 128;
    int32_t* const xflags = wl + 128;
    if constexpr (PLAIN) xdepth[lane] = 0;
    // per-ray accumulators at the owner's index: partial results are deposited whenever a lane
    // finishes a piece of work (before it takes the next one) and once more at the end
    constexpr int ACC = 192;
    int32_t* sum = wl + ACC;                                                        // count
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(wl + ACC);   // closest / first
    lds_i32* const vsum = lw + ACC;
    lds_u64* const vkeys = (lds_u64*)(lw + ACC);
    lds_i32* const vslots = lw + ACC + 128;
    auto deposit = [&]() {
        if constexpr (PLAIN) {
            if (tr_addr_lost(fs.sa)) atomicOr(&xflags[owner], 0x100);
        }
        if (Q == TR_Q_COUNT) {
            if (res.count) atomicAdd(&sum[owner], res.count);
        } else if (Q == TR_Q_ANY) {
            if (res.best_face >= 0) vsum[owner] = 1;      // any hit of any worker
        } else {
            const bool have = res.best_slot >= 0;
            // t_key >= 0, but tr_tri_mt can return -0.0f (a ray that starts exactly in a triangle's
            // plane): its bit pattern 0x80000000 would sort above every positive distance while
            // tr_closer treats it as equal to +0.0f.  Dropping the sign bit is exact for t_key >= 0
            // and makes the integer order of the key the (t_key, face) order of tr_closer.
            const unsigned long long key = ((unsigned long long)(__float_as_uint(res.best_t) & 0x7fffffffu) << 32) |
                                           (unsigned)res.best_face;
            if (have) atomicMin(&keys[owner], key);
            __builtin_amdgcn_wave_barrier();
            if (have && vkeys[owner] == key) vslots[owner] = res.best_slot;   // faces are distinct: one winner
        }
    };
    // DESCENT PHASE (plain stack): the tree is tens of levels deep and its leaves sit near the bottom, so the first leaf of a
    // wave shows up late (headline: after 22 of a wave's 48 trips, profiles/r11_descent_model.txt).  Until some lane has
    // accepted a leaf child every FIFO of the wave is empty and nothing is parked, and a trip of either flavour comes down to
    // fetch, box test, push / descend / pop: tr_descent_step, without the FIFO's selects, room / has_node, the wave-any test in
    // front of the leaf block, the drain and tr_done.  No node is skipped and nothing is reordered: every lane visits the nodes
    // it visits in the loop below, trip by trip, and the state handed over is the state that loop would have reached.  The
    // trip on which a lane accepts a leaf is not repeated: its leaves go into the empty FIFOs as either flavour would enter
    // them, and the loop below continues WHERE THE SCHEDULE STANDS -- a trip without the leaf block first when the phase ends
    // on an odd trip, then at pair `k0` of a round of trips, so that every look at the wave comes at the trip it came at
    // before.  The phase ends before the first look that could give anything away (trip >= steal_min): the looks it runs past
    // would have found a busy lane and nothing to do.
    uint32_t k0 = 0;           // the trips of the loop's first round that are over already (PLAIN: 0, 2 or all 4)
    if constexpr (PLAIN) {
        bool l0 = false, l1 = false;       // child 0 / 1 of the lane's last visit is an accepted leaf
        int32_t c0 = 0, c1 = 0;
        // UNIFORM TOP: under an 8x8 pixel tile the first trips of the phase find every visiting lane at the SAME node, from the
        // root on (headline: 12.7 of a wave's 48 trips, profiles/r11_descent_model.txt), and nearly every tile's rays point
        // into one octant.  On those trips the record, the children, their leaf flags and the choice of each axis' entry and
        // exit plane are the same in all 64 lanes: the record is read once through the scalar memory path (a uniform address
        // in the constant address space, as in tr_fused_step's UNI branch; read only -- every store stays a vector store or an
        // LDS write) and that work is done once on the scalar unit (tr_uniform_test, tr_uniform_wave), in place of the phase's two 64-lane
        // gathers of the same 32 bytes, its address shift, six v_perm_b32 and the sign tests on the children.  Per lane the
        // same fma per plane, the same box test and swap rule, the same push.  The octant test is paid ONCE per wave, against
        // the first lane that has a ray (lane 0 may have none); a wave that fails it goes straight to the phase.  The loop is
        // left after the first trip on which a lane accepts a leaf child, the lanes' next nodes differ, a lane has no child
        // to descend into (it pops here, once, outside the loop: no lane loses its node inside it, so the lanes with a node
        // are the lanes with `go` throughout) or the trip reaches `steal_min`; it leaves behind what the phase's own trips
        // would have: node and stack pointer per lane, the last trip's leaf report, the trip count.
        bool stop = false;                 // wave-uniform: the uniform top ended on a trip that ends the phase as well
        {
            const unsigned long long act = __ballot(go);
            if (act != 0ull && trip < steal_min) {
                const int first = (int)__builtin_ctzll(act);
                const uint32_t sn = (uint32_t)__builtin_amdgcn_readlane((int)r.sel_n, first);
                const uint32_t sf = (uint32_t)__builtin_amdgcn_readlane((int)r.sel_f, first);
                const uint32_t sz = (uint32_t)__builtin_amdgcn_readlane((int)r.sel_z, first);
                if (__ballot(go && (r.sel_n != sn || r.sel_f != sf || r.sel_z != sz)) == 0ull) {
                    const tr_uoctant oct = tr_uniform_octant(sn, sz);
                    int32_t nu = 0;        // the wave's node
                    tr_uwave u;
                    bool more = true;      // (one condition of bitwise terms, one branch: the short-circuit form is twenty scalar instructions longer)
                    // FLOAT TOP: while the wave's node has a slot in the handle's table (tr_bvh.h: tr_top_rec), the trip reads the
                    // record of (octant, slot) -- one 64-byte line, through the scalar memory path as below -- whose twelve planes
                    // are floats already and already the entry and exit planes of this octant: the packed fma take them from their
                    // scalar register pairs, and the selection and the conversions of tr_uniform_test are not run.  Same compares,
                    // same tr_uniform_wave, same push, same conditions to stop; the slot follows the child the wave goes to
                    // (2i + 1 / 2i + 2, as a byte offset).  Below the table (`more` still set) the loop behind goes on at `nu`.
                    if (b.top) {
                        typedef float tr_rec16 __attribute__((ext_vector_type(16)));      // a record as ONE load of sixteen dwords
                        typedef const __attribute__((address_space(4))) tr_rec16* tr_crecp;
                        typedef const __attribute__((address_space(4))) char* tr_cchp;
                        const tr_cchp tab = (tr_cchp)(unsigned long long)(b.top + tr_octant_index(sn, sz) * TR_TOP_SLOTS);
                        uint32_t off = 0;      // the slot's byte offset in its table
                        // (the table's last level as a trip count: the slot is inside the table for TR_TOP_LEVELS trips from the root)
                        const uint32_t lim = steal_min < trip + TR_TOP_LEVELS ? steal_min : trip + TR_TOP_LEVELS;
                        int32_t s0, s1;
                        bool on;               // nothing ends the uniform top
#pragma unroll 1
                        do {
                            const tr_rec16 w = *(tr_crecp)(tab + off);
                            float p[12];
#pragma unroll
                            for (int k = 0; k < 12; k++) p[k] = w[k];
                            s0 = (int32_t)__float_as_uint(w[12]); s1 = (int32_t)__float_as_uint(w[13]);
                            bool a0, a1, lt;
                            tr_top_test<Q>(r, p, res, a0, a1, lt);
                            if (STATS && go) cnt->nodes++;
                            u = tr_uniform_wave(act, __builtin_amdgcn_ballot_w64(a0), __builtin_amdgcn_ballot_w64(a1),
                                                __builtin_amdgcn_ballot_w64(lt), s0, s1);
                            c0 = s0; c1 = s1;
                            if (tr_lane_in(u.both, lane)) tr_addr_push(ar, fs.sa, tr_lane_in(u.sw, lane) ? c0 : c1);
                            TR_CONVERGE();
                            trip++;
                            on = ((u.l0 | u.l1 | u.pop) == 0ull) & ((u.sw == 0ull) | (u.sw == act));
                            off = 2u * off + (u.sw != 0ull ? 128u : 64u);
                        } while (on & (trip < lim));
                        more = on & (trip < steal_min);
                        nu = u.sw != 0ull ? s1 : s0;
                    }
                    if (more) {
#pragma unroll 1
                    do {
                        typedef const __attribute__((address_space(4))) int32_t* tr_ci32p;
                        const tr_ci32p sp = (tr_ci32p)(unsigned long long)tr_qnode_ptr<COMPACT>(b, nu);
                        tr_i4 w0, w1;
                        w0.x = sp[0]; w0.y = sp[1]; w0.z = sp[2]; w0.w = sp[3];
                        w1.x = sp[4]; w1.y = sp[5]; w1.z = sp[6]; w1.w = sp[7];
                        bool a0, a1, lt;
                        tr_uniform_test<Q>(r, w0, w1, oct, res, a0, a1, lt);
                        if (STATS && go) cnt->nodes++;
                        // (the ballots beside their compares, in front of the push's branch: each IS its compare's result register)
                        u = tr_uniform_wave(act, __builtin_amdgcn_ballot_w64(a0), __builtin_amdgcn_ballot_w64(a1),
                                            __builtin_amdgcn_ballot_w64(lt), w1.z, w1.w);
                        c0 = w1.z; c1 = w1.w;
                        if (tr_lane_in(u.both, lane)) tr_addr_push(ar, fs.sa, tr_lane_in(u.sw, lane) ? c0 : c1);
                        TR_CONVERGE();
                        trip++;
                        more = ((u.l0 | u.l1 | u.pop) == 0ull) & ((u.sw == 0ull) | (u.sw == act)) & (trip < steal_min);
                        nu = u.sw != 0ull ? c1 : c0;
                    } while (more);
                    }
                    l0 = tr_lane_in(u.l0, lane); l1 = tr_lane_in(u.l1, lane);
                    if (go) fs.node = tr_lane_in(u.sw, lane) ? c1 : c0;
                    if (tr_lane_in(u.pop, lane)) fs.node = tr_addr_pop(ar, fs.sa);
                    stop = (u.l0 | u.l1) != 0ull || !TR_WAVE_ANY(fs.node >= 0);
                }
            }
        }
        if (!stop) while (trip < steal_min) {
            l0 = false; l1 = false;
            if (fs.node >= 0) tr_descent_step<Q, STATS, COMPACT>(b, r, fs, res, cnt, ring, l0, l1, c0, c1);
            TR_CONVERGE();
            trip++;
            if (TR_WAVE_ANY(l0 || l1) || !TR_WAVE_ANY(fs.node >= 0)) break;
        }
        // the last trip's leaves, into FIFOs that are empty (no lane has any unless that trip found the wave's first)
        fs.p0 = l0 ? ~c0 : (l1 ? ~c1 : -1);
        fs.p1 = (l0 && l1) ? ~c1 : -1;
        if (trip & 1u) {
            trip_step(std::false_type{});
            TR_CONVERGE();
            trip++;
        }
        k0 = trip == 0u ? 0u : ((trip - 1u) & TR_STEAL_EVERY) + 1u;
        trip -= k0;
    }
    for (;;) {
        // TR_STEAL_EVERY+1 plain trips (idle lanes sit them out under the exec mask: a trip takes
        // longer the more lanes take part in its loads), in pairs of a trip with the leaf block and one
        // without (tr_fused_step<..., TEST>), then one look at the wave
#pragma unroll 1
        for (uint32_t k = k0; k <= TR_STEAL_EVERY; k += 2) {
            trip_step(std::true_type{});
            TR_CONVERGE();
            trip_step(std::false_type{});
            TR_CONVERGE();
        }
        k0 = 0;
        trip += (TR_STEAL_EVERY / 2u + 1u) * 2u;
        if (split) {
            // Rays that are traversed by several lanes share what they have found: a lane's bound is
            // the best hit of ANY lane working on its ray (closest / first), and an any-hit ray ends
            // for all of them with the first hit.  A bound that is a real hit of the same ray culls
            // exactly what the lane's own hit at that distance would cull, and the result is the
            // minimum (t_key, face) over all lanes either way -- but the subtrees given away early no
            // longer lose the culling the donor's later hits would have brought.
            if (Q == TR_Q_ANY) {
                if (res.best_face >= 0) vsum[owner] = 1;
                __builtin_amdgcn_wave_barrier();
                if (vsum[owner] != 0 && !tr_done(fs)) { fs.node = -1; fs.p0 = -1; fs.p1 = -1; fs.p2 = -1; }
            } else if (Q == TR_Q_CLOSEST || Q == TR_Q_FIRST) {
                const bool have = res.best_slot >= 0;
                const unsigned long long mine = ((unsigned long long)(__float_as_uint(res.best_t) & 0x7fffffffu) << 32) |
                                                (unsigned)(res.best_face < 0 ? 0x7fffffff : res.best_face);
                if (have) atomicMin(&keys[owner], mine);
                __builtin_amdgcn_wave_barrier();
                const unsigned long long k = vkeys[owner];
                if (have && k == mine) vslots[owner] = res.best_slot;
                if (k < mine) {     // another lane's hit: a bound, not a result of this lane
                    tr_set_best_t(res, __uint_as_float((unsigned)(k >> 32)));
                    res.best_face = (int32_t)(unsigned)k;
                    res.best_slot = -1;
                }
            }
        }
        const bool done = tr_done(fs);
        const unsigned long long idle = __ballot(done);
        if (idle == ~0ull) break;
        // the wave-uniform test first: below the threshold nobody gives, and the lanes' look at their stacks (an LDS round
        // trip for `bot`) would decide nothing -- a coherent wave of the headline is over after 48 trips on average
        if (__popcll(idle) >= TR_STEAL_IDLE && trip >= steal_min) {
            uint32_t bot = 0;
            bool has_far;                            // owed far children that are in the stack
            if constexpr (PLAIN) {
                bot = (uint32_t)xdepth[lane] & 0xffu;
                has_far = tr_addr_can_give(ar, fs.sa, bot);
            } else {
                has_far = (fs.trail & fs.owned) != 0;
            }
            const bool can_give = !done && has_far;
            const unsigned long long donors = __ballot(can_give);
            const int ni = __popcll(idle), nd = __popcll(donors);
            const int np = ni < nd ? ni : nd;
            if (np > 0) {
                if (!split) {   // first hand-over in this wave: set the accumulators up
                    if (Q == TR_Q_COUNT || Q == TR_Q_ANY) vsum[lane] = 0;
                    else vkeys[lane] = ~0ull;
                    split = true;
                    __builtin_amdgcn_wave_barrier();
                }
                const int drank = lane_rank(donors), irank = lane_rank(idle);
                const bool give = can_give && drank < np;
                int gnode = 0, gdepth = 0;
                (void)gdepth;
                if constexpr (PLAIN) {
                    if (give) {
                        // the shallowest = the bottom of the stack; -1 takes its place (tr_addr_give)
                        gnode = tr_addr_give(ar, fs.sa, bot);
                        list[drank] = lane; xnode[lane] = gnode;
                        atomicAdd(&xflags[lane], 1);
                    }
                } else if (give) {
                    // the shallowest = the bottom of the stack; its owned bit stays behind and keeps the others' slots (tr_ring)
                    uint32_t j;
                    gnode = tr_ring_get(ring, tr_bottom_slot<W>(fs.trail, fs.owned, j));
                    gdepth = (int32_t)(j + 1);
                    list[drank] = lane; xnode[lane] = gnode; xdepth[lane] = gdepth;
                    fs.trail &= ~(W(1) << j);
                }
                __builtin_amdgcn_wave_barrier();
                const bool take = done && irank < np;
                const int src = take ? list[irank] : lane;
                // a lane that takes new work first hands in what it has found so far
                if (take) {
                    deposit();
                    tr_result_init(res);
                }
                // the ray (and its owner / current bound) moves with the subtree
                r.ox = __shfl(r.ox, src); r.oy = __shfl(r.oy, src); r.oz = __shfl(r.oz, src);
                r.dx = __shfl(r.dx, src); r.dy = __shfl(r.dy, src); r.dz = __shfl(r.dz, src);
                r.ix = __shfl(r.ix, src); r.iy = __shfl(r.iy, src); r.iz = __shfl(r.iz, src);
                r.kd = __shfl(r.kd, src);
                r.sel_n = (uint32_t)__shfl((int)r.sel_n, src); r.sel_f = (uint32_t)__shfl((int)r.sel_f, src); r.sel_z = (uint32_t)__shfl((int)r.sel_z, src);
                if constexpr (QN) {      // the fused box-test constants of the grid nodes (tr_ray_fuse)
                    r.qax = __shfl(r.qax, src); r.qay = __shfl(r.qay, src); r.qaz = __shfl(r.qaz, src);
                    r.qnx = __shfl(r.qnx, src); r.qny = __shfl(r.qny, src); r.qnz = __shfl(r.qnz, src);
                    r.qfx = __shfl(r.qfx, src); r.qfy = __shfl(r.qfy, src); r.qfz = __shfl(r.qfz, src);
                    r.qaz2 = r.qaz;
                }
                const int own2 = __shfl(owner, src);
                const float bt = __shfl(res.best_t, src);
                if (take) {
                    owner = own2;
                    if constexpr (PLAIN) {
                        tr_state_init(fs, tr_addr_bottom(ar, fs.sa));      // an empty stack again: the lane's slot 0 ...
                        atomicAnd(&xflags[lane], 0x100);                   // ... and nothing given away
                    } else {
                        tr_state_init(fs);
                        fs.depth = (uint32_t)xdepth[src];
                    }
                    fs.node = xnode[src];
                    tr_set_best_t(res, bt);
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (split) {
        // everybody hands in what it still holds; every owner lane reads its ray's total
        deposit();
        __builtin_amdgcn_wave_barrier();
        if (Q == TR_Q_COUNT) {
            res.count = vsum[lane];
        } else if (Q == TR_Q_ANY) {
            res.best_face = vsum[lane] ? 0 : -1;
        } else {
            const unsigned long long k = vkeys[lane];
            tr_result_init(res);
            if (k != ~0ull) {
                tr_set_best_t(res, __uint_as_float((unsigned)(k >> 32)));
                res.best_face = (int32_t)(unsigned)k;
                res.best_slot = vslots[lane];
            }
        }
        if constexpr (PLAIN) lost = (xdepth[lane] & 0x100) != 0;
    } else if constexpr (PLAIN) {
        lost = tr_addr_lost(fs.sa);
    }
    return split;
}

// All 64 lanes of a wave call this together (`in_range` = the lane owns ray i).
template <int Q, bool STATS, bool COMPACT = false, bool UNI = false, bool DEEP = false>
__device__ __forceinline__ void process_ray(const tr_bvh_view& b, const RayFetch& rf,
                                            const QueryOut& out, int64_t i, bool in_range,
                                            tr_counters* cnt, const tr_ring ring) {
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (in_range) fetch_ray(rf, i, o, d);
    tr_ray r;
    const bool valid = tr_ray_setup_a(r, b.frame, o[0], o[1], o[2], d[0], d[1], d[2]) && in_range;
    tr_result res;
    if (Q == TR_Q_LOCATION) {
        // fused multi-hit: uncapped count + the ray's `cap` nearest hits as unsorted entries
        tr_topk<0> top;
        top.ent = out.hits + (in_range ? i : 0) * out.cap;
        top.tris = b.tris;
        top.cap = out.cap;
        if (b.num_tris >= 2) {
            wave_traverse<Q, 0, STATS, COMPACT, UNI, DEEP>(b, r, valid, res, top, cnt, ring);
        } else {
            top.init();
            brute_one<Q>(b, r, valid, res);
            if (res.count) top.insert(res.best_t, res.best_face, 0);
        }
    } else {
        tr_topk<1> top;
        if (b.num_tris >= 2) wave_traverse<Q, 1, STATS, COMPACT, UNI, DEEP>(b, r, valid, res, top, cnt, ring);
        else brute_one<Q>(b, r, valid, res);
    }
    if (in_range) write_result<Q>(b, out, i, r, res);
}

// The rays of a wave whose plain far-child stack lost a child (tr_addr_push; on the lane that owns the ray or on a thief):
// traversed once more, from the best hit so far, by the stackless walk over the exact nodes (tr_traverse_more).  A real call
// behind a branch marked as unlikely, like the float64 part of the hit predicate (tr_drain_exact<COLD>): what it needs is
// saved around the call and it puts nothing into the trips.  Everything arrives by value -- a pointer to the caller's view or
// ray would pin those to scratch for the whole kernel.
template <int Q>
__device__ __attribute__((noinline)) tr_result retraverse_lost(const tr_node* nodes, const tr_link* links, const tr_tri* tris,
                                                               float b0, float b1, float b2, float s0, float s1, float s2,
                                                               float ox, float oy, float oz, float dx, float dy, float dz,
                                                               float best_t, int32_t best_face, int32_t best_slot) {
    tr_bvh_view v;
    v.nodes = nodes; v.links = links; v.tris = tris; v.num_tris = 2; v.qnodes = nullptr; v.frame_dev = nullptr;
    v.frame.base[0] = b0; v.frame.base[1] = b1; v.frame.base[2] = b2;
    v.frame.scale[0] = s0; v.frame.scale[1] = s1; v.frame.scale[2] = s2;
    tr_result res;
    res.best_t = best_t; res.best_face = best_face; res.best_slot = best_slot; res.count = 0;
    tr_ray r;
    if (tr_ray_setup_a(r, v.frame, ox, oy, oz, dx, dy, dz)) {
        tr_topk<1> top;
        tr_counters* nc = nullptr;
        tr_traverse_more<Q, 1, false>(v, r, res, top, nc);
    }
    return res;
}

template <int Q, bool STATS, bool COMPACT, bool DEEP = false, bool QN = false>
__device__ __forceinline__ void process_ray_steal(const tr_bvh_view& b, const RayFetch& rf,
                                                  const QueryOut& out, int64_t i, bool in_range,
                                                  tr_counters* cnt, const tr_ring ring, int32_t* wl,
                                                  uint32_t steal_min) {
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (in_range) fetch_ray(rf, i, o, d);
    tr_ray r;
    const bool valid = tr_ray_setup_q(r, b.frame, o[0], o[1], o[2], d[0], d[1], d[2]) && in_range;
    tr_result res;
    bool split = false, lost = false;
    if (b.num_tris >= 2) split = wave_traverse_steal<Q, STATS, COMPACT, DEEP, QN>(b, r, valid, res, cnt, ring, wl, (int)(threadIdx.x & 63), steal_min, lost);
    else brute_one<Q>(b, r, valid, res);   // no hierarchy below two triangles
    if (split && in_range) {   // this lane may hold another lane's ray now: take its own again
        fetch_ray(rf, i, o, d);
        tr_ray_setup_a(r, b.frame, o[0], o[1], o[2], d[0], d[1], d[2]);
    }
    if constexpr (QN) {
        lost = lost && valid;
        if (__builtin_expect(TR_WAVE_ANY(lost), 0)) {
            if (lost) {
                // (the ray is fetched again: kept from the prologue it would cost the trips six registers)
                fetch_ray(rf, i, o, d);
                res = retraverse_lost<Q>(b.nodes, b.links, b.tris, b.frame.base[0], b.frame.base[1], b.frame.base[2],
                                         b.frame.scale[0], b.frame.scale[1], b.frame.scale[2], o[0], o[1], o[2], d[0], d[1], d[2],
                                         res.best_t, res.best_face, res.best_slot);
            }
        }
    }
    if (in_range) write_result<Q>(b, out, i, r, res);
}

// ---- unordered two-phase schedule (tr_unord_step): any / count / location --------------------
// Wave-level vote per trip: the leaf phase (three triangle loads + the full predicate) runs only
// when a lane's queue is nearly full ("parked": it could not take both children of its node),
// when at least `leaf_min` lanes have something queued, or when no lane has a node left.
template <int Q, int K, bool STATS, bool COMPACT, bool DEEP = false>
__device__ __forceinline__ void wave_traverse_unordered(const tr_bvh_view& b, tr_ray& r, bool go,
                                                        tr_result& res, tr_topk<K>& top, tr_counters* cnt,
                                                        const tr_ring ring, const tr_leafq lq, int leaf_min) {
    typedef typename tr_word<COMPACT, DEEP>::T W;
    tr_result_init(res);
    if (Q == TR_Q_LOCATION) top.init();
    tr_ustate_t<W> st;
    tr_ustate_init(st);
    if (!go) st.node = -1;
    for (;;) {
        const bool can_node = tr_ucan_node(st);
        const unsigned long long mn = __ballot(can_node), ml = __ballot(st.nq > 0);
        if ((mn | ml) == 0ull) break;
        const bool parked = st.node >= 0 && !can_node;
        const bool leaf_phase = mn == 0ull || __ballot(parked) != 0ull || (int)__popcll(ml) >= (int)leaf_min;
        tr_unord_step<Q, K, STATS, COMPACT, W>(b, r, can_node, leaf_phase, st, res, top, cnt, ring, lq);
        TR_CONVERGE();
    }
}

// ---- the unordered schedule with work stealing (count) --------------------------------------------
// A count launch has no culling, but on a silhouette image the grazing rays are outliers here too
// (headline image: bulk done at 377 us of 556), and a launch that leaves wave slots of the chip empty
// ends with its longest waves.  Both are answered by SPLIT launch slots (k_sched_sort): a slot owns
// every 2nd / 4th ray of a block and its other lanes take owed subtrees of those rays from the first
// trips on: headline count 0.545 -> 0.383 ms, C4 at 262 k rays 0.436 -> 0.348, the interior scene at
// 230 k rays 0.254 -> 0.164 (profiles/r03_sweep_usteal.jsonl).  A launch of several rounds of EQUALLY
// long waves (C4 at 1 M rays) gains nothing, also not from splitting the blocks of its last round
// (tried: the ramp-down is half a wave's time whatever the last waves are, and split waves are not
// 2-4x shorter; r03_sweep_usteal_uniform.jsonl).  The multi-hit list query stays on the plain unordered
// schedule: a list that several lanes append to needs its fill count in one place and its overflow
// path (a ray with more than `cap` hits replaces its farthest entry) serialised -- built and measured:
// headline location -25 %, but C4 +5 % and the interior scene, where rays have up to 13 hits, 5x SLOWER
// (profiles/r03_location_steal_experiment.jsonl).  Hand-over as in wave_traverse_steal, with two differences: (1) no LDS scratch --
// the kernel sits exactly at the LDS budget of 7 waves per SIMD (ring + leaf queue), so donor lanes
// are listed with ds_permute / ds_bpermute and counts are handed in through v_readlane loops; (2) the
// merge is a sum, order-free.  Any partition of a tree among lanes visits the same leaves, so the
// counts are bit-identical (tests force thresholds 0 ... 64 on every scene family).
template <int Q, bool STATS, bool COMPACT, bool DEEP = false>
__device__ __forceinline__ int wave_count_unordered_steal(const tr_bvh_view& b, tr_ray& r, bool go, tr_counters* cnt,
                                                          const tr_ring ring, const tr_leafq lq, int leaf_min,
                                                          int lane, uint32_t steal_min) {
    typedef typename tr_word<COMPACT, DEEP>::T W;
    tr_result res;
    tr_result_init(res);
    tr_topk<1> top;
    tr_ustate_t<W> st;
    tr_ustate_init(st);
    if (!go) st.node = -1;
    int owner = lane;      // lane whose ray this lane is working on
    int acc = 0;           // hits of THIS lane's ray that have been handed in (by itself or by others)
    uint32_t trip = 0;
    // lanes with `want` hand the count they hold to the owner of the ray they worked on
    auto hand_in = [&](bool want) {
        unsigned long long m = __ballot(want && res.count != 0);
        while (m != 0ull) {
            const int t = (int)__builtin_ctzll(m);
            const int o = __builtin_amdgcn_readlane(owner, t), c = __builtin_amdgcn_readlane(res.count, t);
            if (lane == o) acc += c;
            m &= m - 1ull;
        }
        if (want) res.count = 0;
    };
    for (;;) {
        bool live = true;      // wave-uniform: some lane still has a node or a queued leaf
#pragma unroll 1
        for (int k = 0; k < 4 && live; k++) {
            const bool can_node = tr_ucan_node(st);
            const unsigned long long mn = __ballot(can_node), ml = __ballot(st.nq > 0);
            live = (mn | ml) != 0ull;
            if (live) {
                const bool parked = st.node >= 0 && !can_node;
                const bool leaf_phase = mn == 0ull || __ballot(parked) != 0ull || (int)__popcll(ml) >= (int)leaf_min;
                tr_unord_step<Q, 1, STATS, COMPACT, W>(b, r, can_node, leaf_phase, st, res, top, cnt, ring, lq);
            }
            TR_CONVERGE();
        }
        trip += 4;
        const bool done = tr_udone(st);
        const unsigned long long idle = __ballot(done);
        if (idle == ~0ull) break;
        if (idle == 0ull) continue;
        const W cand = st.trail & st.owned;          // owed far children that are in the stack
        const bool can_give = !done && cand != 0 && trip >= steal_min;
        const unsigned long long donors = __ballot(can_give);
        const int ni = __popcll(idle), nd = __popcll(donors);
        const int np = ni < nd ? ni : nd;
        if (np == 0) continue;
        const int drank = lane_rank(donors), irank = lane_rank(idle);
        const bool give = can_give && drank < np;
        const bool take = done && irank < np;
        // compact list of the giving lanes without LDS: giver g sends its lane id to lane g (the other
        // lanes send theirs to distinct lanes from the top, so that every lane is written exactly once)
        const unsigned long long givers = __ballot(give);
        const int tgt = give ? drank : 63 - lane_rank(~givers);
        const int list = __builtin_amdgcn_ds_permute(tgt << 2, lane);
        // (the read-back is executed by EVERY lane: ds_bpermute returns 0 for a source lane that is
        // masked off, and list entry g lives in lane g, which need not be a taker itself)
        const int pick = __shfl(list, irank & 63);
        const int src = take ? pick : lane;
        int gnode = 0, gdepth = 0;
        if (give) {
            const uint32_t j = (uint32_t)__builtin_ctzll((unsigned long long)cand);     // the shallowest: the biggest subtree
            gnode = tr_ring_get(ring, j & (TR_RING - 1));      // (this schedule's ring is indexed by depth: tr_unord_step)
            gdepth = (int)(j + 1);
            st.trail &= ~(W(1) << j);
            st.owned &= ~(W(1) << j);
        }
        // a lane that takes new work first hands in what it counted for the ray it is leaving
        if (take && owner == lane) { acc += res.count; res.count = 0; }
        hand_in(take && owner != lane);
        r.ox = __shfl(r.ox, src); r.oy = __shfl(r.oy, src); r.oz = __shfl(r.oz, src);
        r.dx = __shfl(r.dx, src); r.dy = __shfl(r.dy, src); r.dz = __shfl(r.dz, src);
        r.ix = __shfl(r.ix, src); r.iy = __shfl(r.iy, src); r.iz = __shfl(r.iz, src);
        r.kd = __shfl(r.kd, src);
        r.sel_n = (uint32_t)__shfl((int)r.sel_n, src); r.sel_f = (uint32_t)__shfl((int)r.sel_f, src); r.sel_z = (uint32_t)__shfl((int)r.sel_z, src);
        r.qax = __shfl(r.qax, src); r.qay = __shfl(r.qay, src); r.qaz = __shfl(r.qaz, src);      // (tr_ray_fuse)
        r.qnx = __shfl(r.qnx, src); r.qny = __shfl(r.qny, src); r.qnz = __shfl(r.qnz, src);
        r.qfx = __shfl(r.qfx, src); r.qfy = __shfl(r.qfy, src); r.qfz = __shfl(r.qfz, src);
        r.qaz2 = r.qaz;
        const int own2 = __shfl(owner, src), n2 = __shfl(gnode, src), d2 = __shfl(gdepth, src);
        if (take) {
            owner = own2;
            tr_ustate_init(st);
            st.node = n2;
            st.depth = (uint32_t)d2;
        }
        TR_CONVERGE();
    }
    if (owner == lane) { acc += res.count; res.count = 0; }
    hand_in(owner != lane);
    return acc;
}

template <int Q, bool STATS, bool COMPACT, bool DEEP = false, bool USTEAL = false>
__device__ __forceinline__ void process_ray_unordered(const tr_bvh_view& b, const RayFetch& rf,
                                                      const QueryOut& out, int64_t i, bool in_range,
                                                      tr_counters* cnt, const tr_ring ring,
                                                      const tr_leafq lq, int leaf_min, uint32_t steal_min = 0) {
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (in_range) fetch_ray(rf, i, o, d);
    tr_ray r;
    const bool valid = tr_ray_setup_q(r, b.frame, o[0], o[1], o[2], d[0], d[1], d[2]) && in_range;
    tr_result res;
    if (b.num_tris < 2) {
        // no hierarchy below two triangles (wave-uniform): the predicate on the one triangle there may be
        brute_one<Q>(b, r, valid, res);
        if (Q == TR_Q_LOCATION) {
            tr_topk<0> top;
            top.ent = out.hits + (in_range ? i : 0) * out.cap;
            top.tris = b.tris;
            top.cap = out.cap;
            top.init();
            if (res.count) top.insert(res.best_t, res.best_face, 0);
        }
    } else if (Q == TR_Q_LOCATION) {
        tr_topk<0> top;
        top.ent = out.hits + (in_range ? i : 0) * out.cap;
        top.tris = b.tris;
        top.cap = out.cap;
        wave_traverse_unordered<Q, 0, STATS, COMPACT, DEEP>(b, r, valid, res, top, cnt, ring, lq, leaf_min);
    } else if (USTEAL && Q == TR_Q_COUNT) {
        tr_result_init(res);
        res.count = wave_count_unordered_steal<Q, STATS, COMPACT, DEEP>(b, r, valid, cnt, ring, lq, leaf_min,
                                                                       (int)(threadIdx.x & 63), steal_min);
    } else {
        tr_topk<1> top;
        wave_traverse_unordered<Q, 1, STATS, COMPACT, DEEP>(b, r, valid, res, top, cnt, ring, lq, leaf_min);
    }
    if (in_range) write_result<Q>(b, out, i, r, res);
}

#include "traverse_wide.inc"

// Order the blocks of the last launch by measured cost, most expensive first: one workgroup,
// counting sort on the cost quantised to 256 levels (max-reduce, LDS histogram, scan, scatter;
// the order inside a level is arbitrary -- any permutation is a correct launch order).
// Resets the cost array for the next measurement.
// NT threads (a multiple of 64); bins = 8 x 256 words of LDS, misc = 16 more (8-byte aligned).  Two callers: k_sched_sort
// (1024 threads, behind a measuring launch) and the sorter workgroup of a query launch (128 threads, on the LDS the
// traversal would use: query_direct_body, tr_sort_job).
struct tr_sort_job {          // a deferred sort that rides in a query launch (cost == NULL: none)
    uint32_t* cost;           // block costs of the last measuring launch (zeroed by the sort)
    uint32_t* order;          // the order buffer it writes -- NOT the one the carrying launch reads
    uint32_t* prev;           // copy of the costs it sorted (k_sched_rescale)
    int nblocks, xcd_map, split, split4, outlier8, floor_ticks;
};
template <int NT>
__device__ __forceinline__ void sched_sort_body(uint32_t* __restrict__ cost, uint32_t* __restrict__ order, int nblocks,
                                                int xcd_map, int split, int split4, int outlier8, int floor_ticks,
                                                uint32_t* __restrict__ prev, uint32_t (*bins)[256], uint32_t* misc) {
    // list x: blocks whose home in the XCD-chunked map is XCD x (see k_query_direct; the blocks
    // past the last whole span are dealt round-robin there, so their home is i % 8).  Launch
    // slot j*8+x runs on XCD x, so list x fills the slots of XCD x in cost order: expensive
    // blocks first AND every block stays on the XCD (L2) that its neighbours in the image use.
    // |list x| = number of slots of XCD x because the whole spans are multiples of 8 blocks.
    unsigned long long& ssum = *reinterpret_cast<unsigned long long*>(misc);   // misc[0..1]
    uint32_t& smax = misc[2];
    uint32_t* nsplit = misc + 4;         // [8] blocks of list x that are really split (<= split)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < 8 * 256; k += NT) (&bins[0][0])[k] = 0;
    if (tid == 0) { smax = 1; ssum = 0ull; }
    __syncthreads();
    const int T = xcd_map;
    const int nfull = T > 0 ? nblocks / (8 * T) * (8 * T) : 0;
    uint32_t m = 0;
    unsigned long long sum = 0;
    for (int i = tid; i < nblocks; i += NT) { const uint32_t c = cost[i]; m = c > m ? c : m; sum += c; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(m, off); m = o > m ? o : m;
        sum += __shfl_xor(sum, off);
    }
    if (lane == 0) { atomicMax(&smax, m); atomicAdd(&ssum, sum); }
    __syncthreads();
    // any monotone quantisation will do: level 0 = most expensive (costs are < 2^19 ticks)
    const float scale = 255.0f / (float)smax;
    for (int i = tid; i < nblocks; i += NT) {
        const uint32_t q = 255u - min(255u, (uint32_t)((float)cost[i] * scale));
        const int x = i < nfull ? (i / T) & 7 : i & 7;
        atomicAdd(&bins[x][q], 1u);
    }
    __syncthreads();
    // Which blocks are WORTH splitting is decided here, from the costs: a block gets extra launch slots
    // only if it sticks out -- at least outlier8 / 8 times the mean block cost -- and is long enough for
    // hand-overs to pay (floor_ticks: waves of a few dozen trips end before a thief has done anything).
    // The grid has room for `split` blocks per XCD; what is not used stays empty (sentinel entries).
    // An interior scene with evenly expensive rays splits nothing (0.050 -> 0.036 ms at 230 k rays), a
    // silhouette image splits its silhouette (profiles/r03_policy_matrix.jsonl, r03_sweep_outlier.jsonl).
    uint32_t thr = 0;
    if (outlier8 > 0) {
        const float mean = (float)ssum / (float)nblocks;
        const float t = fmaxf(mean * (float)outlier8 * 0.125f, (float)floor_ticks);
        thr = t >= 4.0e9f ? 0xffffffffu : (uint32_t)t;
    }
    // (the level of the threshold: blocks of a level are kept or dropped together)
    const uint32_t thr_level = thr > smax ? 0u : 255u - min(255u, (uint32_t)((float)thr * scale));
    for (int x = wave; x < 8; x += NT / 64) {   // exclusive scan of list x by one wave: 4 bins per lane
        uint32_t v[4], sum4 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { v[k] = bins[x][4 * lane + k]; sum4 += v[k]; }
        uint32_t inc = sum4;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off); if (lane >= off) inc += o; }
        uint32_t run = inc - sum4;
        // blocks at levels < thr_level (strictly more expensive than the threshold's level) qualify
        uint32_t above = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            bins[x][4 * lane + k] = run;
            if ((uint32_t)(4 * lane + k) == thr_level) above = run;
            run += v[k];
        }
        // exactly one lane holds the prefix count at thr_level
        const unsigned long long who = __ballot((uint32_t)(4 * lane) <= thr_level && thr_level < (uint32_t)(4 * lane + 4));
        const uint32_t cnt = __shfl(above, (int)__builtin_ctzll(who));
        if (lane == 0) nsplit[x] = thr > smax ? 0u : min((uint32_t)split, outlier8 > 0 ? cnt : (uint32_t)split);
    }
    __syncthreads();
    // unused extra slots of every XCD: sentinel entries (the query kernel returns at once)
    {
        const uint32_t spmax = (uint32_t)split, q4max = (uint32_t)split4;
        const uint32_t extra_max = spmax + 2u * q4max;
        for (uint32_t k = tid; k < 8u * extra_max; k += (uint32_t)NT) {
            const uint32_t x = k & 7u, e = k >> 3;
            const uint32_t sp = nsplit[x], q4 = sp >> 2;
            const uint32_t len = (uint32_t)((nblocks >> 3) + (((uint32_t)nblocks & 7u) > x ? 1 : 0));
            if (e >= sp + 2u * q4) order[(len + e) * 8u + x] = 0x07ffffffu;
        }
    }
    for (int i = tid; i < nblocks; i += NT) {
        const uint32_t q = 255u - min(255u, (uint32_t)((float)cost[i] * scale));
        const int x = i < nfull ? (i / T) & 7 : i & 7;
        const uint32_t j = atomicAdd(&bins[x][q], 1u);
        // block splitting: the `sp` most expensive blocks of XCD x get two launch slots
        // each (halves of their rays, see k_query_direct); the launch has 8 * split slots more
        // (the first quarter of them four: quarters of their rays)
        const uint32_t sp = nsplit[x], q4 = sp >> 2;
        if (j < q4) {
            for (uint32_t k = 0; k < 4u; k++)
                order[(4u * j + k) * 8u + (uint32_t)x] = (uint32_t)i | (2u << 30) | (k << 28);
        } else if (j < sp) {
            const uint32_t p = 4u * q4 + 2u * (j - q4);
            order[p * 8u + (uint32_t)x] = (uint32_t)i | (1u << 30);
            order[(p + 1u) * 8u + (uint32_t)x] = (uint32_t)i | (1u << 30) | (1u << 28);
        } else {
            order[(j + sp + 2u * q4) * 8u + (uint32_t)x] = (uint32_t)i;
        }
        if (prev) prev[i] = cost[i];      // kept for k_sched_rescale: the next batch SHAPE starts from these
        cost[i] = 0u;
    }
    if (tid == 0) { order[TR_SCHED_MAX] = (uint32_t)nblocks; order[TR_SCHED_MAX + 1] = (uint32_t)split; }
}

// MODE: 0 fused ordered trip, 1 fused trip + intra-wave work stealing, 2 unordered two-phase
// schedule (any / count / location on hierarchies of at least two triangles)
template <int Q, bool STATS, bool COMPACT, int BS, int MODE, bool DEEP, bool QN, bool JOB = false>
__device__ __forceinline__ void query_direct_body(const tr_bvh_view& b, const RayFetch& rf, const QueryOut& out,
                                                  int xcd_map, int scramble, int tile_w, int steal_min,
                                                  const uint32_t* __restrict__ order, int order_split,
                                                  uint32_t* __restrict__ cost,
                                                  unsigned long long* stats,
                                                  const int* __restrict__ sel,
                                                  const tr_wide_args& wa = tr_wide_args{nullptr, nullptr, 0, 0},
                                                  const tr_sort_job& job = tr_sort_job{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0}) {
    // dual launch (k_probe_coherence): this launch shape is the one for coherent batches (id 0)
    if (sel && *sel != 0) return;
    // launch slot of this workgroup and slots of the launch (a launch that carries a sort -- JOB -- has eight slots more in
    // front; the other instantiations compile to what they were without it)
    const unsigned slot_shift = JOB ? 8u : 0u;
    const unsigned bid = blockIdx.x - slot_shift;
    int64_t nblk = gridDim.x - slot_shift;
    const unsigned long long t_start = cost ? wall_clock64() : 0ull;
    __shared__ int32_t ring_lds[MODE == 4 ? 1 : TR_RING * BS];
    const tr_ring ring = {ring_lds + threadIdx.x, BS, ring_lds};
    constexpr int SCR = 384;          // ints of stealing scratch per wave (MODE 1)
    __shared__ alignas(8) int32_t steal_lds[MODE == 1 ? (BS / 64) * SCR : (JOB ? 16 : 2)];
    if constexpr (JOB) {
        static_assert((MODE == 1 || MODE == 3) && BS == 128, "the sorter rides in the launches that steal");
        // The sort of the previous measuring launch's block costs, deferred into THIS launch (tr_sort_job, sched_acquire):
        // workgroup 0 sorts them into the order buffer the NEXT launches read -- 10-20 us of one workgroup in the shadow of
        // a launch instead of a serial 11.5-us k_sched_sort behind every fourth one (r05m: step = kernel + sort / 4) --,
        // workgroups 1-7 leave so that launch slot s still runs on XCD s % 8 (the orders are per-XCD lists).
        if (blockIdx.x < 8) {
            static_assert(sizeof(ring_lds) >= 8 * 256 * 4 && sizeof(steal_lds) >= 16 * 4, "the sorter works on the traversal's LDS");
            if (blockIdx.x == 0 && job.cost)
                sched_sort_body<BS>(job.cost, job.order, job.nblocks, job.xcd_map, job.split, job.split4, job.outlier8,
                                    job.floor_ticks, job.prev, reinterpret_cast<uint32_t(*)[256]>(ring_lds),
                                    reinterpret_cast<uint32_t*>(steal_lds));
            return;
        }
    }
    // XCD-aware block -> ray-tile map: workgroups are dealt round-robin over the 8 XCDs
    // (blocks b and b+8 share one).  The ray range is cut into chunks of `xcd_map` blocks and
    // chunk c goes to XCD c % 8, so each XCD's private L2 works on compact pieces of the image
    // (and of the BVH) while expensive regions are still spread over all XCDs.  Placement only
    // affects speed.
    int64_t blk = bid;
    int part = 0, parts_lg = 0;           // block splitting (k_sched_sort): this launch slot's share
    // (nblk: ray blocks of the launch -- the grid may have extra slots)
    if (order) {
        // The order buffer belongs to the (handle, stream) and is rewritten by the sort behind every
        // measuring launch: a launch replayed from a HIP graph -- or any launch, after such a replay
        // -- may find an order that was written for ANOTHER grid.  The sort stamps what it wrote
        // (block count, split blocks per XCD) behind the array; anything else is ignored and this
        // launch runs in the static order (its extra slots have nothing to do).
        nblk -= 8 * ((int64_t)order_split + 2 * (order_split >> 2));
        const uint32_t* hdr = order + TR_SCHED_MAX;
        if (hdr[0] != (uint32_t)nblk || hdr[1] != (uint32_t)order_split) {
            order = nullptr;
            if ((int64_t)bid >= nblk) return;
        }
    }
    if (order) {
        // measured order: most expensive blocks first.  Bits 30-31 of an entry = lg of the number of
        // launch slots the block's rays were dealt to, bits 28-29 = this slot's part.
        const uint32_t e = order[bid];
        blk = e & 0x07ffffffu;
        if (blk >= nblk) return;          // a launch slot the sort left unused (fewer blocks split than the grid allows)
        parts_lg = (int)(e >> 30);
        part = (int)((e >> 28) & 3u);
        if (MODE != 1 && MODE != 3) {     // (split orders are only written for the shapes that steal)
            if (part) return;
            parts_lg = 0;
        }
    } else if (xcd_map > 0) {
        const int64_t T = xcd_map, span = 8 * T;
        const int64_t nfull = nblk / span * span;                 // blocks covered by whole spans
        if (blk < nfull) {
            const int64_t x = blk & 7;                            // XCD label
            int64_t k = blk >> 3;                                 // index within the XCD
            // no measured order yet: visit the XCD's blocks in a scrambled order (k -> k*P mod
            // count, P prime) so that an expensive image region is spread over the whole
            // launch instead of being started last
            if (scramble > 1) k = (k * scramble) % (nfull >> 3);
            blk = ((k / T) * 8 + x) * T + (k % T);
        }
    }
    int64_t i = blk * BS + threadIdx.x;
    if (tile_w > 0) {
        // image-shaped batch: a wave takes a tile of 2^lgh rows x 2^(6-lgh) pixels (8x8, 4x16 or
        // 2x32; lgh in bits 28-29 of the argument) instead of 64 pixels of one row
        const int lgh = (tile_w >> 28) & 3, lgw = 6 - lgh;
        const int64_t width = tile_w & 0x0fffffff;
        // the tile index and its row / column are the same for the whole wave: scalar arithmetic in 32 bits (a launch has
        // fewer than 2^31 blocks of two tiles; the width is below 2^28), not a 64-bit division per lane
        static_assert(BS % 64 == 0, "a wave is one tile");
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const uint32_t tile = (uint32_t)blk * (uint32_t)(BS / 64) + wave, tpr = (uint32_t)(width >> lgw);
        const int lane = (int)(threadIdx.x & 63);
        const uint32_t ty = tile / tpr, tx = tile - ty * tpr;
        i = (((int64_t)ty << lgh) + (lane >> lgw)) * width + ((int64_t)tx << lgw) + (lane & ((1 << lgw) - 1));
    }
    tr_counters cnt = {0, 0, 0};
    if (MODE == 4) {
        // 8-wide compressed nodes, one ray per lane (wave_traverse_wide): count / location / closest / first / any
        __shared__ int32_t wstack_lds[(TR_WNODES + TR_WLEAVES) * BS];
        const bool in_range = i < rf.n;
        float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
        if (in_range) fetch_ray(rf, i, o, d);
        tr_ray r;
        const bool valid = tr_ray_setup_q(r, b.frame, o[0], o[1], o[2], d[0], d[1], d[2]) && in_range;
        tr_result res;
        if constexpr (Q == TR_Q_LOCATION) {
            tr_topk<0> top;
            top.ent = out.hits + (in_range ? i : 0) * out.cap;
            top.tris = b.tris;
            top.cap = out.cap;
            wave_traverse_wide<Q, 0, STATS, BS>(b, wa, r, valid, res, top, cnt, wstack_lds);
        } else {
            tr_topk<1> top;
            wave_traverse_wide<Q, 1, STATS, BS>(b, wa, r, valid, res, top, cnt, wstack_lds);
        }
        if (in_range) write_result<Q>(b, out, i, r, res);
    } else if (MODE == 2) {
        // the steal_min argument carries the leaf-phase vote threshold of this schedule
        __shared__ int32_t leafq_lds[TR_LEAFQ * BS];
        const tr_leafq lq = {leafq_lds + threadIdx.x, BS};
        process_ray_unordered<Q, STATS, COMPACT, DEEP>(b, rf, out, i, i < rf.n, &cnt, ring, lq, steal_min);
    } else if (MODE == 3) {
        // unordered schedule + stealing: leaf vote (bits 0-7) | trip from which a ray gives subtrees away
        // (bits 8-19) | the same for split blocks (bits 20-31)
        __shared__ int32_t leafq_lds[TR_LEAFQ * BS];
        const tr_leafq lq = {leafq_lds + threadIdx.x, BS};
        const bool mine = (((int)threadIdx.x ^ part) & ((1 << parts_lg) - 1)) == 0;
        const uint32_t smin = parts_lg ? ((uint32_t)steal_min >> 20) & 0xfffu : ((uint32_t)steal_min >> 8) & 0xfffu;
        process_ray_unordered<Q, STATS, COMPACT, DEEP, true>(b, rf, out, i, i < rf.n && mine, &cnt, ring, lq,
                                                            steal_min & 0xff, smin);
    } else if (MODE == 1) {
        // A split block (one of the most expensive of the previous launch): this slot owns the rays
        // of every 2^parts_lg-th lane; the other lanes start idle and take subtrees of those rays
        // from the trip in the upper half of the argument on (the lower half: everybody else)
        const bool mine = (((int)threadIdx.x ^ part) & ((1 << parts_lg) - 1)) == 0;
        const uint32_t smin = parts_lg ? (uint32_t)steal_min >> 16 : (uint32_t)steal_min & 0xffffu;      // (bit 15: adaptive, wave_traverse_steal)
        process_ray_steal<Q, STATS, COMPACT, DEEP, QN>(b, rf, out, i, i < rf.n && mine, &cnt, ring,
                                                       steal_lds + (threadIdx.x >> 6) * SCR, smin);
    } else {
        // the plain shape is what large coherent batches get (small ones steal, incoherent ones
        // stream): look for wave-uniform trips (tr_fused_step)
        process_ray<Q, STATS, COMPACT, !STATS && BS == 128 && Q != TR_Q_LOCATION, DEEP>(b, rf, out, i, i < rf.n, &cnt, ring);
    }
    if (cost && (threadIdx.x & 63) == 0) {
        // 100 MHz ticks.  A split block records twice what it would have cost in one piece (roughly):
        // it has to stay among the expensive ones, or the split set alternates between two groups of
        // blocks from one measurement to the next (and every other group of launches has a long tail)
        constexpr int TR_SPLIT_STICKY = 1;     // extra doubling of a split block's recorded cost (0: recorded as parts x its slots' time: r05_ab_split_sticky.txt)
        const unsigned long long dt = (wall_clock64() - t_start) << (parts_lg ? parts_lg + TR_SPLIT_STICKY : 0);
        atomicMax(&cost[blk], (uint32_t)(dt > 0x7ffffull ? 0x7ffffull : dt));
    }
    flush_stats<STATS>(cnt, stats);
}

// MODE: 0 fused ordered trip, 1 fused trip + intra-wave work stealing, 2 unordered two-phase schedule,
// 3 unordered + stealing (query_direct_body)
// Round 6: six waves per SIMD asked for (80 registers).  With the float64 call at the end of a trip (tr_drain_exact) the
// compiler's own budget puts the stealing closest kernel at 83-88 (five waves); held to 80 -- and with the drain's branch
// marked as cold -- it saves four to six registers around the call and touches scratch nowhere else
// (tests/test_round4_cpu.py reads that off the shipped ISA; before the hint six kernel-lifetime values sat in scratch:
// 48 MB of traffic per launch and 2 % of the headline, profiles/r06_ab_cold_drain.txt).  0 = the compiler's budget.
#ifndef TR_DIRECT_WAVES
#define TR_DIRECT_WAVES 6
#endif
// The instantiations with 64-bit trail words (DEEP: hierarchies of more than 32 levels) are the ones in which forced spills
// have faulted: with KERNEL-LIFETIME values in scratch -- stored in the prologue, reloaded in the hand-over code of the
// stealing loop and behind it -- they die with a memory access fault on the 21 M-triangle mesh of the test suite (round 5:
// k_query_count_steal<true, true> at seven waves, profiles/r05_count_waves_fault.txt; round 6: k_query_direct<2, false,
// true, 1, true, true> at six, profiles/r06_deep_spill_fault.txt) while every 32-bit instantiation with the same kind of
// spills passes the whole suite.  Since the drain of parked leaf tests is a cold branch (tr_drain_exact<COLD>) the only
// scratch traffic of these kernels is the save / restore AROUND the float64 call, and in that form the DEEP kernels run the
// same mesh and the whole suite clean at six waves (5.2 M triangles, 34 levels: closest 0.280 -> 0.259 ms, first -7 %,
// any -5 %: profiles/r06_deep_six_waves.txt).  The mechanism of the fault itself is still open (DESIGN.md section 9);
// tests/test_round4_cpu.py pins the DEEP kernels to "no scratch instruction outside the call's neighbourhood".
#if TR_DIRECT_WAVES > 0
#ifndef TR_DEEP_WAVES
#define TR_DEEP_WAVES TR_DIRECT_WAVES
#endif
// (DEEP on the exact 64-byte nodes -- option grid_nodes = 0 -- would keep one kernel-lifetime value in scratch at six waves: the
// pattern that faulted; it stays at the compiler's budget)
// ... and so do the instantiations with 64-bit ADDRESSING (COMPACT = false: arrays above 4 GiB, 64-bit trail words as well):
// three kernel-lifetime values in scratch at six waves
#define TR_DIRECT_W ((!COMPACT || (DEEP && !QN)) ? TR_DEEP_WAVES - 1 : DEEP ? TR_DEEP_WAVES : TR_DIRECT_WAVES)
#define TR_DIRECT_OCC __attribute__((amdgpu_waves_per_eu(TR_DIRECT_W, TR_DIRECT_W)))
#else
#define TR_DIRECT_OCC
#endif
// One workgroup = 128 rays = two waves (block sizes of 64 and 256 rays were options until round 5: never faster, three
// times the kernels -- profiles/r02_sweep.jsonl; the option block_size is accepted and ignored).
constexpr int TR_BS = 128;
template <int Q, bool STATS, bool COMPACT, int MODE = 0, bool DEEP = false, bool QN = false>
__global__ __launch_bounds__(TR_BS) TR_DIRECT_OCC void k_query_direct(tr_bvh_view b, RayFetch rf, QueryOut out,
                                                      int xcd_map, int scramble, int tile_w, int steal_min,
                                                      const uint32_t* __restrict__ order, int order_split,
                                                      uint32_t* __restrict__ cost,
                                                      unsigned long long* stats,
                                                      const int* __restrict__ sel) {
    TR_VIEW_LIVE(b);
    query_direct_body<Q, STATS, COMPACT, TR_BS, MODE, DEEP, QN>(b, rf, out, xcd_map, scramble, tile_w, steal_min, order,
                                                                order_split, cost, stats, sel);
}
// The unordered count launch with stealing (query_direct_body MODE 3) as a kernel of its own, for its occupancy.  It waits more
// than it issues (C4 count: VALU pipes 69 % busy, wait_any 0.59, profiles/r05_c4count_summary.md) and gains from a SEVENTH wave
// per SIMD (72 registers, 8-10 kernel-lifetime values in scratch, none inside the trips; the LDS -- ring + leaf queue -- was
// sized for seven from the start): round 5 measured -3 % and did not ship it, because the instantiation for hierarchies of
// more than 32 levels then died with a memory access fault (profiles/r05_count_waves_fault.txt).  Round 6 narrowed that fault
// to 64-bit-trail instantiations with kernel-lifetime spills (profiles/r06_deep_fault_probe.txt): those -- DEEP, and the ones
// with 64-bit addressing -- keep the compiler's budget, the 32-bit ones run at seven: C4 count 0.717 -> 0.680 ms (round 5:
// 0.688), headline count 0.358 -> 0.344, 4 M rays -4.7 %, the interior scene -1...-2 %, terrain / C3 +-1 %
// (profiles/r06_ab_count_waves.txt).  Eight waves (a 4-entry leaf queue for the LDS): +10...+35 % (round 5).
#ifndef TR_COUNT_WAVES
#define TR_COUNT_WAVES 7
#endif
#if TR_COUNT_WAVES > 0
// (only the instantiations with 32-bit trail words and 32-bit addressing: the others keep the compiler's budget -- kernel-lifetime
// spills in a 64-bit instantiation are the pattern that faulted)
#define TR_COUNT_W ((DEEP || !COMPACT) ? 5 : TR_COUNT_WAVES)
#define TR_COUNT_OCC __attribute__((amdgpu_waves_per_eu(TR_COUNT_W, TR_COUNT_W)))
#else
#define TR_COUNT_OCC
#endif
template <bool COMPACT, bool DEEP>
__global__ __launch_bounds__(TR_BS) TR_COUNT_OCC void k_query_count_steal(tr_bvh_view b, RayFetch rf, QueryOut out,
                                                      int xcd_map, int scramble, int tile_w, int steal_min,
                                                      const uint32_t* __restrict__ order, int order_split,
                                                      uint32_t* __restrict__ cost,
                                                      unsigned long long* stats,
                                                      const int* __restrict__ sel) {
    TR_VIEW_LIVE(b);
    query_direct_body<TR_Q_COUNT, false, COMPACT, TR_BS, 3, DEEP, false>(b, rf, out, xcd_map, scramble, tile_w, steal_min, order,
                                                                         order_split, cost, stats, sel);
}

// ... and the count launch that carries the deferred sort (see k_query_direct_sort below; 32-bit addressing only)
template <bool DEEP, bool COMPACT = true>
__global__ __launch_bounds__(TR_BS) TR_COUNT_OCC void k_query_count_steal_sort(tr_bvh_view b, RayFetch rf, QueryOut out,
                                                      int xcd_map, int scramble, int tile_w, int steal_min,
                                                      const uint32_t* __restrict__ order, int order_split,
                                                      unsigned long long* stats, tr_sort_job job) {
    TR_VIEW_LIVE(b);
    query_direct_body<TR_Q_COUNT, false, true, TR_BS, 3, DEEP, false, true>(b, rf, out, xcd_map, scramble, tile_w, steal_min, order,
                                                                            order_split, nullptr, stats, nullptr,
                                                                            tr_wide_args{nullptr, nullptr, 0, 0}, job);
}

// The stealing closest / first / any launch on the grid nodes that CARRIES the deferred sort of the last measured block costs
// (tr_sort_job, sched_acquire: every fourth launch of a batch shape in its steady state): eight launch slots more in front,
// workgroup 0 sorts, 1-7 leave (query_direct_body).  A kernel of its own so that the launches without a sort run the very
// code they ran before (the sorter in the common kernel cost it 1 %: 64-bit block arithmetic, two registers, a longer
// argument block -- profiles/r05_ab_sort_inline.txt).
template <int Q, bool DEEP, bool QN = true, bool COMPACT = true>      // (always the grid nodes and 32-bit addressing; named for TR_DIRECT_OCC)
__global__ __launch_bounds__(TR_BS) TR_DIRECT_OCC void k_query_direct_sort(tr_bvh_view b, RayFetch rf, QueryOut out,
                                                      int xcd_map, int scramble, int tile_w, int steal_min,
                                                      const uint32_t* __restrict__ order, int order_split,
                                                      unsigned long long* stats, tr_sort_job job) {
    TR_VIEW_LIVE(b);
    query_direct_body<Q, false, true, TR_BS, 1, DEEP, true, true>(b, rf, out, xcd_map, scramble, tile_w, steal_min, order,
                                                                  order_split, nullptr, stats, nullptr,
                                                                  tr_wide_args{nullptr, nullptr, 0, 0}, job);
}

// The direct launch on the 8-wide compressed nodes (query_direct_body MODE 4; option wide_direct): the block -> ray
// map, the tiles and the learned launch order of the direct launch, the per-lane two-stack walk of k_query_wide.
template <int Q>
__global__ __launch_bounds__(128) void k_query_direct_wide(tr_bvh_view b, RayFetch rf, QueryOut out, int xcd_map, int scramble,
                                                           int tile_w, const uint32_t* __restrict__ order, int order_split,
                                                           uint32_t* __restrict__ cost, unsigned long long* stats,
                                                           const int* __restrict__ sel, tr_wide_args wa) {
    TR_VIEW_LIVE(b);
    query_direct_body<Q, false, true, TR_BS, 4, false, false>(b, rf, out, xcd_map, scramble, tile_w, 0, order, order_split,
                                                              cost, stats, sel, wa);
}

// A batch of a new SHAPE (another image resolution of the same scene) need not start from nothing: the block costs
// measured at the previous shape are resampled onto the new launch's blocks -- block b of the new launch covers some
// piece of the image, the old block that covered that piece lends its cost -- and sorted into a launch order before the
// first launch of the new shape (VERDICT r03 "next" #7b: a resolution change fell back to the static order, 0.33-0.43 ms
// for the headline batch).  Shapes: image width / height and the rows-per-tile exponent of the block -> ray map
// (0 = rows of 64 pixels); blocks hold 128 rays.  Speed only: any order is a correct order.
__device__ __forceinline__ void sched_block_pixel(int64_t b, int64_t w, int lgh, int64_t* x, int64_t* y) {
    const int64_t i = b * 128;
    if (lgh == 0) { *y = i / w; *x = i - *y * w; return; }
    const int lgw = 6 - lgh;
    const int64_t tile = i >> 6, tpr = w >> lgw, ty = tile / tpr, tx = tile - ty * tpr;
    *y = ty << lgh; *x = tx << lgw;
}
__global__ __launch_bounds__(256) void k_sched_rescale(const uint32_t* __restrict__ prev, int64_t pn, int64_t pw, int64_t ph, int plgh,
                                                       uint32_t* __restrict__ cost, int64_t nn, int64_t w, int64_t h, int lgh) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nn) return;
    int64_t x, y;
    sched_block_pixel(b, w, lgh, &x, &y);
    // the block's footprint: 128 pixels of a row, or two tiles side by side; sampled at 4 x 2 points, the lenders' costs
    // averaged (a block of 8 rows x 16 pixels that borrows from blocks of 1 row x 128 pixels meets eight of them)
    const int64_t fw = lgh ? (int64_t)(128 >> lgh) : 128, fh = lgh ? (int64_t)(1 << lgh) : 1;
    unsigned long long sum = 0;
    int cnt = 0;
#pragma unroll
    for (int sy = 0; sy < 4; sy++)
#pragma unroll
        for (int sx = 0; sx < 2; sx++) {
            const double fx = ((double)x + (double)fw * (0.25 + 0.5 * sx)) / (double)w;
            const double fy = ((double)y + (double)fh * (0.125 + 0.25 * sy)) / (double)h;
            int64_t xo = (int64_t)(fx * (double)pw), yo = (int64_t)(fy * (double)ph);
            xo = xo < 0 ? 0 : (xo >= pw ? pw - 1 : xo);
            yo = yo < 0 ? 0 : (yo >= ph ? ph - 1 : yo);
            int64_t io;
            if (plgh == 0) io = yo * pw + xo;
            else {
                const int plgw = 6 - plgh;
                io = (((yo >> plgh) * (pw >> plgw) + (xo >> plgw)) << 6);
            }
            const int64_t bo = io >> 7;
            if (bo < pn) { sum += prev[bo]; cnt++; }
        }
    cost[b] = cnt ? (uint32_t)(sum / (unsigned)cnt) : 0u;
}

// the sort as a launch of its own: behind the measuring launches of a batch shape's learning phase, and wherever the
// next launch cannot carry it (sched_acquire)
__global__ __launch_bounds__(1024) void k_sched_sort(uint32_t* __restrict__ cost,
                                                      uint32_t* __restrict__ order, int nblocks,
                                                      int xcd_map, int split, int split4,
                                                      int outlier8, int floor_ticks,
                                                      const int* __restrict__ sel, uint32_t* __restrict__ prev) {
    // dual launch (k_probe_coherence): the direct launch whose costs this would sort returned at its first
    // instruction -- nothing was measured, the order (if any) stays as it is (round 3 sorted an all-zero cost
    // array of 97 656 blocks behind every streamed 12.5 M-ray launch: 215 us of serial work per call)
    if (sel && *sel != 0) return;
    __shared__ uint32_t bins[8][256];
    __shared__ alignas(8) uint32_t misc[16];
    sched_sort_body<1024>(cost, order, nblocks, xcd_map, split, split4, outlier8, floor_ticks, prev, bins, misc);
}

