// kernels_stream.inc -- included by traverse.hip inside its anonymous namespace: the STREAMING launch for incoherent
// batches (persistent waves, ballot / mbcnt refill of idle lanes) on the binary grid nodes, and the coherence probe
// that picks between it and the direct launch on the device.  (The same launch on the 8-wide nodes: traverse_wide.inc.)
// ---- streaming launch with wave-level ray refill ("active-ray repacking") -------------------------
// For incoherent batches a wave of the direct launch runs until its slowest ray is done while most
// of its lanes finished long ago: VALU lane utilisation is 10 of 64 on C3 and on a C5(ii) shard
// (profiles/r02_c3any_summary.md, r02_c5s_summary.md) against 35-49 on coherent images.  Here
// every wave owns a contiguous range of `rays_per_wave` rays and keeps its lanes busy: whenever at
// least `refill_min` lanes are idle it stores their finished results and hands them the next rays
// of ITS OWN range -- no atomics, no work counters (the round-1 refill kernel paid three dependent
// round trips per refill: flush, atomic, ray fetch), just a wave-uniform cursor and a prefix rank
// (v_mbcnt) among the idle lanes.  One refill costs about one trip and serves >= refill_min rays.
// Results do not depend on the schedule: the per-ray state machine is the fused trip of the direct
// launch (tr_fused_step), only the lane <-> ray assignment changes.
// Which of the two launch shapes suits a large flat batch?  Coherent rays (a flattened image) run
// 1.6-1.9x faster in the direct launch (XCD-local image pieces, measured launch order, lanes that
// share nodes), incoherent ones 1.3-1.9x faster in the streaming launch
// (profiles/r02_sweep_stream*.jsonl).  One workgroup samples 256 pairs of NEIGHBOURING rays
// spread over the batch: a pair is coherent when the directions are within ~2.5 degrees and the
// origins within 1 % of the scene diagonal.  *sel = 0 (direct) when at least 3/4 of the pairs
// are, else 1 (stream).  Both kernels are then enqueued and the one not selected returns at its
// first instruction -- no host round trip; a wrong guess costs speed, never correctness.
__global__ __launch_bounds__(256) void k_probe_coherence(RayFetch rf, float scene_diag, int* __restrict__ sel) {
    __shared__ int votes;
    if (threadIdx.x == 0) votes = 0;
    __syncthreads();
    const int64_t stride = rf.n / 256 > 0 ? rf.n / 256 : 1;
    const int64_t i = (int64_t)threadIdx.x * stride;
    if (i + 1 < rf.n) {
        float o0[3], d0[3], o1[3], d1[3];
        fetch_ray(rf, i, o0, d0);
        fetch_ray(rf, i + 1, o1, d1);
        const float dd = d0[0] * d1[0] + d0[1] * d1[1] + d0[2] * d1[2];
        const float n0 = d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2];
        const float n1 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
        const float ox = o1[0] - o0[0], oy = o1[1] - o0[1], oz = o1[2] - o0[2];
        const bool par = dd > 0.f && dd * dd >= 0.998f * n0 * n1;                    // cos^2 >= 0.998
        const bool near = ox * ox + oy * oy + oz * oz <= 1e-4f * scene_diag * scene_diag;
        if (par && near) atomicAdd(&votes, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *sel = votes >= 192 ? 0 : 1;
        sel[2] = 0; sel[3] = 0;        // the streaming launch's work counter (2nd 64-bit word of the slot)
    }
}

template <int Q, bool STATS, bool COMPACT, int BS, bool DEEP>
__device__ __forceinline__ void query_stream_body(const tr_bvh_view& b, const RayFetch& rf, const QueryOut& out,
                                                  int rays_per_wave, int refill_min, int xcd_map,
                                                  unsigned long long* stats,
                                                  const int* __restrict__ sel,
                                                  unsigned long long* work) {
    if (sel && *sel != 1) return;      // dual launch: this is the shape for incoherent batches (id 1)
    typedef typename tr_word<COMPACT, DEEP>::T W;
    __shared__ int32_t ring_lds[TR_RING * BS];
    const tr_ring ring = {ring_lds + threadIdx.x, BS};
    // the XCD-chunked block -> range map of the direct launch: consecutive ranges stay on one
    // XCD's L2 in chunks of `xcd_map` blocks (matters for coherent batches; speed only)
    int64_t blk = blockIdx.x;
    if (xcd_map > 0) {
        const int64_t T = xcd_map, span = 8 * T;
        const int64_t nfull = (int64_t)gridDim.x / span * span;
        if (blk < nfull) {
            const int64_t x = blk & 7, k = blk >> 3;
            blk = ((k / T) * 8 + x) * T + (k % T);
        }
    }
    const int64_t wave = blk * (BS / 64) + (threadIdx.x >> 6);
    int64_t next = wave * rays_per_wave;                 // wave-uniform cursor into the wave's range
    int64_t end = next + rays_per_wave;
    if (end > rf.n) end = rf.n;
    // work != NULL: ranges are handed out by a work counter instead (one atomic per range): a wave
    // that has used its range up takes the next one and keeps refilling, so only the very last
    // range of every wave is drained and the launch ends within one range's time for all waves
    // (the first range of a wave is still the static one: no burst of atomics at the start)
    bool exhausted = work == nullptr;
    const unsigned long long first_dynamic = (unsigned long long)gridDim.x * (BS / 64) * (unsigned long long)rays_per_wave;
    if (next >= rf.n) { next = 0; end = 0; }
    tr_counters cnt = {0, 0, 0};
    int64_t rid = -1;          // ray this lane holds (-1 none); its result is stored when the lane is refilled
    bool busy = false;         // still traversing
    tr_ray r;
    tr_state_t<W> fs;
    tr_result res;
    tr_topk<1> top;
    tr_state_init(fs);
    tr_result_init(res);
    tr_ray_setup_q(r, b.frame, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
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
        const unsigned long long idle = __ballot(!busy);
        const int nidle = __popcll(idle);
        const bool more = next < end;
        if (!more && nidle == 64) break;
        if (more && (nidle >= refill_min || nidle == 64)) {
            if (!busy) {
                if (rid >= 0) write_result<Q>(b, out, rid, r, res);      // the finished ray of this lane
                const int64_t cand = next + lane_rank(idle);
                rid = -1;
                if (cand < end) {
                    rid = cand;
                    float o[3], d[3];
                    fetch_ray(rf, cand, o, d);
                    const bool valid = tr_ray_setup_q(r, b.frame, o[0], o[1], o[2], d[0], d[1], d[2]);
                    tr_state_init(fs);
                    tr_result_init(res);
                    if (b.num_tris >= 2) busy = valid;
                    else brute_one<Q>(b, r, valid, res);                 // no hierarchy below two triangles
                }
            }
            next += nidle;     // lanes past `end` took nothing; the cursor only has to reach `end`
        }
        // trips until the next refill is due (or, once the range is used up, until all lanes are
        // done): a plain single-exit loop like the direct launch's, with a wave-uniform exit test
        const int stop = (next < end || !exhausted) ? refill_min : 64;
        int idle_now;
        do {
            if (busy) {
                tr_fused_step<Q, 1, STATS, COMPACT, W, false, true, TR_STREAM_QN, TR_STREAM_COLD<Q>>(b, r, fs, res, top, &cnt, ring);
                busy = !tr_done(fs);
            }
            TR_CONVERGE();
            // the trip without the leaf block, as a loop of one trip: written without the loop, the first / closest
            // instantiations compile to the same instructions in another order -- an unmeasured change
#pragma unroll
            for (int a = 0; a < 1; a++) {
                if (busy) {
                    tr_fused_step<Q, 1, STATS, COMPACT, W, false, false, TR_STREAM_QN, TR_STREAM_COLD<Q>>(b, r, fs, res, top, &cnt, ring);
                    busy = !tr_done(fs);
                }
                TR_CONVERGE();
            }
            idle_now = __popcll(__ballot(!busy));
        } while (idle_now < stop);
    }
    if (rid >= 0) write_result<Q>(b, out, rid, r, res);
    flush_stats<STATS>(cnt, stats);
}
// (Round 3 ran the compact instantiations at 8 waves per SIMD, 64 registers: -2...-7 %.  Round 4's sign-selected slab
// test needs three registers more and is worth about as much on these fabric-bound launches -- C3 any -1.7 %, C5(ii)
// shard -1 %, count +1.5 % at 7 waves: profiles/r04_ab_qsign.txt -- so every instantiation keeps the compiler's budget.)
// Round 5: the fused box test's per-ray constants (tr_ray_fuse) put the kernel's refill path -- every lane's traversal
// state live across a ray fetch, a set-up and a result write -- at 85-89 registers, five waves per SIMD; asked for six
// (80 registers) the compiler parks 2-5 kernel-lifetime values in scratch (stored once in the prologue, read once per
// refill, nothing inside the trips: tests/test_round4_cpu.py) and the launch is as fast or faster than both the
// five-wave build and round 4's 72-register kernel without the fused test (C3 any 0.892 -> 0.847 ms, C5(ii) shard
// 1.845 -> 1.851, shard count 2.505 -> 2.427; seven waves: slower again -- profiles/r05_ab_stream_waves.txt).
// Round 6: FIVE again.  With the float64 part of the hit predicate a real call at the end of a trip (tr_drain_exact) and
// the barycentrics of the winning triangle from float64 (tr_tri_bary_call, in the refill path) the six-wave build sent
// 5-28 registers to scratch -- the closest kernel's trail word inside the trips in one build -- and measured slower
// than five waves on every incoherent config: C3 closest 1.412 -> 1.154 ms, C3 any 0.838 -> 0.821, C5(ii) shard
// 1.816 -> 1.794 (profiles/r06_ab_stream_waves.txt).  At 96 registers nothing but three kernel-lifetime values of the
// closest kernels spills.
#ifndef TR_STREAM_WAVES
#define TR_STREAM_WAVES 5
#endif
#if TR_STREAM_WAVES > 0
// (the instantiations with 64-bit addressing -- arrays above 4 GiB -- get one wave less)
#define TR_STREAM_OCC __attribute__((amdgpu_waves_per_eu(COMPACT ? TR_STREAM_WAVES : TR_STREAM_WAVES - 1, COMPACT ? TR_STREAM_WAVES : TR_STREAM_WAVES - 1)))
#else
#define TR_STREAM_OCC
#endif
template <int Q, bool COMPACT, int BS, bool DEEP = false>
__global__ __launch_bounds__(BS) TR_STREAM_OCC void k_query_stream(tr_bvh_view b, RayFetch rf, QueryOut out,
                                                     int rays_per_wave, int refill_min, int xcd_map,
                                                     unsigned long long* stats, const int* __restrict__ sel,
                                                     unsigned long long* work) {
    TR_VIEW_LIVE(b);
    query_stream_body<Q, false, COMPACT, BS, DEEP>(b, rf, out, rays_per_wave, refill_min, xcd_map, stats, sel, work);
}
// the instrumented launch (tr_trace_stats_query: three more live counters): the compiler's own register budget
template <int Q, bool COMPACT, int BS, bool DEEP = false>
__global__ __launch_bounds__(BS) void k_query_stream_stats(tr_bvh_view b, RayFetch rf, QueryOut out,
                                                           int rays_per_wave, int refill_min, int xcd_map,
                                                           unsigned long long* stats, const int* __restrict__ sel,
                                                           unsigned long long* work) {
    TR_VIEW_LIVE(b);
    query_stream_body<Q, true, COMPACT, BS, DEEP>(b, rf, out, rays_per_wave, refill_min, xcd_map, stats, sel, work);
}
