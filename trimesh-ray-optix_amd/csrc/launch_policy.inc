// launch_policy.inc -- included by traverse.hip inside its anonymous namespace: the HOST side of a query -- device
// checks, the per-(handle, stream) scheduling state (learned launch order, node-flavour tuner), and launch_query: which
// launch shape a batch gets and why.  (Ray marshaling: make_fetch, kernels_common.inc.)
// ---- host side ----------------------------------------------------------------------------------
// Every query runs on the device that owns the BVH arena, whatever device is current in the
// calling thread (tr_device_guard restores it), and refuses rays that live on another GPU:
// the kernel would dereference them (or the arena) across devices -- a memory fault that kills
// the process, or silent peer traffic.  The pointer query is skipped when the caller is already
// on the handle's device (the common, checked-by-the-binding case costs nothing extra).
int enter_bvh_device(const tr_bvh* bvh, const tr_rays* rays, tr_device_guard* guard) {
    TR_TRY(tr_enter_device(guard, bvh->device));
    if (guard->changed && rays && rays->nray > 0) {
        for (const float* p : {rays->d_origins, rays->d_directions}) {
            hipPointerAttribute_t attr;
            if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); continue; }
            if (attr.type == hipMemoryTypeDevice && attr.device != bvh->device)
                return tr_fail(TR_ERR_INVALID_ARG, "rays are on device " + std::to_string(attr.device) +
                                                       " but the BVH lives on device " + std::to_string(bvh->device));
        }
    }
    return TR_OK;
}

// ---- adaptive launch order ------------------------------------------------------------------------------------------------
// The blocks of a launch are started most-expensive-first, in the order learned from the measured block costs of the
// previous launches on the same (handle, stream) with the same block count: the longest rays of a batch -- its critical
// path -- do not start last.  Hints never affect results; each stream has its own buffers, so overlapping launches cannot
// see a half-written order.
// buf = cost[TR_SCHED_MAX] | order 0 | its stamp (block count, split blocks, 2 spare words) | 8 words of per-stream launch
// scratch (coherence-probe result, work counter) | costs of the last sort | order 1 | its stamp
constexpr size_t TR_SCHED_WORDS = 4 * (size_t)TR_SCHED_MAX + 4 + 8 + 4;
constexpr int64_t TR_MEASURE_EVERY = 4;     // (a power of two) steady state of a batch shape: every 4th launch measures its block costs
                                            // (every 2nd: r05_ab_measure_every.txt)
constexpr int64_t TR_MEASURE_MASK = TR_MEASURE_EVERY - 1;
constexpr size_t TR_SCHED_PREV = 2 * (size_t)TR_SCHED_MAX + 4 + 8;
constexpr size_t TR_SCHED_ORDER1 = 3 * (size_t)TR_SCHED_MAX + 4 + 8;
// the two order buffers of a slot (each followed by its stamp): launches read order_buf(slot, slot->cur), sorts write the other
inline uint32_t* order_buf(const tr_sched_slot* slot, int k) { return slot->buf + ((k & 1) ? TR_SCHED_ORDER1 : (size_t)TR_SCHED_MAX); }
// the slot of (stream, class) of this handle, created on first use; sched_mutex must be held
tr_sched_slot* sched_slot(tr_bvh* mb, hipStream_t stream, int cls) {
    for (int k = 0; k < TR_SCHED_SLOTS; k++)
        if (mb->sched[k].used && mb->sched[k].stream == stream && mb->sched[k].cls == cls) return &mb->sched[k];
    for (int k = 0; k < TR_SCHED_SLOTS; k++)
        if (!mb->sched[k].used) {
            uint32_t* buf = nullptr;
            if (hipMalloc((void**)&buf, sizeof(uint32_t) * TR_SCHED_WORDS) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            if (hipMemsetAsync(buf, 0, sizeof(uint32_t) * TR_SCHED_WORDS, stream) != hipSuccess) { (void)hipFree(buf); return nullptr; }
            mb->sched[k].used = true; mb->sched[k].stream = stream; mb->sched[k].cls = cls; mb->sched[k].buf = buf; mb->sched[k].nblocks = 0;
            return &mb->sched[k];
        }
    return nullptr;
}

// Eight words that belong to (handle, stream): the coherence probe's result and the streaming
// launch's work counter.  Launches of one stream are ordered, so the words are never shared by two
// launches in flight -- also not when one of them is a graph replay (a slot of the per-device ring,
// the fallback when the handle has no free slot, is reused after 512 launches on ANY stream).
unsigned long long* stream_scratch(const tr_bvh* bvh, tr_device_state* st, hipStream_t stream) {
    tr_bvh* mb = const_cast<tr_bvh*>(bvh);
    if (mb->sched_mutex) {
        std::lock_guard<std::mutex> lock(*mb->sched_mutex);
        tr_sched_slot* slot = sched_slot(mb, stream, 0);
        if (slot) return reinterpret_cast<unsigned long long*>(slot->buf + 2 * (size_t)TR_SCHED_MAX + 4);
    }
    unsigned slot = __atomic_fetch_add(&st->next_counter, 1u, __ATOMIC_RELAXED) % (TR_NUM_COUNTERS / 8);
    return reinterpret_cast<unsigned long long*>(st->counters) + 8 * slot;
}

// The one place that enqueues k_sched_sort: `cost` sorted into `order` (and zeroed), a copy of what was sorted kept in
// `prev` (NULL: none); behind a launch that the coherence probe may have switched off, `sel` is the probe's verdict.
void enqueue_sort(hipStream_t stream, uint32_t* cost, uint32_t* order, const tr_sort_params& p, const int* sel, uint32_t* prev) {
    hipLaunchKernelGGL(k_sched_sort, dim3(1), dim3(1024), 0, stream, cost, order, p.nblocks, p.xc, p.split, p.split4, p.outlier8,
                       p.floor_ticks, sel, prev);
}

struct sched_shape {        // a launch as the learned order sees it: what sched_acquire stamps, k_sched_rescale resamples and k_sched_sort sorts
    int64_t w, h;           // image width / height of the batch (0: not image-shaped)
    int tile_w;             // the block -> ray map of the kernels: 0 rows of 64 pixels, else width | rows-per-tile exponent << 28
    tr_sort_params sort;
    int lgh() const { return tile_w ? (tile_w >> 28) & 3 : 0; }
};
struct sched_grant {                    // what sched_acquire grants a launch
    bool plain = true;                  // the launch takes the `plain` shape (false: `want`)
    const uint32_t* order = nullptr;    // the learned order it reads (NULL: none exists for this block count)
    uint32_t* cost = nullptr;           // != NULL: it records its block costs here
    uint32_t* order_out = nullptr;      // != NULL: ... and a k_sched_sort right behind it sorts them into this buffer
    tr_sort_job job = {nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0};   // cost != NULL: the deferred sort it carries as an extra workgroup
};
inline bool sched_matches(const tr_sched_slot* slot, int64_t nblocks, const sched_shape& sh) {
    return slot->nblocks == nblocks && slot->split == sh.sort.split && slot->lgh == sh.lgh();
}

// Phase 1: the slot's deferred sort, which this launch cannot carry, now, as a kernel of its own; launches read the new order.
void sched_flush_pending(tr_sched_slot* slot, hipStream_t stream) {
    enqueue_sort(stream, slot->buf, order_buf(slot, slot->cur ^ 1), slot->pending_sort, nullptr, slot->buf + TR_SCHED_PREV);
    (void)hipGetLastError();
    slot->cur ^= 1;
    slot->pending = false;
}

// Phase 2: a launch whose shape the slot is not stamped with -- the first launches of a batch shape.  The shape a batch runs
// in once it has a learned order (`want`: tiles + split blocks) is a poor shape WITHOUT one: 8x8 tiles pack the expensive
// silhouette rays into the same waves, and only the split slots -- which need measured costs -- take those waves apart again
// (headline batch: 0.42 ms for tiles without an order against 0.33 ms for rows).  So the FIRST launch of a batch shape on a
// (handle, stream) runs in the plain shape (`plain`: the tile rule of launches without split blocks, no split slots); its
// measured block costs -- uninflated: nothing was split -- order and split the SECOND launch, which runs in `want`.  When
// the slot holds the costs of the last sort and the stream is not `recording` into a graph, they order this launch already:
// resampled from ANOTHER image shape (a change of resolution: option order_transfer, k_sched_rescale), or as they are when
// they were measured on these very blocks.  Returns the shape taken and the order to read.
sched_grant sched_first_launches(tr_sched_slot* slot, const tr_options& opt, hipStream_t stream, int64_t nblocks,
                                 const sched_shape& want, const sched_shape& plain, bool recording) {
    sched_grant g;
    slot->launches = 0;
    const bool same_shape = want.sort.split == plain.sort.split && want.lgh() == plain.lgh();
    // Second launch of this batch shape (the first ran `plain`, the slot is stamped with it): on to `want`; anything
    // else -- a fresh slot, another resolution -- starts in `plain`.  (The step must not depend on `lend` below:
    // a batch that is not image-shaped -- a flat [n, 3] batch with split slots -- or a launch issued under stream
    // capture would never leave the plain shape, never get an order and re-measure behind every launch: ADVICE r04.)
    const bool second = !same_shape && sched_matches(slot, nblocks, plain);
    g.plain = !(second || same_shape);
    const sched_shape& use = g.plain ? plain : want;
    const bool can_sort = opt.order_transfer && slot->prev_valid && !recording;
    // the costs of the last sort can be resampled when both shapes are images and nothing is being captured
    const bool lend = can_sort && slot->prev_w > 0 && want.w > 0;
    // ... and taken as they are when the wanted shape has the very blocks they were measured on: the second launch
    // of a batch whose plain and wanted shapes share the block -> ray map (a flat batch: only the split slots differ)
    const bool reuse = can_sort && !lend && second && slot->prev_nblocks == nblocks && slot->prev_w == want.w &&
                       slot->prev_h == want.h && slot->prev_lgh == want.lgh();
    uint32_t* prev = slot->buf + TR_SCHED_PREV;
    tr_sort_params sort = use.sort;
    bool have_costs = lend;         // slot->buf holds costs that can order this launch
    if (lend) {
        hipLaunchKernelGGL(k_sched_rescale, dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0, stream, prev, slot->prev_nblocks,
                           slot->prev_w, slot->prev_h, slot->prev_lgh, slot->buf, nblocks, use.w, use.h, use.lgh());
        // borrowed costs only ORDER the launch: no block is split on their word (outlier threshold out of reach: the
        // extra launch slots stay sentinels).  The split set is sticky by design -- a split block records its cost
        // doubled so that it stays split -- and a set chosen from resampled costs stayed, and cost the terrain 18 %
        // and the shells 4 % for good (profiles/r04_first_launch_policy_debug.txt); the sort behind THIS launch picks
        // it from costs measured on this launch's own blocks.
        sort.outlier8 = 1 << 20;
    } else if (reuse) {
        // measured on these blocks, nothing split, nothing resampled: they order the launch AND pick its split set
        have_costs = hipMemcpyAsync(slot->buf, prev, sizeof(uint32_t) * (size_t)nblocks, hipMemcpyDeviceToDevice, stream) == hipSuccess;
        if (!have_costs) (void)hipGetLastError();
    }
    if (have_costs) {
        enqueue_sort(stream, slot->buf, order_buf(slot, slot->cur), sort, nullptr, nullptr);
        if (hipGetLastError() == hipSuccess) g.order = order_buf(slot, slot->cur);
    }
    slot->prev_valid = false;      // (the costs kept are used up; the sort behind this launch keeps new ones)
    return g;
}

// Phase 3: does this launch -- of shape `use`, the slot's `launches`-th -- measure its block costs, and where does their
// sort go?  Measure + re-sort after each of the first three launches of a batch shape, then every 4th: the costs of a scene
// change slowly and the sort (8 us) is serial work behind every launch.  In the learning phase the sort runs right behind
// the launch (g.order_out); in the steady state it is DEFERRED into the next launch of the shape, which does not measure,
// carries it as an extra workgroup and still reads the old order (`can_carry`: the launch is of a kernel flavour that has
// the sorter).  Fills g.cost and g.order_out.
void sched_measure(tr_sched_slot* slot, const tr_options& opt, int64_t nblocks, const sched_shape& use, bool can_carry,
                   bool recording, sched_grant& g) {
    // (no measurement while a deferred sort waits behind a graph recording: the cost array is still the unsorted one)
    if (!(slot->pending && recording) && (slot->launches < 3 || (slot->launches & TR_MEASURE_MASK) == TR_MEASURE_MASK)) {
        g.cost = slot->buf;
        // the sort behind this launch keeps a copy of what it sorted, in this launch's shape
        slot->prev_valid = true;
        slot->prev_nblocks = nblocks; slot->prev_w = use.w; slot->prev_h = use.h; slot->prev_lgh = use.lgh();
        if (slot->launches >= 3 && can_carry && !recording && opt.sort_inline && !g.plain && nblocks <= (1 << 16)) {
            // steady state: the sort is deferred into the next launch of this shape (which does not measure)
            slot->pending = true;
            slot->pending_sort = use.sort;
        } else {
            // behind this launch, into the buffer the NEXT launches read
            g.order_out = order_buf(slot, slot->cur ^ 1);
            slot->cur ^= 1;
        }
    }
}

// What the learned order grants the direct launch of `nblocks` blocks on (handle, stream): its shape, the order it reads,
// whether it measures, and the sort it carries or is followed by.  Nothing is granted (the plain shape, no order, no
// measurement) without option adaptive, below 64 blocks, above TR_SCHED_MAX, or when the handle has no free slot.
sched_grant sched_acquire(const tr_bvh* bvh, const tr_options& opt, hipStream_t stream, int64_t nblocks,
                          const sched_shape& want, const sched_shape& plain, bool can_carry) {
    tr_bvh* mb = const_cast<tr_bvh*>(bvh);
    if (!opt.adaptive || !mb->sched_mutex || nblocks < 64 || nblocks > TR_SCHED_MAX) return sched_grant{};
    // launches with split blocks (the stealing shapes) and launches without learn separate orders:
    // their costs differ, and a plain shape would only skip the extra slots of a split order
    const int cls = want.sort.split != 0;
    std::lock_guard<std::mutex> lock(*mb->sched_mutex);
    tr_sched_slot* slot = sched_slot(mb, stream, cls);
    if (!slot) return sched_grant{};
    const bool measures_next = slot->launches + 1 < 3 || ((slot->launches + 1) & TR_MEASURE_MASK) == TR_MEASURE_MASK;
    // A launch that is being RECORDED into a graph neither carries the deferred sort (it would sort again at every replay)
    // nor has it run in front of it (the sort would only exist in the graph): the sort stays pending for the next launch
    // that is really enqueued.
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool recording = hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (recording) (void)hipGetLastError();
    if (slot->pending && !recording && !(sched_matches(slot, nblocks, want) && can_carry && opt.sort_inline && !measures_next))
        sched_flush_pending(slot, stream);
    sched_grant g;
    if (sched_matches(slot, nblocks, want)) {
        g.plain = false;
        g.order = order_buf(slot, slot->cur);
        slot->launches++;
        if (slot->pending && !recording) {
            // the slot's deferred sort as the kernels take it: into the buffer that launches do NOT read
            const tr_sort_params& p = slot->pending_sort;
            g.job = tr_sort_job{slot->buf, order_buf(slot, slot->cur ^ 1), slot->buf + TR_SCHED_PREV, p.nblocks, p.xc, p.split, p.split4, p.outlier8, p.floor_ticks};
            slot->cur ^= 1;          // (this launch reads the buffer handed out above; the next ones the new order)
            slot->pending = false;
        }
    } else {
        g = sched_first_launches(slot, opt, stream, nblocks, want, plain, recording);
    }
    const sched_shape& use = g.plain ? plain : want;
    slot->nblocks = nblocks;   // the sort enqueued after the launch makes it valid for the next one
    slot->split = use.sort.split;
    slot->lgh = use.lgh();
    sched_measure(slot, opt, nblocks, use, can_carry, recording, g);
    return g;
}

// the 8-wide nodes of the handle, built if necessary (defined behind the scan kernels' host wrapper); NULL = not
// available for this launch (the caller keeps the binary launch shapes)
const tr_wnode* ensure_wide(const tr_bvh* bvh, hipStream_t stream);
int32_t* wide_spill(const tr_bvh* bvh, hipStream_t stream, size_t elems);

// ---- the launch policy: every threshold in one place, with the measurement that set it ---------------------------
// (none of it changes results; the files are under profiles/)
struct tr_policy {
    // which launch
    // From how many rays on the streaming launch is enqueued beside the direct one, behind the coherence probe (incoherent batches
    // 1.3-1.9x faster, coherent ones 0.55x: r02_sweep_stream*.jsonl).  Round 5 re-measured where the two cross on incoherent hash
    // rays, streaming forced against the direct launch forced, per query and mesh -- twice: with the direct launch as it was
    // (r05_policy_stream_boundary.txt: one boundary of 2 M rays cost a 2.2 M-ray count 44 %), and again after its waves of
    // unrelated rays learned to steal from their first look on (wave_traverse_steal: the direct launch 26-32 % faster on such
    // batches, r05_ab_steal_incoherent.txt).  Closest / first / any: the size up to which the direct launch steals at all
    // (STEAL_MAX_RAYS; 2.2 M rays: direct 0.30 / 0.37 ms against 0.37 / 0.55 streamed on the 82 k- / 1.31 M-triangle mesh, 4.2 M:
    // equal / direct 8 % faster, 6 M -- no stealing any more --: streaming 27-38 % faster); COUNT, whose direct launch steals
    // from its first look (USTEAL_FROM_TRIP) and splits: 16 M (at 2.2 M rays the direct launch is 44 % faster than streaming, at
    // 6 M 10-33 %, at 12.5 M 0-4 %, at 16.7 M streaming 2 %, at 25 M 6-7 %: r05_ab_usteal_trip.txt).
    static int64_t stream_min_rays(const tr_device_state* st, int query) {
        if (query == TR_Q_COUNT) return rounds3(st, 128);      // 16 M rays
        return steal_max_rays(st) + 1;
    }
    // Ray-count boundaries in DEVICE UNITS (round 6, VERDICT r05 "next" #6): what was measured is how many ROUNDS OF RESIDENT LANES a
    // batch is -- lanes = CUs x resident waves per CU of the stealing closest launch x 64, the CU count from the device, the waves
    // from the occupancy query (tr_policy_units) -- not an absolute ray count.  On the MI355X in SPX mode (256 CUs x 24 waves x 64 =
    // 393 216 lanes) the figures are the ones every profile below was taken with: 32/3 rounds = 4 M rays, 64/3 = 8 M, 128/3 = 16 M;
    // on a partition (CPX: one XCD of 32 CUs per device) or another SKU they scale with the device instead of staying put.
    static int64_t rounds3(const tr_device_state* st, int64_t thirds) { return (int64_t)st->num_cus * (st->waves_per_cu > 0 ? st->waves_per_cu : WAVES_PER_CU) * 64 * thirds / 3; }
    static int64_t steal_max_rays(const tr_device_state* st) { return rounds3(st, 32); }   // intra-wave stealing, split slots and tiles-by-splitting up to 4 M rays:
                                                                                           // r02_sweep_steal.jsonl (+11 % at 1 M, -7 % at 10 M incoherent rays)
    static int64_t tile_min_rays(const tr_device_state* st) { return rounds3(st, 32); }    // 8x8 tiles on their own (no split slots) from 4 M rays on: r02_sweep_tile_density.jsonl
    static constexpr int64_t WIDE_MIN_TRIS = 1000000;              // streaming launch on the 8-wide nodes: r05_ab_wide_waves.txt (1.31 M: -3 %, 82 k: +10 %)
    static int64_t wide_min_rays(const tr_device_state* st) { return rounds3(st, 64); }    // ... and only for batches of 8 M rays and more: r05_policy_wide_by_query.txt (1.31 M
                                                                   // triangles: 12.5 M rays closest -4 %, first -3.5 %, count -20 %, but 4.2 M rays +5...+7 %
                                                                   // for closest / first / any; 5.2 M triangles: 12.5 M rays -10...-27 %, 4.2 M rays closest +12 %)
    static constexpr int64_t WIDE_LIST_MIN_TRIS = 500000;          // multi-hit list query on the 8-wide nodes (direct launch): r04_policy_*.txt
    // split slots of the learned order: the nblocks >> shift most expensive blocks, by launch size (r03_sweep_small_split.jsonl,
    // r03_ab_split_half.txt); flat batches below 2048 blocks >> 4
    static int split_shift_tiled(int64_t nblocks) { return nblocks <= 2048 ? 2 : (nblocks <= 4096 ? 3 : (nblocks <= 8192 ? 4 : (nblocks < 32768 ? 5 : 0))); }
    static constexpr int64_t SPLIT_MIN_BLOCKS = 512;               // no split slots below 64 k rays (launches of one round of waves)
    // a block is really split when it costs >= outlier8 / 8 of the mean: 1.0 x while the launch leaves wave slots free, 2.5 x
    // from two rounds of waves on (r03_sweep_outlier.jsonl)
    static int outlier8(double rounds_of_waves) { return rounds_of_waves <= 1.0 ? 8 : (rounds_of_waves >= 2.0 ? 20 : 8 + (int)(12.0 * (rounds_of_waves - 1.0))); }
    static constexpr int WAVES_PER_CU = 24;                        // resident waves of the stealing closest launch (6 per SIMD: r05a_summary.md)
    static constexpr int STEAL_FROM_TRIP = 64;                     // a ray gives subtrees away from its 64th trip on (48: -6 %, 32: -15 %: r02_sweep_steal_share.jsonl)
    static constexpr int REFILL_ORDERED = 28, REFILL_UNORDERED = 20;   // idle lanes that trigger a refill of the streaming launches: r05_retune_refill.txt
    static constexpr int USTEAL_FROM_TRIP = 4;                     // ... in the unordered count launch: from its first look (nothing is culled in a count, so nothing
                                                                   // is lost by giving away early: r05_ab_usteal_trip.txt -- incoherent batches -9...-12 % against 16, images equal)
};

// resident waves per CU of the launch the ray-count boundaries were measured with (the stealing closest launch on the grid
// nodes), from the runtime's occupancy calculator instead of the constant 24; once per device
void tr_policy_units(tr_device_state* st) {
    if (st->waves_per_cu > 0) return;
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_query_direct<TR_Q_CLOSEST, false, true, 1, false, true>, TR_BS, 0);
    if (e != hipSuccess) (void)hipGetLastError();
    st->waves_per_cu = (e == hipSuccess && nb > 0) ? nb * (TR_BS / 64) : tr_policy::WAVES_PER_CU;
}

// The batch as an image, from the shape of its ray tensor (once per call).  Three predicates, different on purpose:
struct batch_image {
    bool image_shaped;      // [..., H, W, 3] in whole rows of 8 <= W < 2^28 pixels: block costs can be resampled between resolutions
    int64_t w, h;           // ... its width and rows (0: not image-shaped)
    bool rows_padded;       // the block -> ray map of the direct launch is laid over the batch padded to whole 8-row tiles
    int64_t n_map;          // ... the rays that map covers (rf.n unless rows_padded)
    bool rows_tile8;        // W % 8 == 0 and n_map is whole bands of 8 rows: a wave can take an 8x8 pixel tile
    explicit batch_image(const RayFetch& rf) {
        image_shaped = rf.s1 > 1 && rf.s2 >= 8 && rf.s2 < (1 << 28) && rf.n % rf.s2 == 0;
        w = image_shaped ? rf.s2 : 0;
        h = image_shaped ? rf.n / rf.s2 : 0;
        // Image-shaped batches whose row count is not a multiple of 8 (from 64 rows on): the block -> ray map of the direct
        // launch is laid over the batch PADDED to whole 8-row tiles -- a tile row beyond the batch maps to ray indices >= n,
        // which every kernel treats as out of range -- so that such a batch keeps the tile shapes (a 1050-row band of the
        // headline image: 0.241 ms in rows of 64 pixels, 0.206 in 8x8 tiles)
        rows_padded = rf.s1 > 1 && rf.s2 % 8 == 0 && rf.s2 >= 8 && rf.s2 < (1 << 28) && rf.n % rf.s2 == 0 &&
                      rf.n % (8 * rf.s2) != 0 && rf.n >= 64 * rf.s2;
        n_map = rows_padded ? (rf.n / rf.s2 + 7) / 8 * 8 * rf.s2 : rf.n;
        rows_tile8 = rf.s1 > 1 && rf.s2 % 8 == 0 && rf.s2 >= 8 && rf.s2 < (1 << 28) && n_map % (8 * rf.s2) == 0;
    }
};

// The addressing flavour of a launch (compact / deep / generic: launch_query) handed to a kernel family's launch as the
// compile-time constants (COMPACT, DEEP) of its template: launch(c, d) names the family once and says with `if constexpr`
// which of the three flavours it does not have
template <typename F>
void by_addressing(bool compact, bool deep, F launch) {
    if (compact) launch(std::true_type{}, std::false_type{});
    else if (deep) launch(std::true_type{}, std::true_type{});
    else launch(std::false_type{}, std::false_type{});
}
template <int M> using tr_mode = std::integral_constant<int, M>;    // MODE of k_query_direct: 0 plain / 1 stealing / 2 the unordered schedule

// The 8-wide walk keeps `lds_cap` entries of a lane's node stack in LDS and the rest in a global spill row of `spill_cap`
// entries.  Node-stack bound: 7 pending siblings per wide level + the 8 children of the node in hand.
struct wide_caps { int lds_cap, spill_cap; };
wide_caps wide_stack_caps(const tr_bvh* bvh, const tr_options& opt) {
    const int need = 7 * ((bvh->depth + 2) / 3) + 9;
    const int lds_cap = opt.wide_stack < TR_WSTACK ? opt.wide_stack : TR_WSTACK;
    return wide_caps{lds_cap, need > lds_cap ? need - lds_cap : 0};
}

// The shape of a batch's DIRECT launch, decided on the host from the batch, the mesh and the options (thresholds: tr_policy):
// XCD chunking, tiles, stealing, the unordered schedule's stealing, the 8-wide direct launch, block splitting.  Pure
// arithmetic: nothing is enqueued here (launch_direct does that, after sched_acquire has said whether an order exists).
struct direct_shape {
    int64_t nblocks;        // blocks of TR_BS rays of the block -> ray map
    int tile_w, steal_min;
    bool steal, usteal, use_wd, small_tris, can_tile8;
    tr_sort_params sort;    // ... as the sorter of the learned order takes them: XCD chunk, split blocks and their thresholds
    int steal_arg;
};
template <int Q, bool STATS>
direct_shape decide_direct_shape(const tr_bvh* bvh, const tr_device_state* st, const tr_options& opt, const RayFetch& rf,
                                 const batch_image& img, bool addr32) {
    constexpr bool pruning = Q == TR_Q_CLOSEST || Q == TR_Q_FIRST || Q == TR_Q_ANY;
    const int64_t nblocks_direct = (img.n_map + TR_BS - 1) / TR_BS;
    // chunk size of the XCD map: the option is in units of 256 rays; at least 4 chunks per XCD so that the XCDs' shares of
    // an uneven image stay comparable
    // (one XCD -- a CPX partition -- has ONE L2: nothing to keep local, the blocks run in plain order.  The learned order's eight
    // lists (launch slot j*8 + x) are then eight interleaved cost-sorted lists on the same XCD; on a device of 2 or 4 XCDs lists x
    // and x + 4 (x + 2, ...) share an XCD and a block still runs where its neighbours in the image run.)
    int xc = st->num_xcd > 1 ? opt.xcd_chunk * (256 / TR_BS) : 0;
    while (xc > 0 && (int64_t)xc * 32 > nblocks_direct) xc >>= 1;
    int tile_w = 0;
    // Image-shaped batches ([..., H, W, 3] with W % 8 == 0 and a multiple of 8 rows in total): a wave can take an 8x8 pixel
    // tile instead of 64 pixels of one row.  Tiles make the lanes of a wave more alike (12 % fewer wave-trips on the
    // headline image, +19 % at 16.7 M rays) but they also pack the expensive silhouette rays into waves whose 64 lanes all
    // stay active through hundreds of trips: the critical path of a small launch gets longer (-25 % at 1 M rays).  Hence,
    // on their own, tiles only from TILE_MIN_RAYS on; below that together with block splitting (further down), which takes
    // those waves apart (option tile: 0 never, 1 auto, 2 always).  Queries without distance pruning (count, location) have
    // no such critical path and take tiles at any size: C4 count 1.12 -> 0.93 ms (profiles/r02_sweep_c4.jsonl).
    const bool tile_any_size = opt.tile == 2 || !pruning;
    if (opt.tile && (tile_any_size || rf.n >= tr_policy::tile_min_rays(st)) && img.rows_tile8)
        tile_w = (int)rf.s2 | (3 << 28);
    // Smaller image-shaped batches of the pruning queries: flatter tiles where the triangles are large on screen (option
    // tile_small: 0 rows, 1 = 2x32, 2 = 4x16, 3 = 8x8, 4 = auto: 4x16 from 32 rays per triangle on, 2x32 from 8;
    // profiles/r02_sweep_tile_density.jsonl)
    if (opt.tile && !tile_w && opt.tile_small > 0 && rf.s1 > 1 && rf.s2 < (1 << 28)) {
        int lgh = opt.tile_small;
        if (lgh == 4) lgh = rf.n >= 32 * bvh->num_tris ? 2 : (rf.n >= 8 * bvh->num_tris ? 1 : 0);
        const int w = 64 >> lgh, h = 1 << lgh;
        if (lgh > 0 && rf.s2 % w == 0 && img.n_map % ((int64_t)h * rf.s2) == 0) tile_w = (int)rf.s2 | (lgh << 28);
    }
    // intra-wave work stealing (wave_traverse_steal).  steal = 1 (default): closest / first / any launches of up to
    // STEAL_MAX_RAYS, donors from their 64th trip on; steal >= 2 forces it on for them at any size, with that trip threshold
    const int steal_min = opt.steal > 1 ? opt.steal : tr_policy::STEAL_FROM_TRIP;
    const bool steal = !STATS && pruning && bvh->num_tris >= 2 && ((opt.steal == 1 && rf.n <= tr_policy::steal_max_rays(st)) || opt.steal > 1);
    // count / location: the unordered two-phase schedule (queued leaves, leaf phases by wave vote); count additionally hands
    // owed subtrees over between the lanes of a wave and takes split launch slots (usteal: 0 off, 1 on, >= 2 forced threshold)
    const bool usteal = Q == TR_Q_COUNT && !STATS && bvh->num_tris >= 2 && opt.usteal > 0;
    // The direct launch on the 8-wide compressed nodes (k_query_direct_wide): its own launch shape -- no stealing, no split
    // blocks, the plain learned order.  Option wide_direct: 0 never, 1 (default) where measured faster -- the multi-hit LIST
    // query (the one unordered query that does not steal) on meshes from WIDE_LIST_MIN_TRIS on --, 2 count and location
    // everywhere, 3 every query (closest / first / any lose 25...50 % without stealing and splitting)
    const bool wd_query = opt.wide_direct == 3 || (opt.wide_direct == 2 && !pruning) ||
                          (opt.wide_direct == 1 && Q == TR_Q_LOCATION && bvh->num_tris >= tr_policy::WIDE_LIST_MIN_TRIS);
    const bool use_wd = wd_query && addr32 && bvh->num_tris >= 2;
    // Block splitting: the most expensive blocks of the previous launch get two (the first quarter of them four) launch
    // slots of half / quarter lane density whose other lanes steal from trip split_steal on -- which is what makes 8x8 tiles
    // affordable below TILE_MIN_RAYS.  Launch shapes that steal only.  split: 0 off, 1 auto, N >= 2: nblocks >> N.
    const bool small_tris = rf.n >= 8 * bvh->num_tris;   // triangles of many pixels: flat tiles, balanced waves
    const bool can_tile8 = opt.tile && img.rows_tile8;
    int split_shift = 0;
    if ((steal || usteal) && opt.split > 1) split_shift = opt.split;
    else if ((steal || usteal) && opt.split == 1 && rf.n <= tr_policy::steal_max_rays(st)) {
        if (can_tile8 && !small_tris) split_shift = tr_policy::split_shift_tiled(nblocks_direct);
        // ... and HALF of them while the launch then still leaves three tenths of the chip's wave slots free
        // (profiles/r03_ab_split_half.txt)
        if (split_shift == 2) {
            const int64_t s1 = (nblocks_direct >> 1) / 8;
            if (2 * (nblocks_direct + 8 * (s1 + 2 * (s1 >> 2))) <= (int64_t)st->num_cus * 28 * 7 / 10) split_shift = 1;
        }
        else if (!can_tile8 && nblocks_direct <= 2048) split_shift = 4;
    }
    int64_t split = 0;
    if (use_wd) split_shift = 0;
    if (split_shift > 0 && nblocks_direct >= (opt.split > 1 ? 64 : tr_policy::SPLIT_MIN_BLOCKS)) split = (nblocks_direct >> split_shift) / 8;
    if (nblocks_direct + 12 * split > TR_SCHED_MAX || !opt.adaptive) split = 0;   // no learned order, no split
    int64_t split4 = split >> 2;
    int outlier8 = opt.split_outlier;       // 0 every block the grid has room for, 1 the rule, >= 2 eighths of the mean
    if (outlier8 == 1) outlier8 = tr_policy::outlier8(2.0 * (double)nblocks_direct / ((double)st->num_cus * 28.0));
    // trip thresholds: ordinary | split blocks; bit 15 (automatic policy only): a wave of unrelated rays starts at TR_STEAL_EARLY
    const int steal_arg = (steal_min & 0x7fff) | (opt.steal == 1 ? 0x8000 : 0) | (opt.split_steal << 16);
    // (the block count as the sorter takes it: above TR_SCHED_MAX blocks nothing is measured or sorted)
    const tr_sort_params sort = {(int)nblocks_direct, xc, (int)split, (int)split4, outlier8, opt.split_floor * 100};
    return direct_shape{nblocks_direct, tile_w, steal_min, steal, usteal, use_wd, small_tris, can_tile8, sort, steal_arg};
}

// Streaming launch with ray refill for large incoherent batches (option stream: 0 never, 1 auto, 2 always; returned alike).
// Auto: every batch of at least tr_policy::stream_min_rays rays gets BOTH launch shapes enqueued behind a coherence probe that
// selects one on the device (k_probe_coherence): a camera image -- flat or [H, W, 3] -- keeps the direct launch (and its 8x8
// tiles), a batch of unrelated rays takes the streaming launch whatever its tensor shape.  The multi-hit list query keeps
// the direct launch (its per-ray list pointer belongs to a launch slot).
int decide_streaming(const tr_bvh* bvh, const tr_device_state* st, const tr_options& opt, const RayFetch& rf, int query) {
    if (query == TR_Q_LOCATION) return 0;
    if (opt.stream == 2) return 2;
    return (opt.stream == 1 && rf.n >= tr_policy::stream_min_rays(st, query) && bvh->num_tris >= 2) ? 1 : 0;
}
// The coherence probe in front of both launch shapes; returns its verdict word (scratch[0]; it zeroes the work counter
// scratch[1] too), which both launches read at their first instruction.
const int* enqueue_probe(const tr_bvh* bvh, const RayFetch& rf, unsigned long long* scratch, hipStream_t stream) {
    int* d_sel = reinterpret_cast<int*>(scratch);
    float diag2 = 0.f;
    for (int k = 0; k < 3; k++) { const float e = bvh->aabb_max[k] - bvh->aabb_min[k]; diag2 += e * e; }
    hipLaunchKernelGGL(k_probe_coherence, dim3(1), dim3(256), 0, stream, rf, sqrtf(diag2), d_sel);
    return d_sel;
}

// The streaming launch of a batch (persistent waves, ray refill: kernels_stream.inc, traverse_wide.inc).  `sel` != NULL: behind
// the coherence probe, which selects between it and the direct launch on the device -- the direct launch is then enqueued
// behind it and returns at its first instruction unless the probe chose it.
template <int Q, bool STATS>
int launch_streaming(const tr_bvh* bvh, tr_device_state* st, const tr_options& opt, const tr_bvh_view& view, const RayFetch& rf,
                     const QueryOut& out, unsigned long long* d_stats, hipStream_t stream, bool addr32, bool compact,
                     bool deep, unsigned long long* scratch, const int* sel) {
    const int rpw = opt.stream_rays;
    // idle lanes that trigger a refill: option stream_refill, 0 (default) = by query -- the pruning-by-distance queries
    // want fuller waves before they pay a refill (28-32), any-hit and count, whose rays end or cost alike, refill sooner
    // (profiles/r05_retune_refill.txt: shard count 2.247 -> 2.122 ms, shard any 1.387 -> 1.344, C3 any 0.845 -> 0.814)
    const int refill_min = opt.stream_refill > 0 ? opt.stream_refill : ((Q == TR_Q_CLOSEST || Q == TR_Q_FIRST) ? tr_policy::REFILL_ORDERED : tr_policy::REFILL_UNORDERED);
    const int64_t nwaves = (rf.n + rpw - 1) / rpw;
    unsigned grid = (unsigned)((nwaves + 1) / 2);
    int sxc = (opt.xcd_chunk > 0 && st->num_xcd > 1) ? 16 : 0;       // blocks (2 ranges each) per XCD-local chunk
    while (sxc > 0 && (int64_t)sxc * 32 > grid) sxc >>= 1;
    // stream_dynamic (default): the ranges come from a work counter (the 2nd word of the probe's slot, zeroed by
    // the probe; memset when the launch is forced) and the grid is what can be resident -- the static map gives
    // every wave exactly one range
    unsigned long long* work = nullptr;
    if (opt.stream_dynamic) {
        work = scratch + 1;
        if (!sel) TR_HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned long long), stream));
        const unsigned resident = (unsigned)st->num_cus * 16u;
        if (grid > resident) grid = resident;
        sxc = 0;
    }
    bool wide_launched = false;
    if constexpr (!STATS) {
        // 8-wide compressed nodes (option wide: 0 never, 1 always, 2 where measured faster = tr_policy::WIDE_MIN_TRIS)
        const bool wide_auto = bvh->num_tris >= tr_policy::WIDE_MIN_TRIS && rf.n >= tr_policy::wide_min_rays(st);
        const tr_wnode* wn = ((opt.wide == 1 || (opt.wide == 2 && wide_auto)) && addr32) ? ensure_wide(bvh, stream) : nullptr;
        if (wn) {
            static std::atomic<int> wocc_a{0};   // per instantiation <Q>
            int wocc = wocc_a.load(std::memory_order_relaxed);
            if (wocc == 0) {
                int nb = 0;
                hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_query_wide<Q>, 128, 0);
                wocc = (e == hipSuccess && nb > 0) ? nb : 8;
                wocc_a.store(wocc, std::memory_order_relaxed);
            }
            unsigned wgrid = (unsigned)((nwaves + 1) / 2);
            if (work) { const unsigned resident = (unsigned)st->num_cus * (unsigned)wocc; if (wgrid > resident) wgrid = resident; }
            const wide_caps wc = wide_stack_caps(bvh, opt);
            int32_t* spill = wc.spill_cap > 0 ? wide_spill(bvh, stream, (size_t)wgrid * 128 * (size_t)wc.spill_cap) : nullptr;
            if (wc.spill_cap == 0 || spill) {
                hipLaunchKernelGGL((k_query_wide<Q>), dim3(wgrid), dim3(128), 0, stream, view, wn, rf, out, rpw,
                                   refill_min, sel, work, spill, wc.spill_cap, wc.lds_cap, d_stats);
                wide_launched = true;
            }
        }
    }
    if (!wide_launched) {
        if constexpr (STATS)
            hipLaunchKernelGGL((k_query_stream_stats<Q, false, 128>), dim3(grid), dim3(128), 0, stream, view, rf, out, rpw,
                               refill_min, sxc, d_stats, sel, work);
        else
            by_addressing(compact, deep, [&](auto c, auto d) {
                hipLaunchKernelGGL((k_query_stream<Q, decltype(c)::value, 128, decltype(d)::value>), dim3(grid), dim3(128), 0, stream,
                                   view, rf, out, rpw, refill_min, sxc, d_stats, sel, work);
            });
    }
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

// what tr_bvh_last_launch reports: the direct launch as it was enqueued (the handle has a sched_mutex)
template <int Q>
void record_last_launch(const tr_bvh* bvh, const RayFetch& rf, const direct_shape& sh, const sched_shape& run, int64_t nslots,
                        bool ordered, bool wd_launched, bool sort_carried, bool qn_used, int addressing) {
    constexpr bool unord = Q == TR_Q_COUNT || Q == TR_Q_LOCATION;
    tr_bvh* mb = const_cast<tr_bvh*>(bvh);
    std::lock_guard<std::mutex> lock(*mb->sched_mutex);
    tr_launch_info& li = mb->last_launch;
    li.rays = rf.n; li.blocks = sh.nblocks; li.slots = nslots; li.query = Q;
    li.shape = wd_launched ? 4 : (unord ? (sh.usteal ? 3 : 2) : (sh.steal ? 1 : 0));
    li.tile_rows_lg = run.lgh();
    li.split_blocks = ordered ? (int32_t)run.sort.split : 0;
    li.sort_carried = sort_carried ? 1 : 0;
    li.learned_order = ordered;
    li.grid_nodes = (qn_used || unord) && !wd_launched;
    li.addressing = addressing;
    mb->have_last_launch = true;
}

// The direct launch of a batch: its shape (decide_direct_shape), what the learned order grants it (sched_acquire), then
// the kernel -- every family is named in one launch statement below.  `sel`: the coherence probe's verdict when the
// streaming launch is enqueued beside it (NULL: none).
template <int Q, bool STATS>
int launch_direct(const tr_bvh* bvh, const tr_device_state* st, const tr_options& opt, const tr_bvh_view& view, const RayFetch& rf,
                  const batch_image& img, const QueryOut& out, unsigned long long* d_stats, hipStream_t stream,
                  bool addr32, bool compact, bool deep, const int* sel) {
    constexpr bool pruning = Q == TR_Q_CLOSEST || Q == TR_Q_FIRST || Q == TR_Q_ANY;      // queries that end or prune by distance
    constexpr bool unord = !pruning;
    const direct_shape sh = decide_direct_shape<Q, STATS>(bvh, st, opt, rf, img, addr32);
    // The shape the launch takes once the (handle, stream) has an order for it (`want`): with split blocks the pruning queries
    // take 8x8 tiles at any size.  The first launch of a batch shape (`plain`) runs without split slots in the tile shape
    // chosen so far.
    sched_shape want = {img.w, img.h, sh.tile_w, sh.sort};
    if (sh.sort.split > 0 && sh.can_tile8 && !sh.small_tris && opt.tile_small == 4) want.tile_w = (int)rf.s2 | (3 << 28);
    sched_shape plain = want;
    if (opt.order_transfer) { plain.tile_w = sh.tile_w; plain.sort.split = 0; plain.sort.split4 = 0; }
    // (the kernel flavours with the sorter workgroup: the stealing launch on the grid nodes and the stealing count launch, with
    // 32-bit addressing, not behind the coherence probe)
    const bool can_carry = !STATS && addr32 && !sh.use_wd && sel == nullptr &&
                           ((sh.steal && pruning && opt.grid_nodes > 0) || (Q == TR_Q_COUNT && sh.usteal));
    sched_grant g;      // (the instrumented launches take no part in the learned order: the plain shape, which is theirs anyway)
    if constexpr (!STATS) g = sched_acquire(bvh, opt, stream, sh.nblocks, want, plain, can_carry);
    const sched_shape& run = g.plain ? plain : want;
    const int xc = sh.sort.xc, tile_w = run.tile_w, split_key = run.sort.split;
    const int64_t nslots = sh.nblocks + (g.order ? 8 * ((int64_t)run.sort.split + 2 * run.sort.split4) : 0);
    // launches without an order visit every XCD's blocks in a scrambled order (k -> k * P mod count, P prime): an expensive
    // image region is spread over the launch instead of being started last
    int scramble = 0;
    if (xc > 0) {
        const int64_t cnt = sh.nblocks / (8 * (int64_t)xc) * xc;   // blocks per XCD in whole spans
        for (int p : {7919, 7907, 7901})
            if (cnt > 1 && cnt % p != 0) { scramble = p; break; }
    }
    // Node flavour of the stealing closest / first launches: the 32-byte grid nodes (two gathers per visit, the fused box
    // test of round 5) wherever their 32-bit addressing exists; option grid_nodes = 0 keeps the exact 64-byte nodes.  (Until
    // round 5 the library MEASURED both flavours per batch shape -- 16 events, alternating launches --: with the fused test
    // the grid nodes win or tie on every scene, headline 0.212 -> 0.186 ms, C4 0.163 -> 0.144, C2 0.136 -> 0.128, terrain
    // 0.147 -> 0.139, the cloud 0.253 -> 0.220, the interior scene 0.035 = 0.035: profiles/r05_node_flavour.txt.)
    // Any-hit, which kept the exact nodes through round 4 (-3 % on the grid nodes then), gains too: headline any 0.164 -> 0.148,
    // C4 0.140 -> 0.127, terrain 0.122 -> 0.111, C2 equal, the interior scene 0.030 -> 0.032 (profiles/r05_any_flavour.txt).
    const bool qn_used = sh.steal && pruning && addr32 && opt.grid_nodes > 0;
    const int addressing = compact ? 1 : (deep ? 2 : 0);        // as tr_launch_info reports it
    static const bool debug_launch = getenv("TRIRO_DEBUG_LAUNCH") != nullptr;
    if (debug_launch)
        fprintf(stderr, "[triro] query %d: rays %lld blocks %lld slots %lld tile 0x%x split %lld order %d cost %d sort: carried %d behind %d steal %d usteal %d grid nodes %d addressing %d\n",
                Q, (long long)rf.n, (long long)sh.nblocks, (long long)nslots, (unsigned)tile_w, (long long)run.sort.split,
                g.order != nullptr, g.cost != nullptr, g.job.cost != nullptr, g.order_out != nullptr, (int)sh.steal, (int)sh.usteal,
                (int)qn_used, addressing);
    const dim3 grid((unsigned)nslots), grid_sort((unsigned)nslots + 8u);    // (the sorter workgroup: eight slots more in front)
    bool wd_launched = false, sort_carried = false;
    // k_query_direct, not instrumented.  mode: 0 plain / 1 stealing / 2 the unordered schedule; qn: on the grid nodes
    auto direct = [&](auto mode, auto qn, int arg) {
        by_addressing(compact, deep, [&](auto c, auto d) {
            constexpr bool C = decltype(c)::value, D = decltype(d)::value, QN = decltype(qn)::value;
            // generic addressing has no grid-node flavour (qn_used: 32-bit offsets only)
            if constexpr (C || !QN)
                hipLaunchKernelGGL((k_query_direct<Q, false, C, decltype(mode)::value, D, QN>), grid, dim3(TR_BS), 0, stream, view, rf, out,
                                   xc, scramble, tile_w, arg, g.order, split_key, g.cost, d_stats, sel);
        });
    };
    if constexpr (STATS) {
        // the instrumented launch: generic addressing only; plain shape (pruning queries) / unordered schedule (count, location)
        hipLaunchKernelGGL((k_query_direct<Q, true, false, unord ? 2 : 0, false, false>), grid, dim3(TR_BS), 0, stream, view, rf, out,
                           xc, scramble, tile_w, unord ? opt.leaf_vote : sh.steal_min, g.order, split_key, g.cost, d_stats, sel);
    } else {
        const tr_wnode* wn = sh.use_wd ? ensure_wide(bvh, stream) : nullptr;
        if (wn) {
            const wide_caps wc = wide_stack_caps(bvh, opt);
            // (one spill row per lane of the GRID: above 1 GiB -- tens of millions of rays on a deep hierarchy -- the launch
            // keeps the binary shapes, whose state needs no memory)
            const size_t spill_elems = (size_t)nslots * 128 * (size_t)wc.spill_cap;
            int32_t* spill = (wc.spill_cap > 0 && spill_elems <= ((size_t)1 << 28)) ? wide_spill(bvh, stream, spill_elems) : nullptr;
            if (wc.spill_cap == 0 || spill) {
                const tr_wide_args wa = {wn, spill, wc.spill_cap, wc.lds_cap};
                hipLaunchKernelGGL((k_query_direct_wide<Q>), grid, dim3(128), 0, stream, view, rf, out,
                                   xc, scramble, tile_w, g.order, split_key, g.cost, d_stats, sel, wa);
                wd_launched = true;
            }
        }
        if (wd_launched) {
        } else if constexpr (unord) {
            if (sh.usteal) {
                if constexpr (Q == TR_Q_COUNT) {
                    // leaf vote | trip threshold of ordinary blocks | of split blocks
                    const int us_min = opt.usteal > 1 ? opt.usteal : tr_policy::USTEAL_FROM_TRIP;
                    const int uarg = (opt.leaf_vote & 0xff) | ((us_min & 0xfff) << 8) | ((opt.split_steal & 0xfff) << 20);
                    // (the launch that carries the deferred sort never measures: sched_measure)
                    sort_carried = g.job.cost && !g.cost && g.order && addr32;
                    if (sort_carried)
                        by_addressing(compact, deep, [&](auto c, auto d) {
                            if constexpr (decltype(c)::value)       // the sort-carrying kernels have no generic flavour
                                hipLaunchKernelGGL((k_query_count_steal_sort<decltype(d)::value>), grid_sort, dim3(TR_BS), 0, stream,
                                                   view, rf, out, xc, scramble, tile_w, uarg, g.order, split_key, d_stats, g.job);
                        });
                    else
                        by_addressing(compact, deep, [&](auto c, auto d) {
                            hipLaunchKernelGGL((k_query_count_steal<decltype(c)::value, decltype(d)::value>), grid, dim3(TR_BS), 0, stream,
                                               view, rf, out, xc, scramble, tile_w, uarg, g.order, split_key, g.cost, d_stats, sel);
                        });
                }
            } else {
                direct(tr_mode<2>{}, std::false_type{}, opt.leaf_vote);
            }
        } else if (qn_used) {       // (stealing on the grid nodes)
            sort_carried = g.job.cost && !g.cost && g.order;
            if (sort_carried)
                by_addressing(compact, deep, [&](auto c, auto d) {
                    if constexpr (decltype(c)::value)           // the sort-carrying kernels have no generic flavour
                        hipLaunchKernelGGL((k_query_direct_sort<Q, decltype(d)::value>), grid_sort, dim3(TR_BS), 0, stream,
                                           view, rf, out, xc, scramble, tile_w, sh.steal_arg, g.order, split_key, d_stats, g.job);
                });
            else
                direct(tr_mode<1>{}, std::true_type{}, sh.steal_arg);
        } else if (sh.steal) {
            direct(tr_mode<1>{}, std::false_type{}, sh.steal_arg);
        } else {
            // the plain shape: coherent batches above STEAL_MAX_RAYS (wave-uniform trips fetch their node by the scalar unit)
            direct(tr_mode<0>{}, std::false_type{}, sh.steal_min);
        }
    }
    if (g.job.cost && !sort_carried) {
        // (cannot happen: sched_acquire hands a job only to a launch of the flavour that carries it) -- the sort as a kernel
        const tr_sort_job& j = g.job;
        enqueue_sort(stream, j.cost, j.order, tr_sort_params{j.nblocks, j.xcd_map, j.split, j.split4, j.outlier8, j.floor_ticks}, nullptr, j.prev);
    }
    if (g.cost && g.order_out) enqueue_sort(stream, g.cost, g.order_out, run.sort, sel, g.cost + TR_SCHED_PREV);
    if (!STATS && bvh->sched_mutex) record_last_launch<Q>(bvh, rf, sh, run, nslots, g.order != nullptr, wd_launched, sort_carried, qn_used, addressing);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

template <int Q, bool STATS>
int launch_query(const tr_bvh* bvh, const tr_rays* rays, const QueryOut& out,
                 unsigned long long* d_stats, hipStream_t stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    RayFetch rf;
    TR_TRY(make_fetch(rays, &rf));
    if (rf.n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(enter_bvh_device(bvh, rays, &guard));
    tr_device_state* st;
    TR_TRY(tr_get_device_state(bvh->device, &st));
    tr_policy_units(st);
    const tr_bvh_view view = tr_view_of(bvh);
    const tr_options opt = tr_opts();   // one snapshot per call
    // 32-bit offsets when both arrays are below 4 GiB; 32-bit trail words when the hierarchy is at most 32 levels high
    // (`compact` = both, `deep` = offsets only).  The instrumented launches (STATS) exist in the generic addressing only.
    const bool addr32 = !STATS && opt.compact && bvh->num_nodes * (int64_t)sizeof(tr_node) < ((int64_t)1 << 32) &&
                        bvh->num_tris * (int64_t)sizeof(tr_tri) < ((int64_t)1 << 32);
    const bool compact = addr32 && bvh->depth <= 32;
    const bool deep = addr32 && !compact;
    const int* sel = nullptr;
    if constexpr (Q != TR_Q_LOCATION) {
        const int streaming = decide_streaming(bvh, st, opt, rf, Q);
        if (streaming) {
            unsigned long long* scratch = stream_scratch(bvh, st, stream);
            if (streaming == 1) sel = enqueue_probe(bvh, rf, scratch, stream);
            TR_TRY((launch_streaming<Q, STATS>(bvh, st, opt, view, rf, out, d_stats, stream, addr32, compact, deep, scratch, sel)));
            if (!sel) return TR_OK;     // the batch is taken care of
        }
    }
    return launch_direct<Q, STATS>(bvh, st, opt, view, rf, batch_image(rf), out, d_stats, stream, addr32, compact, deep, sel);
}

template <typename T>
int scan_impl(const T* d_in, int64_t n, int32_t cap, int64_t* d_offsets, int64_t* d_total,
              int64_t* h_total, hipStream_t stream) {
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    if (!d_total) return tr_fail(TR_ERR_INVALID_ARG, "d_total == NULL");
    if (n > 0 && (!d_in || !d_offsets)) return tr_fail(TR_ERR_INVALID_ARG, "null scan pointer");
    int dev = 0;
    TR_HIP_TRY(hipGetDevice(&dev));
    tr_device_state* st;
    TR_TRY(tr_get_device_state(dev, &st));
    if (n == 0) {
        TR_HIP_TRY(hipMemsetAsync(d_total, 0, sizeof(int64_t), stream));
    } else {
        int64_t nblocks = (n + SCAN_TILE - 1) / SCAN_TILE;
        // block partials: a stream-ordered allocation, so scans enqueued on different streams
        // (or from different host threads) never share scratch and nothing synchronises
        int64_t* partial = nullptr;
        const size_t bytes = sizeof(int64_t) * (size_t)nblocks;
        bool pooled = hipMallocAsync((void**)&partial, bytes, stream) == hipSuccess;
        if (!pooled) {
            (void)hipGetLastError();
            TR_HIP_TRY(hipMalloc((void**)&partial, bytes));
        }
        hipLaunchKernelGGL((k_scan_partial<T>), dim3((unsigned)nblocks), dim3(SCAN_BLOCK), 0, stream, d_in, n, cap, partial);
        hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(SCAN_BLOCK), 0, stream, partial, nblocks, d_total);
        hipLaunchKernelGGL((k_scan_final<T>), dim3((unsigned)nblocks), dim3(SCAN_BLOCK), 0, stream, d_in, n, cap, partial, d_offsets);
        hipError_t le = hipGetLastError();
        if (pooled) {
            hipError_t fe = hipFreeAsync(partial, stream);
            if (le == hipSuccess) le = fe;
        } else {
            (void)hipStreamSynchronize(stream);   // no stream-ordered allocator: free after the work
            (void)hipFree(partial);
        }
        TR_HIP_TRY(le);
    }
    if (h_total) {
        TR_HIP_TRY(hipMemcpyAsync(h_total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        TR_HIP_TRY(hipStreamSynchronize(stream));
    }
    return TR_OK;
}

// ---- 8-wide nodes: construction on first use (traverse_wide.inc) ----------------------------------------------
const tr_wnode* ensure_wide(const tr_bvh* cbvh, hipStream_t stream) {
    tr_bvh* bvh = const_cast<tr_bvh*>(cbvh);
    if (!bvh->sched_mutex || bvh->num_nodes < 1 || bvh->num_tris < 2) return nullptr;
    std::lock_guard<std::mutex> lock(*bvh->sched_mutex);
    if (bvh->wide_valid) {
        if (stream != bvh->wide_stream && bvh->wide_event) (void)hipStreamWaitEvent(stream, bvh->wide_event, 0);
        return bvh->wnodes;
    }
    // (ADVICE r04: a hierarchy whose wide nodes cannot be built -- 4 GiB of records and more, no memory -- used to run
    // the marking rounds and a synchronising scan again behind EVERY streaming query; one failed attempt per build now)
    if (bvh->wide_unavailable) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return nullptr; }
    struct mark_failed { tr_bvh* b; bool ok = false; ~mark_failed() { if (!ok) b->wide_unavailable = true; } } outcome{bvh};
    const int64_t n = bvh->num_nodes;
    if (bvh->wtmp_cap < n) {
        if (bvh->wflag) (void)hipFree(bvh->wflag);
        if (bvh->widx) (void)hipFree(bvh->widx);
        bvh->wflag = nullptr; bvh->widx = nullptr; bvh->wtmp_cap = 0;
        if (hipMalloc((void**)&bvh->wflag, (size_t)n) != hipSuccess || hipMalloc((void**)&bvh->widx, sizeof(int64_t) * (size_t)(n + 1)) != hipSuccess) {
            (void)hipGetLastError();
            if (bvh->wflag) { (void)hipFree(bvh->wflag); bvh->wflag = nullptr; }
            return nullptr;
        }
        bvh->wtmp_cap = n;
    }
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const int rounds = (bvh->depth + 2) / 3 + 1;
    for (int r = 0; r <= rounds; r++)
        hipLaunchKernelGGL(k_wide_mark, dim3(blocks), dim3(256), 0, stream, bvh->nodes, n, bvh->wflag, r);
    int64_t nw = 0;
    if (scan_impl<uint8_t>(bvh->wflag, n, 1, bvh->widx, bvh->widx + n, &nw, stream) != TR_OK || nw < 1) return nullptr;
    if (nw * (int64_t)sizeof(tr_wnode) >= ((int64_t)1 << 32)) return nullptr;      // 32-bit offsets in the kernel
    if (bvh->wcap < nw) {
        if (bvh->wnodes) (void)hipFree(bvh->wnodes);
        bvh->wnodes = nullptr; bvh->wcap = 0;
        if (hipMalloc((void**)&bvh->wnodes, sizeof(tr_wnode) * (size_t)nw) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        bvh->wcap = nw;
    }
    hipLaunchKernelGGL(k_wide_emit, dim3(blocks), dim3(256), 0, stream, bvh->nodes, n, bvh->wflag, bvh->widx, bvh->wnodes);
    if (hipGetLastError() != hipSuccess) return nullptr;
    if (!bvh->wide_event && hipEventCreateWithFlags(&bvh->wide_event, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); bvh->wide_event = nullptr; }
    if (bvh->wide_event) (void)hipEventRecord(bvh->wide_event, stream);
    else (void)hipStreamSynchronize(stream);
    bvh->wide_stream = stream;
    bvh->wcount = nw;
    bvh->wide_valid = true;
    outcome.ok = true;
    return bvh->wnodes;
}

int32_t* wide_spill(const tr_bvh* cbvh, hipStream_t stream, size_t elems) {
    tr_bvh* bvh = const_cast<tr_bvh*>(cbvh);
    if (!bvh->sched_mutex) return nullptr;
    std::lock_guard<std::mutex> lock(*bvh->sched_mutex);
    tr_sched_slot* slot = sched_slot(bvh, stream, 0);
    if (!slot) return nullptr;
    if (slot->wspill_elems < elems) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return nullptr; }
        if (slot->wspill) { (void)hipStreamSynchronize(stream); (void)hipFree(slot->wspill); slot->wspill = nullptr; slot->wspill_elems = 0; }
        if (hipMalloc((void**)&slot->wspill, elems * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        slot->wspill_elems = elems;
    }
    return slot->wspill;
}
