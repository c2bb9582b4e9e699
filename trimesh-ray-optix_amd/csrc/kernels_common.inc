// kernels_common.inc -- included by traverse.hip inside its anonymous namespace: what every launch shape shares -- the
// per-call ABI of the kernels (RayFetch = the reference's RayInput marshaling, LaunchParams.h:11-28; QueryOut), the
// strided ray fetch (shaders.cu:27-63), the result writer (shaders.cu:120-172 and friends), the single-triangle
// fallback and the counters of the instrumented launches.
struct RayFetch {
    const float* o;
    const float* d;
    int64_t n;
    int64_t s0, s1, s2;   // leading dims (right-aligned; unused = INT64_MAX)
    int64_t os[4], ds[4]; // element strides
    int omode, dmode;     // 0 dense [n,3], 1 broadcast (all leading strides 0), 2 general
    // the frame rays are anchored to (tr_ray_anchor_q), for the kernels that have no tr_bvh_view: tr_closest_from_slots
    // (device memory, read when the kernel runs: a graph replay sees the frame of a later refit); NULL = no anchoring
    const tr_qframe* aframe;
};

struct QueryOut {
    uint8_t* hit;
    uint8_t* front;
    int32_t* tri;
    float* loc;
    float* uv;
    int32_t* count;
    tr_hit_entry* hits;   // TR_Q_LOCATION: [n, cap] unsorted nearest hits (tr_topk<0>)
    int32_t cap;
    tr_packed_hit* packed;   // TR_Q_CLOSEST: when set, 12 bytes per ray instead of the five arrays
    int packed_slots;        // ... with the arena slot of the triangle instead of its face index (tr_intersects_closest_packed_slots)
};

// tr_rays -> RayFetch (host): the shape checks and the stride class of each tensor, for every entry that takes rays
int make_fetch(const tr_rays* rays, RayFetch* rf) {
    if (!rays) return tr_fail(TR_ERR_INVALID_ARG, "rays == NULL");
    if (rays->nray < 0) return tr_fail(TR_ERR_INVALID_ARG, "nray < 0");
    if (rays->shape[3] != 3) return tr_fail(TR_ERR_INVALID_ARG, "last ray dimension must be 3");
    int64_t prod = 1;
    for (int k = 0; k < 3; k++) {
        int64_t s = rays->shape[k];
        if (s == INT64_MAX) continue;
        if (s < 0) return tr_fail(TR_ERR_INVALID_ARG, "negative ray dimension");
        prod *= s;
    }
    if (prod != rays->nray) return tr_fail(TR_ERR_INVALID_ARG, "nray != product of leading dims");
    if (rays->nray > 0 && (!rays->d_origins || !rays->d_directions))
        return tr_fail(TR_ERR_INVALID_ARG, "null ray pointer");
    rf->o = rays->d_origins; rf->d = rays->d_directions; rf->n = rays->nray;
    rf->s0 = rays->shape[0]; rf->s1 = rays->shape[1]; rf->s2 = rays->shape[2];
    auto classify = [&](const int64_t* st) {
        bool bcast = true, dense = st[3] == 1;
        int64_t expect = 3;
        for (int k = 2; k >= 0; k--) {
            int64_t s = rays->shape[k];
            if (s == INT64_MAX || s == 1) continue;
            if (st[k] != 0) bcast = false;
            if (st[k] != expect) dense = false;
            expect *= s;
        }
        return dense ? 0 : (bcast ? 1 : 2);
    };
    for (int k = 0; k < 4; k++) { rf->os[k] = rays->ostride[k]; rf->ds[k] = rays->dstride[k]; }
    rf->omode = classify(rays->ostride);
    rf->dmode = classify(rays->dstride);
    rf->aframe = nullptr;      // no anchoring unless a caller sets the frame (tr_closest_from_slots)
    if (rf->s0 == INT64_MAX) rf->s0 = 1;   // keep the general path's divisions cheap and safe
    if (rf->s1 == INT64_MAX) rf->s1 = 1;
    if (rf->s2 == INT64_MAX) rf->s2 = 1;
    if (rf->s0 == 0 || rf->s1 == 0 || rf->s2 == 0) { rf->s0 = rf->s1 = rf->s2 = 1; }
    return TR_OK;
}

// strided fetch of ray `idx`: the reference's getRay/getIndices (shaders.cu:27-63) with
// 64-bit index math and fast paths for dense and broadcast tensors
__device__ __forceinline__ void fetch_ray(const RayFetch& rf, int64_t idx, float* o, float* d) {
    int64_t i0 = 0, i1 = 0, i2 = 0;
    if (rf.omode == 2 || rf.dmode == 2) {
        uint64_t r = (uint64_t)idx;
        i2 = (int64_t)(r % (uint64_t)rf.s2); r /= (uint64_t)rf.s2;
        i1 = (int64_t)(r % (uint64_t)rf.s1); r /= (uint64_t)rf.s1;
        i0 = (int64_t)(r % (uint64_t)rf.s0);
    }
    {
        int64_t off, s3 = rf.os[3];
        if (rf.omode == 0) { off = idx * 3; s3 = 1; }
        else if (rf.omode == 1) off = 0;
        else off = i0 * rf.os[0] + i1 * rf.os[1] + i2 * rf.os[2];
        o[0] = rf.o[off]; o[1] = rf.o[off + s3]; o[2] = rf.o[off + 2 * s3];
    }
    {
        int64_t off, s3 = rf.ds[3];
        if (rf.dmode == 0) { off = idx * 3; s3 = 1; }
        else if (rf.dmode == 1) off = 0;
        else off = i0 * rf.ds[0] + i1 * rf.ds[1] + i2 * rf.ds[2];
        d[0] = rf.d[off]; d[1] = rf.d[off + s3]; d[2] = rf.d[off + 2 * s3];
    }
}

template <int Q>
__device__ __forceinline__ void write_result(const tr_bvh_view& b, const QueryOut& out, int64_t i,
                                             const tr_ray& r, const tr_result& res) {
    if (Q == TR_Q_ANY) {
        out.hit[i] = res.best_face >= 0 ? 1 : 0;
    } else if (Q == TR_Q_FIRST) {
        out.tri[i] = res.best_face;
    } else if (Q == TR_Q_COUNT || Q == TR_Q_LOCATION) {
        out.count[i] = res.count;
    } else if (Q == TR_Q_CLOSEST) {
        float loc[3] = {0.f, 0.f, 0.f}, uv[2] = {0.f, 0.f};
        uint8_t hit = 0, front = 0;
        if (out.packed && out.packed_slots == 2) {      // tr_intersects_closest_slots: the slot and nothing else
            reinterpret_cast<int32_t*>(out.packed)[i] = res.best_face >= 0 ? res.best_slot : -1;
            return;
        }
        if (out.packed) {
            // packed form (tr_intersects_closest_packed): {face | front << 30, u, v}; tr_closest_expand
            // applies tr_bary_outputs to the same (u, v) and the same vertices -> the same bits
            tr_packed_hit ph = {0xffffffffu, 0.f, 0.f};
            if (res.best_face >= 0) {
                tr_counters* nc = nullptr;
                tr_tri t = tr_load_tri<false>(b, res.best_slot, nc);
                bool fr;
                tr_tri_bary(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, ph.w0, ph.w1, fr);
                ph.tri = (uint32_t)(out.packed_slots ? res.best_slot : res.best_face) | (fr ? 0x40000000u : 0u);
            }
            out.packed[i] = ph;
            return;
        }
        if (res.best_face >= 0) {
            tr_counters* nc = nullptr;
            tr_tri t = tr_load_tri<false>(b, res.best_slot, nc);
            // the barycentrics of the WINNING triangle from the float64 edge functions (tr_tri_bary): nothing but
            // (distance, face, slot) is carried through the traversal loop
            const bool fr = tr_hit_outputs(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, loc, uv);
            hit = 1; front = fr ? 1 : 0;
        }
        out.hit[i] = hit;
        out.front[i] = front;
        out.tri[i] = res.best_face;
        out.loc[3 * i] = loc[0]; out.loc[3 * i + 1] = loc[1]; out.loc[3 * i + 2] = loc[2];
        out.uv[2 * i] = uv[0]; out.uv[2 * i + 1] = uv[1];
    }
}

// single-triangle / empty meshes: no hierarchy exists; evaluate the predicate directly
template <int Q>
__device__ __forceinline__ void brute_one(const tr_bvh_view& b, const tr_ray& r, bool valid,
                                          tr_result& res) {
    tr_set_best_t(res, TR_TMAX); res.best_face = -1; res.best_slot = -1;
    res.count = 0;
    if (!valid || b.num_tris < 1) return;
    tr_counters* nc = nullptr;
    tr_tri t = tr_load_tri<false>(b, 0, nc);
    tr_hit h;
    if (tr_tri_test(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, h)) {
        tr_set_best_t(res, h.t); res.best_face = t.face; res.best_slot = 0;
        res.count = 1;
    }
}

template <bool STATS>
__device__ __forceinline__ void flush_stats(const tr_counters& c, unsigned long long* stats) {
    if (!STATS) return;
    unsigned long long a = c.nodes, t = c.tris, k = c.climbs;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off); t += __shfl_xor(t, off); k += __shfl_xor(k, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&stats[1], a); atomicAdd(&stats[2], t); atomicAdd(&stats[3], k);
    }
}
