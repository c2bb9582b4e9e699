// abi.inc -- included by traverse.hip: the query entry points of the C ABI (include/triro_hip.h), thin wrappers over
// launch_query and the list / expansion kernels.  Replaces the launch wrappers of ray.cpp:161-378.
extern "C" {

int tr_intersects_any(const tr_bvh* bvh, const tr_rays* rays, uint8_t* d_hit, void* stream) {
    if (!d_hit && rays && rays->nray > 0) return tr_fail(TR_ERR_INVALID_ARG, "d_hit == NULL");
    QueryOut out = {d_hit, nullptr, nullptr, nullptr, nullptr, nullptr};
    return launch_query<TR_Q_ANY, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

int tr_intersects_first(const tr_bvh* bvh, const tr_rays* rays, int32_t* d_tri, void* stream) {
    if (!d_tri && rays && rays->nray > 0) return tr_fail(TR_ERR_INVALID_ARG, "d_tri == NULL");
    QueryOut out = {nullptr, nullptr, d_tri, nullptr, nullptr, nullptr};
    return launch_query<TR_Q_FIRST, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

int tr_intersects_closest(const tr_bvh* bvh, const tr_rays* rays, uint8_t* d_hit, uint8_t* d_front,
                          int32_t* d_tri, float* d_loc, float* d_uv, void* stream) {
    if (rays && rays->nray > 0 && (!d_hit || !d_front || !d_tri || !d_loc || !d_uv))
        return tr_fail(TR_ERR_INVALID_ARG, "null output pointer");
    QueryOut out = {d_hit, d_front, d_tri, d_loc, d_uv, nullptr};
    return launch_query<TR_Q_CLOSEST, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

int tr_intersects_closest_packed(const tr_bvh* bvh, const tr_rays* rays, tr_packed_hit* d_packed, void* stream) {
    if (rays && rays->nray > 0 && !d_packed) return tr_fail(TR_ERR_INVALID_ARG, "d_packed == NULL");
    if (bvh && bvh->num_tris >= ((int64_t)1 << 30)) return tr_fail(TR_ERR_INVALID_ARG, "packed results hold face indices below 2^30");
    QueryOut out = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, d_packed};
    return launch_query<TR_Q_CLOSEST, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

int tr_closest_expand(const tr_packed_hit* d_packed, int64_t n, const float* d_vertices, int64_t nv,
                      const int32_t* d_faces, int64_t nf, uint8_t* d_hit, uint8_t* d_front, int32_t* d_tri,
                      float* d_loc, float* d_uv, void* stream) {
    if (n < 0 || nv < 0 || nf < 0) return tr_fail(TR_ERR_INVALID_ARG, "negative size");
    if (n == 0) return TR_OK;
    if (!d_packed) return tr_fail(TR_ERR_INVALID_ARG, "d_packed == NULL");
    if (nf > 0 && (!d_vertices || !d_faces)) return tr_fail(TR_ERR_INVALID_ARG, "null mesh pointer");
    // four rays per thread, 256 apart, the mesh rows through buffer loads (a miss fetches nothing); small batches and meshes
    // beyond the 2 GiB a buffer descriptor addresses: one ray per thread
    const bool buf_ok = nf * 12 < ((int64_t)1 << 31) && nv * 12 < ((int64_t)1 << 31) && nf > 0 && nv > 0;
    if (n >= 4096 && buf_ok) {
        int64_t blocks = (n + 1023) / 1024;
        const tr_options o2 = tr_opts();
        if (o2.expand_cus > 0) {
            int dev = 0;
            tr_device_state* st = nullptr;
            if (hipGetDevice(&dev) == hipSuccess && tr_get_device_state(dev, &st) == TR_OK && blocks > (int64_t)st->num_cus * o2.expand_cus)
                blocks = (int64_t)st->num_cus * o2.expand_cus;
        }
        hipLaunchKernelGGL(k_closest_expand_buf<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           d_packed, n, d_vertices, nv, d_faces, nf, d_hit, d_front, d_tri, d_loc, d_uv);
    } else {
        hipLaunchKernelGGL(k_closest_expand<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           d_packed, n, d_vertices, nv, d_faces, nf, d_hit, d_front, d_tri, d_loc, d_uv);
    }
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

int tr_intersects_closest_packed_slots(const tr_bvh* bvh, const tr_rays* rays, tr_packed_hit* d_packed, void* stream) {
    if (rays && rays->nray > 0 && !d_packed) return tr_fail(TR_ERR_INVALID_ARG, "d_packed == NULL");
    if (bvh && bvh->num_tris >= ((int64_t)1 << 30)) return tr_fail(TR_ERR_INVALID_ARG, "packed results hold triangle slots below 2^30");
    QueryOut out = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, d_packed, 1};
    return launch_query<TR_Q_CLOSEST, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

extern "C++" {
template <bool RAYS>
static int expand_slots_impl(const tr_bvh* bvh, const void* d_rec, int64_t n, int64_t row_length, const RayFetch& rf_in, uint8_t* d_hit,
                             uint8_t* d_front, int32_t* d_tri, float* d_loc, float* d_uv, void* stream) {
    RayFetch rf = rf_in;
    rf.aframe = bvh->frame_dev;      // the frame the trace anchored its rays to (tr_ray_anchor_q)
    if (bvh->num_tris * (int64_t)sizeof(tr_tri) >= ((int64_t)1 << 31)) return tr_fail(TR_ERR_INVALID_ARG, "slot form needs a triangle array below 2 GiB");
    tr_device_state* st;
    TR_TRY(tr_get_device_state(bvh->device, &st));
    const tr_options opt = tr_opts();
    // image-shaped rows (row_length pixels each): blocks of 8 rows x 32 pixels per wave, so that the rays that share a
    // triangle record share a wave (option expand_tiles).  A row count that is not a multiple of 8 leaves the last row
    // of blocks partly empty: taken from 64 rows on.
    const bool tiled = opt.expand_tiles && row_length >= 32 && row_length % 32 == 0 && n % row_length == 0 && n >= 4096 &&
                       (n % (8 * row_length) == 0 || n >= 64 * row_length);
    if (tiled) {
        const int64_t n_map = (n / row_length + 7) / 8 * 8 * row_length;
        int64_t blocks = (n_map / 256 + 3) / 4;               // 4 waves per workgroup, one block of 8 x 32 pixels per wave and pass
        // one wave per block of 8 rows x 32 pixels (expand_cus = N > 0: at most N workgroups per CU, the waves loop;
        // measured on 7.3 M records of the headline image: no cap 0.066 ms, 8 per CU 0.072, what is resident 0.078)
        if (opt.expand_cus > 0 && blocks > (int64_t)st->num_cus * opt.expand_cus) blocks = (int64_t)st->num_cus * opt.expand_cus;
        if (n_map == n)
            hipLaunchKernelGGL((k_closest_expand_slots_tiled<RAYS, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                               d_rec, n, row_length, bvh->tris, bvh->num_tris, d_hit, d_front, d_tri, d_loc, d_uv, rf);
        else
            hipLaunchKernelGGL((k_closest_expand_slots_tiled<RAYS, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                               d_rec, n, row_length, bvh->tris, bvh->num_tris, d_hit, d_front, d_tri, d_loc, d_uv, rf);
    } else if (n >= 4096) {
        int64_t blocks = (n + 1023) / 1024;
        if (opt.expand_cus > 0 && blocks > (int64_t)st->num_cus * opt.expand_cus) blocks = (int64_t)st->num_cus * opt.expand_cus;
        hipLaunchKernelGGL((k_closest_expand_slots<4, RAYS>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           d_rec, n, bvh->tris, bvh->num_tris, d_hit, d_front, d_tri, d_loc, d_uv, rf);
    } else {
        hipLaunchKernelGGL((k_closest_expand_slots<1, RAYS>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           d_rec, n, bvh->tris, bvh->num_tris, d_hit, d_front, d_tri, d_loc, d_uv, rf);
    }
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}
}   // extern "C++"

int tr_closest_expand_slots_rows(const tr_bvh* bvh, const tr_packed_hit* d_packed, int64_t n, int64_t row_length, uint8_t* d_hit,
                                 uint8_t* d_front, int32_t* d_tri, float* d_loc, float* d_uv, void* stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    if (n < 0 || row_length < 0) return tr_fail(TR_ERR_INVALID_ARG, "negative size");
    if (n == 0) return TR_OK;
    if (!d_packed) return tr_fail(TR_ERR_INVALID_ARG, "d_packed == NULL");
    tr_device_guard guard;
    TR_TRY(enter_bvh_device(bvh, nullptr, &guard));
    RayFetch none{};
    return expand_slots_impl<false>(bvh, d_packed, n, row_length, none, d_hit, d_front, d_tri, d_loc, d_uv, stream);
}

// The 4-byte record form (round 4): the traversal writes only the arena slot of the winning triangle (or -1), and
// whoever holds the RAYS finishes the query from (ray, slot) -- what write_result does at the end of a dense trace.
int tr_intersects_closest_slots(const tr_bvh* bvh, const tr_rays* rays, int32_t* d_slot, void* stream) {
    if (!d_slot && rays && rays->nray > 0) return tr_fail(TR_ERR_INVALID_ARG, "d_slot == NULL");
    if (bvh && bvh->num_tris * (int64_t)sizeof(tr_tri) >= ((int64_t)1 << 31))
        return tr_fail(TR_ERR_INVALID_ARG, "slot form needs a triangle array below 2 GiB");
    QueryOut out = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, reinterpret_cast<tr_packed_hit*>(d_slot), 2};
    return launch_query<TR_Q_CLOSEST, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

int tr_device_topology(int device, tr_topology* out) {
    if (!out) return tr_fail(TR_ERR_INVALID_ARG, "out == NULL");
    tr_device_state* st;
    TR_TRY(tr_get_device_state(device, &st));
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, device));
    tr_policy_units(st);
    out->num_cus = st->num_cus; out->num_xcd = st->num_xcd; out->waves_per_cu = st->waves_per_cu; out->reserved = 0;
    out->l2_bytes = st->l2_bytes;
    out->resident_lanes = (int64_t)st->num_cus * st->waves_per_cu * 64;
    out->steal_max_rays = tr_policy::steal_max_rays(st);
    out->wide_min_rays = tr_policy::wide_min_rays(st);
    out->count_stream_min_rays = tr_policy::stream_min_rays(st, TR_Q_COUNT);
    return TR_OK;
}

int tr_closest_from_slots(const tr_bvh* bvh, const tr_rays* rays, const int32_t* d_slot, int64_t row_length, uint8_t* d_hit,
                          uint8_t* d_front, int32_t* d_tri, float* d_loc, float* d_uv, void* stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    if (row_length < 0) return tr_fail(TR_ERR_INVALID_ARG, "negative size");
    RayFetch rf;
    TR_TRY(make_fetch(rays, &rf));
    if (rf.n == 0) return TR_OK;
    if (!d_slot) return tr_fail(TR_ERR_INVALID_ARG, "d_slot == NULL");
    tr_device_guard guard;
    TR_TRY(enter_bvh_device(bvh, rays, &guard));
    return expand_slots_impl<true>(bvh, d_slot, rf.n, row_length, rf, d_hit, d_front, d_tri, d_loc, d_uv, stream);
}

int tr_closest_expand_slots(const tr_bvh* bvh, const tr_packed_hit* d_packed, int64_t n, uint8_t* d_hit, uint8_t* d_front,
                            int32_t* d_tri, float* d_loc, float* d_uv, void* stream) {
    return tr_closest_expand_slots_rows(bvh, d_packed, n, 0, d_hit, d_front, d_tri, d_loc, d_uv, stream);
}

int tr_intersects_count(const tr_bvh* bvh, const tr_rays* rays, int32_t* d_count, void* stream) {
    if (!d_count && rays && rays->nray > 0) return tr_fail(TR_ERR_INVALID_ARG, "d_count == NULL");
    QueryOut out = {nullptr, nullptr, nullptr, nullptr, nullptr, d_count};
    return launch_query<TR_Q_COUNT, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

int tr_hits_scan(const int32_t* d_count, int64_t n, int32_t cap, int64_t* d_offsets,
                 int64_t* d_total, int64_t* h_total, void* stream) {
    if (cap < 0) return tr_fail(TR_ERR_INVALID_ARG, "cap < 0");
    return scan_impl<int32_t>(d_count, n, cap, d_offsets, d_total, h_total, (hipStream_t)stream);
}

int tr_mask_scan(const uint8_t* d_hit, int64_t n, int64_t* d_offsets, int64_t* d_total,
                 int64_t* h_total, void* stream) {
    return scan_impl<uint8_t>(d_hit, n, 1, d_offsets, d_total, h_total, (hipStream_t)stream);
}

int tr_intersects_location_fill(const tr_bvh* bvh, const tr_rays* rays, int32_t cap,
                                const int64_t* d_offsets, float* d_loc, int32_t* d_ray_idx,
                                int32_t* d_tri_idx, int64_t ray_base, void* stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    if (cap < 0 || cap > TR_MAX_HITS_CAP) return tr_fail(TR_ERR_INVALID_ARG, "cap out of range");
    RayFetch rf;
    TR_TRY(make_fetch(rays, &rf));
    if (rf.n == 0 || cap == 0) return TR_OK;
    if (!d_offsets) return tr_fail(TR_ERR_INVALID_ARG, "d_offsets == NULL");
    tr_device_guard guard;
    TR_TRY(enter_bvh_device(bvh, rays, &guard));
    tr_bvh_view view = tr_view_of(bvh);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((rf.n + 255) / 256)), block(256);
    if (cap <= 8)
        hipLaunchKernelGGL(k_location<8>, grid, block, 0, s, view, rf, cap, d_offsets, d_loc, d_ray_idx, d_tri_idx, ray_base);
    else if (cap <= 16)
        hipLaunchKernelGGL(k_location<16>, grid, block, 0, s, view, rf, cap, d_offsets, d_loc, d_ray_idx, d_tri_idx, ray_base);
    else
        hipLaunchKernelGGL(k_location<32>, grid, block, 0, s, view, rf, cap, d_offsets, d_loc, d_ray_idx, d_tri_idx, ray_base);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

int tr_intersects_count_topk(const tr_bvh* bvh, const tr_rays* rays, int32_t cap, int32_t* d_count,
                             tr_hit_entry* d_hits, void* stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    if (cap < 1 || cap > TR_MAX_HITS_CAP) return tr_fail(TR_ERR_INVALID_ARG, "cap out of range");
    RayFetch rf;
    TR_TRY(make_fetch(rays, &rf));
    if (rf.n == 0) return TR_OK;
    if (!d_count || !d_hits) return tr_fail(TR_ERR_INVALID_ARG, "null output pointer");
    QueryOut out = {nullptr, nullptr, nullptr, nullptr, nullptr, d_count, d_hits, cap};
    return launch_query<TR_Q_LOCATION, false>(bvh, rays, out, nullptr, (hipStream_t)stream);
}

int tr_location_fill_slots(const tr_bvh* bvh, const tr_rays* rays, int32_t cap, const int32_t* d_count,
                           const int64_t* d_offsets, const tr_hit_entry* d_hits, float* d_loc,
                           int32_t* d_ray_idx, int32_t* d_tri_idx, int64_t ray_base, void* stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    if (cap < 1 || cap > TR_MAX_HITS_CAP) return tr_fail(TR_ERR_INVALID_ARG, "cap out of range");
    RayFetch rf;
    TR_TRY(make_fetch(rays, &rf));
    if (rf.n == 0) return TR_OK;
    if (!d_count || !d_offsets || !d_hits) return tr_fail(TR_ERR_INVALID_ARG, "null input pointer");
    tr_device_guard guard;
    TR_TRY(enter_bvh_device(bvh, rays, &guard));
    tr_bvh_view view = tr_view_of(bvh);
    const int64_t threads = rf.n * cap;
    hipLaunchKernelGGL(k_fill_list, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       view, rf, cap, d_count, d_offsets, d_hits, d_loc, d_ray_idx, d_tri_idx, ray_base);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

int tr_compact_closest(const uint8_t* d_hit, const int64_t* d_offsets, int64_t n,
                       const uint8_t* d_front, const int32_t* d_tri, const float* d_loc,
                       const float* d_uv, int64_t ray_base, uint8_t* d_front_out,
                       int32_t* d_ray_idx_out, int32_t* d_tri_out, float* d_loc_out,
                       float* d_uv_out, void* stream) {
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    if (n == 0) return TR_OK;
    if (!d_hit || !d_offsets) return tr_fail(TR_ERR_INVALID_ARG, "null mask/offsets");
    if ((d_front_out && !d_front) || (d_tri_out && !d_tri) || (d_loc_out && !d_loc) || (d_uv_out && !d_uv))
        return tr_fail(TR_ERR_INVALID_ARG, "output requested without its input");
    hipLaunchKernelGGL(k_compact_closest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       d_hit, d_offsets, n, d_front, d_tri, d_loc, d_uv, ray_base, d_front_out,
                       d_ray_idx_out, d_tri_out, d_loc_out, d_uv_out);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

int tr_trace_stats_query(const tr_bvh* bvh, const tr_rays* rays, int query, tr_trace_stats* h_stats,
                   void* stream) {
    if (!bvh || !rays || !h_stats) return tr_fail(TR_ERR_INVALID_ARG, "null argument");
    if (query < TR_Q_ANY || query > TR_Q_LOCATION) return tr_fail(TR_ERR_INVALID_ARG, "unknown query id");
    hipStream_t s = (hipStream_t)stream;
    tr_device_guard guard;
    TR_TRY(enter_bvh_device(bvh, rays, &guard));
    int64_t n = rays->nray;
    unsigned long long* d_stats = nullptr;
    uint8_t* buf = nullptr;
    // scratch outputs of the instrumented launch: closest 26 B/ray, multi-hit 4 + 8*cap B/ray
    const size_t per_ray = 4 + 8 * (size_t)TR_MAX_ANYHIT_SIZE;
    TR_HIP_TRY(hipMalloc((void**)&d_stats, 64));
    hipError_t e = hipMalloc((void**)&buf, per_ray * (size_t)(n > 0 ? n : 1) + 64);
    if (e != hipSuccess) { (void)hipFree(d_stats); return tr_fail(TR_ERR_OUT_OF_MEMORY, "stats outputs"); }
    size_t nn = (size_t)(n > 0 ? n : 1);
    float* loc = (float*)buf;                       // 12 n
    float* uv = loc + 3 * nn;                       // 8 n
    int32_t* tri = (int32_t*)(uv + 2 * nn);         // 4 n
    uint8_t* hitp = (uint8_t*)(tri + nn);           // n
    uint8_t* front = hitp + nn;                     // n
    int status = TR_OK;
    if (hipMemsetAsync(d_stats, 0, 64, s) != hipSuccess) status = tr_fail(TR_ERR_HIP, "memset stats");
    if (status == TR_OK) {
        QueryOut out = {hitp, front, tri, loc, uv, nullptr, nullptr, 0};
        switch (query) {
            case TR_Q_ANY: status = launch_query<TR_Q_ANY, true>(bvh, rays, out, d_stats, s); break;
            case TR_Q_FIRST: status = launch_query<TR_Q_FIRST, true>(bvh, rays, out, d_stats, s); break;
            case TR_Q_CLOSEST: status = launch_query<TR_Q_CLOSEST, true>(bvh, rays, out, d_stats, s); break;
            case TR_Q_COUNT: out.count = (int32_t*)buf; status = launch_query<TR_Q_COUNT, true>(bvh, rays, out, d_stats, s); break;
            default:
                out.count = (int32_t*)buf;
                out.hits = (tr_hit_entry*)(buf + 4 * ((nn + 1) / 2 * 2));   // 8-byte aligned
                out.cap = TR_MAX_ANYHIT_SIZE;
                status = launch_query<TR_Q_LOCATION, true>(bvh, rays, out, d_stats, s);
        }
    }
    unsigned long long h[4] = {0, 0, 0, 0};
    if (status == TR_OK && hipMemcpyAsync(h, d_stats, 32, hipMemcpyDeviceToHost, s) != hipSuccess)
        status = tr_fail(TR_ERR_HIP, "memcpy stats");
    if (hipStreamSynchronize(s) != hipSuccess && status == TR_OK) status = tr_fail(TR_ERR_HIP, "sync stats");
    (void)hipFree(d_stats);
    (void)hipFree(buf);
    h_stats->rays = (uint64_t)n; h_stats->node_visits = h[1]; h_stats->tri_tests = h[2]; h_stats->climb_steps = h[3];
    return status;
}

int tr_trace_stats_closest(const tr_bvh* bvh, const tr_rays* rays, tr_trace_stats* h_stats, void* stream) {
    return tr_trace_stats_query(bvh, rays, TR_Q_CLOSEST, h_stats, stream);
}

}  // extern "C"
