// planes.hip -- libtriro_planes.so (include/triro_planes.h): the faces that each plane meets or cuts, and the section segments.
//
// The contract, the culling proof, the walk and the ordering network are csrc/tr_planes.h (host + device); this file is the wave
// loop around tr_planes_visit / tr_planes_sub_next, the workgroup loop around tr_planes_step, the launches and the C entries.
//
//  * k_planes<ANY | COUNT | FILL>: ONE WAVE PER PLANE, one wave per workgroup (block i is plane i), so the barriers that order
//    the frontier's LDS traffic are workgroup barriers of a single wave and every branch around them is wave-uniform.  The
//    frontier is TR_PLANES_FRONTIER node ids, 8 KB of LDS.  FILL leaves the rows of a plane as faces in walk order (and, where
//    segments are asked for, the arena slot of each row in word 0 of its segment).
//  * k_planes_rows: ONE WORKGROUP PER PLANE orders the rows by face index with the network of tr_planes.h, a barrier between its
//    steps; a plane of at most PL_TILE rows is ordered in LDS, a longer one in place in global memory.
//  * k_planes_segments: ONE LANE PER ROW evaluates (p0, p1) from (plane, slot).
#include <string>

#include "tr_internal.h"
#include "tr_planes.h"
#include "../../include/triro_planes.h"

namespace {

constexpr int PL_ROWS_BS = 256;      // k_planes_rows, k_planes_segments
constexpr int PL_TILE = 4096;        // rows of a plane that are ordered in LDS: 2 x 16 KB

__device__ __forceinline__ tr_plane pl_load(const float* __restrict__ org, const float* __restrict__ nrm, int64_t i) {
    tr_plane q;
    q.ox = org[3 * i]; q.oy = org[3 * i + 1]; q.oz = org[3 * i + 2];
    q.nx = nrm[3 * i]; q.ny = nrm[3 * i + 1]; q.nz = nrm[3 * i + 2];
    return q;
}

// where FILL writes the rows of its plane
struct pl_rows {
    int32_t* face;
    int32_t* seg;
    int64_t off;
    int32_t limit;
};

// evaluate the candidates of the wave (an arena slot per lane, or -1) in converged code and record the hits at the cursor by
// ballot + lane rank; returns the new cursor (wave-uniform)
template <int MODE>
__device__ __forceinline__ int32_t pl_record(const tr_bvh_view& b, const tr_plane& q, int cut, int lane, int32_t cand, int32_t cursor,
                                             const pl_rows& rows) {
    if (__ballot(cand >= 0) == 0ull) return cursor;
    int32_t f = 0;
    const bool hit = cand >= 0 && tr_planes_leaf(b, cand, q, cut, f);
    TR_CONVERGE();
    const uint64_t mh = __ballot(hit);
    if (MODE == TR_PLANES_FILL) {
        const int32_t pos = cursor + tr_planes_rank(mh, lane);
        if (hit && pos < rows.limit) {
            rows.face[rows.off + pos] = f;
            if (rows.seg) rows.seg[6 * (rows.off + pos)] = cand;
        }
    }
    return cursor + tr_planes_popc(mh);
}

}  // namespace

// ANY: out8[i] = 0 / 1.  COUNT: out32[i] = the number of faces met (cut).  FILL: the faces of plane i, in walk order, at rows
// offsets[i] .. of face, at most tr_rows_limit of them; with seg, the arena slot of a row in the first word of its segment.
template <int MODE>
__global__ __launch_bounds__(TR_PLANES_WAVE) void k_planes(tr_bvh_view b, const float* __restrict__ org, const float* __restrict__ nrm,
                                                           uint8_t* __restrict__ out8, int32_t* __restrict__ out32,
                                                           const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                           int64_t total, int32_t* __restrict__ face, int32_t* __restrict__ seg, int cut,
                                                           int frontier_entries) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t frontier[TR_PLANES_FRONTIER];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x;
    const tr_plane q = pl_load(org, nrm, i);
    const int32_t cap = frontier_entries > 0 ? frontier_entries : TR_PLANES_FRONTIER;
    int32_t limit = 0;
    int64_t off = 0;
    if (MODE == TR_PLANES_FILL) {
        off = offsets[i];
        limit = tr_rows_limit(count[i], off, total);
    }
    int32_t cursor = 0;      // faces found so far (wave-uniform)
    const pl_rows rows = {face, seg, off, limit};
    const bool walk = tr_plane_valid(q) && b.num_tris > 0 && !(MODE == TR_PLANES_FILL && limit <= 0);      // (wave-uniform)
    if (walk && b.num_tris < 2) {
        cursor = pl_record<MODE>(b, q, cut, lane, lane == 0 ? 0 : -1, cursor, rows);      // no hierarchy below two triangles
    } else if (walk) {
        int32_t top = 1;
        if (lane == 0) frontier[0] = 0;
        __syncthreads();
        tr_planes_sub sub;
        tr_planes_sub_init(sub);
        for (;;) {
            if (__ballot(sub.node >= 0) != 0ull) {      // subtree walks first: each lane on to its next candidate
                const int32_t cand = sub.node >= 0 ? tr_planes_sub_next(b, q, sub) : -1;
                TR_CONVERGE();
                cursor = pl_record<MODE>(b, q, cut, lane, cand, cursor, rows);
                if (tr_planes_full<MODE>(cursor, limit)) break;
                continue;
            }
            if (top == 0) break;
            // a round: lane l takes entry top - 1 - l
            const int32_t take = top < TR_PLANES_WAVE ? top : TR_PLANES_WAVE;
            const int32_t node = lane < take ? frontier[top - 1 - lane] : -1;
            top -= take;
            __syncthreads();      // every entry is read before the pushes reuse its place
            const tr_planes_found fd = tr_planes_visit(b, node, q);
            TR_CONVERGE();
            const uint64_t m0 = __ballot(fd.push0 >= 0), m1 = __ballot(fd.push1 >= 0);
            const int32_t at0 = top + tr_planes_rank(m0, lane), at1 = top + tr_planes_popc(m0) + tr_planes_rank(m1, lane);
            if (fd.push0 >= 0) { if (at0 < cap) frontier[at0] = fd.push0; else tr_planes_sub_start(sub, fd.push0); }
            if (fd.push1 >= 0) { if (at1 < cap) frontier[at1] = fd.push1; else tr_planes_sub_start(sub, fd.push1); }
            top += tr_planes_popc(m0) + tr_planes_popc(m1);
            top = top < cap ? top : cap;
            __syncthreads();
            cursor = pl_record<MODE>(b, q, cut, lane, fd.leaf0, cursor, rows);
            if (tr_planes_full<MODE>(cursor, limit)) break;
            cursor = pl_record<MODE>(b, q, cut, lane, fd.leaf1, cursor, rows);
            if (tr_planes_full<MODE>(cursor, limit)) break;
        }
    }
    if (lane == 0) {
        if (MODE == TR_PLANES_ANY) out8[i] = cursor > 0 ? 1 : 0;
        if (MODE == TR_PLANES_COUNT) out32[i] = cursor;
    }
}

// after k_planes<FILL> (or on keys of the caller's: tr_planes_order): the rows of plane i into ascending order; seg (may be null):
// word 0 of each row's segment rides along
__global__ __launch_bounds__(PL_ROWS_BS) void k_planes_rows(const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                            int64_t total, int32_t* __restrict__ face, int32_t* __restrict__ seg) {
    __shared__ int32_t keys[PL_TILE];
    __shared__ int32_t ride[PL_TILE];
    const int64_t i = (int64_t)blockIdx.x;
    const int64_t off = offsets[i];
    const uint32_t m = (uint32_t)tr_rows_limit(count[i], off, total);      // (uniform in the workgroup)
    if (m < 2u) return;
    int32_t* f = face + off;
    int32_t* s = seg ? seg + 6 * off : nullptr;
    int64_t stride = 6;
    const bool tile = m <= (uint32_t)PL_TILE;
    if (tile) {
        for (uint32_t r = threadIdx.x; r < m; r += PL_ROWS_BS) {
            keys[r] = f[r];
            if (s) ride[r] = s[6 * (int64_t)r];
        }
        f = keys;
        s = s ? ride : nullptr;
        stride = 1;
        __syncthreads();
    }
    for (uint32_t k = 1u; k < m; k <<= 1) {
        tr_planes_step(f, s, stride, m, k, 0u, threadIdx.x, PL_ROWS_BS);
        __syncthreads();
        for (uint32_t j = k >> 1; j >= 1u; j >>= 1) {
            tr_planes_step(f, s, stride, m, k, j, threadIdx.x, PL_ROWS_BS);
            __syncthreads();
        }
    }
    if (tile) {
        int32_t* gf = face + off;
        for (uint32_t r = threadIdx.x; r < m; r += PL_ROWS_BS) {
            gf[r] = keys[r];
            if (seg) seg[6 * (off + (int64_t)r)] = ride[r];
        }
    }
}

// after k_planes_rows: (p0, p1) of every row that belongs to a plane
__global__ __launch_bounds__(PL_ROWS_BS) void k_planes_segments(tr_bvh_view b, const float* __restrict__ org, const float* __restrict__ nrm,
                                                                int64_t n, const int32_t* __restrict__ count,
                                                                const int64_t* __restrict__ offsets, int64_t total, float* __restrict__ seg) {
    TR_VIEW_LIVE(b);
    const int64_t r = (int64_t)blockIdx.x * PL_ROWS_BS + threadIdx.x;
    if (r >= total || b.num_tris <= 0) return;
    const int64_t i = tr_planes_owner(offsets, n, r);
    const int64_t off = offsets[i];
    const int32_t m = tr_rows_limit(count[i], off, total);
    if (r < off || r >= off + m) return;      // (a row between the planes' rows: counts and offsets that are not a scan)
    const int32_t slot = reinterpret_cast<const int32_t*>(seg)[6 * r];
    tr_planes_row(b, pl_load(org, nrm, i), slot, seg + 6 * r);
}

namespace {

// the checks every entry shares
int pl_check(const tr_bvh* bvh, const float* d_org, const float* d_nrm, int64_t n, const void* d_required, int cut, int frontier_entries) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    if (cut != 0 && cut != 1) return tr_fail(TR_ERR_INVALID_ARG, "cut must be 0 (meet) or 1 (cut)");
    if (frontier_entries < 0 || frontier_entries > TR_PLANES_FRONTIER)
        return tr_fail(TR_ERR_INVALID_ARG, "frontier_entries must be 0 (all) or 1 .. " + std::to_string(TR_PLANES_FRONTIER));
    if (n > 0 && (!d_org || !d_nrm || !d_required)) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    if (n > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many planes for one launch");
    return TR_OK;
}

template <int MODE>
int pl_launch(const tr_bvh* bvh, const float* d_org, const float* d_nrm, int64_t n, uint8_t* out8, int32_t* out32, const int32_t* d_count,
              const int64_t* d_offsets, int64_t total, int32_t* d_face, float* d_segments, int cut, int frontier_entries, void* stream) {
    hipLaunchKernelGGL(k_planes<MODE>, dim3((unsigned)n), dim3(TR_PLANES_WAVE), 0, (hipStream_t)stream, tr_view_of(bvh), d_org, d_nrm, out8,
                       out32, d_count, d_offsets, total, d_face, reinterpret_cast<int32_t*>(d_segments), cut, frontier_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_planes_abi_version(void) { return TR_PLANES_ABI_VERSION; }

int tr_planes_frontier_capacity(void) { return TR_PLANES_FRONTIER; }

int tr_planes_any(const tr_bvh* bvh, const float* d_origins, const float* d_normals, int64_t n, uint8_t* d_any, int cut, int frontier_entries,
                  void* stream) {
    if (int rc = pl_check(bvh, d_origins, d_normals, n, d_any, cut, frontier_entries)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return pl_launch<TR_PLANES_ANY>(bvh, d_origins, d_normals, n, d_any, nullptr, nullptr, nullptr, 0, nullptr, nullptr, cut, frontier_entries,
                                    stream);
}

int tr_planes_count(const tr_bvh* bvh, const float* d_origins, const float* d_normals, int64_t n, int32_t* d_count, int cut,
                    int frontier_entries, void* stream) {
    if (int rc = pl_check(bvh, d_origins, d_normals, n, d_count, cut, frontier_entries)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return pl_launch<TR_PLANES_COUNT>(bvh, d_origins, d_normals, n, nullptr, d_count, nullptr, nullptr, 0, nullptr, nullptr, cut,
                                      frontier_entries, stream);
}

int tr_planes_fill(const tr_bvh* bvh, const float* d_origins, const float* d_normals, int64_t n, const int32_t* d_count,
                   const int64_t* d_offsets, int64_t total, int32_t* d_face, float* d_segments, int cut, int frontier_entries, void* stream) {
    if (int rc = pl_check(bvh, d_origins, d_normals, n, d_count, cut, frontier_entries)) return rc;
    if (total < 0) return tr_fail(TR_ERR_INVALID_ARG, "total < 0");
    if (d_segments && cut != 1) return tr_fail(TR_ERR_INVALID_ARG, "segments are those of cut faces: d_segments needs cut == 1");
    if (n > 0 && !d_offsets) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    if (n > 0 && total > 0 && !d_face) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument (d_face)");
    const int64_t row_blocks = (total + PL_ROWS_BS - 1) / PL_ROWS_BS;
    if (d_segments && row_blocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many rows for one launch");
    if (n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    if (int rc = pl_launch<TR_PLANES_FILL>(bvh, d_origins, d_normals, n, nullptr, nullptr, d_count, d_offsets, total, d_face, d_segments, cut,
                                           frontier_entries, stream))
        return rc;
    hipLaunchKernelGGL(k_planes_rows, dim3((unsigned)n), dim3(PL_ROWS_BS), 0, (hipStream_t)stream, d_count, d_offsets, total, d_face,
                       reinterpret_cast<int32_t*>(d_segments));
    TR_HIP_TRY(hipGetLastError());
    if (d_segments) {
        hipLaunchKernelGGL(k_planes_segments, dim3((unsigned)row_blocks), dim3(PL_ROWS_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_origins,
                           d_normals, n, d_count, d_offsets, total, d_segments);
        TR_HIP_TRY(hipGetLastError());
    }
    return TR_OK;
}

int tr_planes_order(int device, int64_t n, const int32_t* d_count, const int64_t* d_offsets, int64_t total, int32_t* d_key, void* stream) {
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    if (total < 0) return tr_fail(TR_ERR_INVALID_ARG, "total < 0");
    if (n > 0 && (!d_count || !d_offsets)) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    if (n > 0 && total > 0 && !d_key) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument (d_key)");
    if (n > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many segments for one launch");
    if (n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, device));
    hipLaunchKernelGGL(k_planes_rows, dim3((unsigned)n), dim3(PL_ROWS_BS), 0, (hipStream_t)stream, d_count, d_offsets, total, d_key,
                       (int32_t*)nullptr);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
