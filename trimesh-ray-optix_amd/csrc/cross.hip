// cross.hip -- libtriro_cross.so (include/triro_cross.h): every crossing of a ray on a per-ray interval [tmin, tmax]: the count,
// and the uncapped ordered list.
//
// The contract, the culling argument, the walk and the ordering are csrc/tr_cross.h (host + device) on the ray set-up, the
// bounds, the per-triangle predicate and the box tests of csrc/tr_range.h; this file is the wave loop around tr_cross_visit,
// the launches and the C entries.
//
//  * One ray per lane, block k takes rays 128 k ... 128 k + 127 (64-bit index math), shaped like k_range_query.  No stealing,
//    no learned launch order, no grid nodes, no anchoring: the walk reads the exact 64-byte nodes and the triangle records.
//  * Rays arrive as tr_rays and are read as every other kernel reads them: RayFetch / fetch_ray of kernels_common.inc
//    (dense, broadcast and general strides).
//  * k_cross<COUNT | FILL>: the stack of a lane is a column of LDS, TR_CROSS_STACK = 32 node ids, 16 KB per workgroup.  A
//    lane whose stack overflowed drops what it found and walks the tree again without one (tr_rewalk on a tr_cross_probe) after the wave's
//    loop.  FILL leaves the rows of a ray in walk order; k_cross_rows (no LDS) orders them by (t, face) and evaluates the
//    optional front / loc / uv / ray rows.
#include <string>

#include "tr_internal.h"
#include "tr_cross.h"
#include "../../include/triro_cross.h"

namespace {

#include "kernels_common.inc"

constexpr int CR_BS = 128;      // one ray per lane, two waves per workgroup

struct cr_query {
    tr_ray r;
    float lo, hi;
    bool in_range, valid;
};

__device__ __forceinline__ cr_query cr_load(const tr_bvh_view& b, const RayFetch& rf, const float* __restrict__ tmin,
                                            const float* __restrict__ tmax, int64_t i) {
    cr_query q;
    q.in_range = i < rf.n;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    q.lo = 0.0f; q.hi = TR_TMAX;
    if (q.in_range) {
        fetch_ray(rf, i, o, d);
        if (tmin) q.lo = tmin[i];
        if (tmax) q.hi = tmax[i];
    }
    bool valid = tr_ray_setup(q.r, o[0], o[1], o[2], d[0], d[1], d[2]);
    q.valid = tr_range_bounds(q.lo, q.hi, q.lo, q.hi) && valid && q.in_range && b.num_tris > 0;
    return q;
}

}  // namespace

// COUNT: out32[i] = the number of crossings.  FILL: the crossings of ray i, in walk order, at rows offsets[i] .. of face and t
// (and their arena slots at the same rows of slot, where given), at most tr_rows_limit of them.
template <int MODE>
__global__ __launch_bounds__(CR_BS) void k_cross(tr_bvh_view b, RayFetch rf, const float* __restrict__ tmin,
                                                 const float* __restrict__ tmax, int32_t* __restrict__ out32,
                                                 const int32_t* __restrict__ count, const int64_t* __restrict__ offsets, int64_t total,
                                                 int32_t* __restrict__ face, float* __restrict__ t, int32_t* __restrict__ slot,
                                                 int stack_entries) {
    __shared__ int32_t stack_lds[TR_CROSS_STACK * CR_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, CR_BS};
    const int64_t i = (int64_t)blockIdx.x * CR_BS + threadIdx.x;
    const cr_query q = cr_load(b, rf, tmin, tmax, i);
    tr_cross_acc acc;
    acc.count = 0; acc.limit = 0; acc.face = nullptr; acc.t = nullptr; acc.slot = nullptr;
    if (MODE == TR_CROSS_FILL && q.in_range) {
        const int64_t off = offsets[i];
        acc.limit = tr_rows_limit(count[i], off, total);
        if (acc.limit > 0) { acc.face = face + off; acc.t = t + off; acc.slot = slot ? slot + off : nullptr; }
    }
    const bool walk = q.valid && !tr_cross_full<MODE>(acc);      // (FILL: a ray without rows has nothing to do)
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_CROSS_STACK);
        tr_cross_state st;
        st.node = walk ? 0 : -1; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) tr_cross_visit<MODE>(b, q.r, q.lo, q.hi, st, acc, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_walk_lost(st.sp) && !tr_cross_full<MODE>(acc)) {      // cold: the partial result is dropped, not added to
            acc.count = 0;
            tr_rewalk(b, tr_cross_probe<MODE>{b, q.r, q.lo, q.hi, acc});
        }
    } else if (walk) {
        tr_counters* nc = nullptr;
        const tr_tri w = tr_load_tri<false, false>(b, 0, nc);      // no hierarchy below two triangles
        float tt;
        if (tr_range_tri(q.r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, q.lo, q.hi, tt))
            tr_cross_record<MODE>(acc, w.face, tt, 0);
    }
    if (MODE == TR_CROSS_COUNT && q.in_range) out32[i] = acc.count;
}

// after k_cross<FILL>: the rows of ray i into ascending (t, face) order, then the optional outputs of each row
__global__ __launch_bounds__(CR_BS) void k_cross_rows(tr_bvh_view b, RayFetch rf, const int32_t* __restrict__ count,
                                                      const int64_t* __restrict__ offsets, int64_t total, int32_t* __restrict__ face,
                                                      float* __restrict__ t, int32_t* __restrict__ slot, uint8_t* __restrict__ front,
                                                      float* __restrict__ loc, float* __restrict__ uv, int64_t* __restrict__ ray,
                                                      int64_t ray_base) {
    const int64_t i = (int64_t)blockIdx.x * CR_BS + threadIdx.x;
    if (i >= rf.n) return;
    const int64_t off = offsets[i];
    const int32_t m = tr_rows_limit(count[i], off, total);
    if (m <= 0) return;
    float o[3], d[3];
    fetch_ray(rf, i, o, d);
    tr_ray r;
    tr_ray_setup(r, o[0], o[1], o[2], d[0], d[1], d[2]);
    tr_cross_rows(b, r, face + off, t + off, slot ? slot + off : nullptr, m, front ? front + off : nullptr, loc ? loc + 3 * off : nullptr,
                  uv ? uv + 2 * off : nullptr, ray ? ray + off : nullptr, i + ray_base);
}

namespace {

// the checks every entry shares (what range_launch refuses); the RayFetch and nblocks come back
int cross_check(const tr_bvh* bvh, const tr_rays* rays, const void* required, int stack_entries, RayFetch& rf, int64_t& nblocks) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    TR_TRY(make_fetch(rays, &rf));
    if (stack_entries < 0 || stack_entries > TR_CROSS_STACK)
        return tr_fail(TR_ERR_INVALID_ARG, "stack_entries must be 0 (all) or 1 .. " + std::to_string(TR_CROSS_STACK));
    if (rf.n > 0 && !required) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    nblocks = (rf.n + CR_BS - 1) / CR_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many rays for one launch");
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_cross_abi_version(void) { return TR_CROSS_ABI_VERSION; }

int tr_cross_stack_capacity(void) { return TR_CROSS_STACK; }

int tr_cross_count(const tr_bvh* bvh, const tr_rays* rays, const float* d_tmin, const float* d_tmax, int32_t* d_count,
                   int stack_entries, void* stream) {
    RayFetch rf;
    int64_t nblocks = 0;
    if (int rc = cross_check(bvh, rays, d_count, stack_entries, rf, nblocks)) return rc;
    if (rf.n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    hipLaunchKernelGGL((k_cross<TR_CROSS_COUNT>), dim3((unsigned)nblocks), dim3(CR_BS), 0, (hipStream_t)stream, tr_view_of(bvh), rf,
                       d_tmin, d_tmax, d_count, nullptr, nullptr, (int64_t)0, nullptr, nullptr, nullptr, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

int tr_cross_fill(const tr_bvh* bvh, const tr_rays* rays, const float* d_tmin, const float* d_tmax, const int32_t* d_count,
                  const int64_t* d_offsets, int64_t total, int32_t* d_face, float* d_t, uint8_t* d_front, float* d_loc3, float* d_uv2,
                  int64_t* d_ray, int64_t ray_base, int32_t* d_slot, int stack_entries, void* stream) {
    RayFetch rf;
    int64_t nblocks = 0;
    if (int rc = cross_check(bvh, rays, d_count, stack_entries, rf, nblocks)) return rc;
    if (total < 0) return tr_fail(TR_ERR_INVALID_ARG, "total < 0");
    if (rf.n > 0 && !d_offsets) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    const bool evaluate = d_front || d_loc3 || d_uv2;
    if (rf.n > 0 && total > 0 && (!d_face || !d_t || (evaluate && !d_slot)))
        return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument (d_face, d_t, or d_slot with d_front / d_loc3 / d_uv2)");
    if (rf.n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    if (!evaluate) d_slot = nullptr;
    hipLaunchKernelGGL((k_cross<TR_CROSS_FILL>), dim3((unsigned)nblocks), dim3(CR_BS), 0, (hipStream_t)stream, tr_view_of(bvh), rf,
                       d_tmin, d_tmax, nullptr, d_count, d_offsets, total, d_face, d_t, d_slot, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cross_rows, dim3((unsigned)nblocks), dim3(CR_BS), 0, (hipStream_t)stream, tr_view_of(bvh), rf, d_count, d_offsets,
                       total, d_face, d_t, d_slot, d_front, d_loc3, d_uv2, d_ray, ray_base);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
