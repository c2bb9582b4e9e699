// range.hip -- libtriro_range.so (include/triro_range.h): any / closest on a per-ray interval [tmin, tmax], one launch each.
//
// The contract, the band around a bound, the culling proof and the walk are csrc/tr_range.h (host + device); this file is
// the wave loop around tr_range_visit, the launch and the C entries.
//
//  * One ray per lane, block k takes rays 128 k ... 128 k + 127 (64-bit index math).  No stealing, no learned launch
//    order, no grid nodes, no anchoring: the walk reads the exact 64-byte nodes (tr_node) and the triangle records.
//  * Rays arrive as tr_rays and are read as every other kernel reads them: RayFetch / fetch_ray of kernels_common.inc
//    (dense, broadcast and general strides).
//  * The far-child stack of a lane is a column of LDS: TR_RANGE_STACK = 32 entries of {node, entry distance}, 32 KB per
//    workgroup.  A lane whose stack overflowed walks the tree again without one (tr_rewalk on a tr_range_probe) after the wave's loop.
//  * One instantiation per query, 64-bit address arithmetic.
#include <string>

#include "tr_internal.h"
#include "tr_range.h"
#include "../../include/triro_range.h"

namespace {

#include "kernels_common.inc"

constexpr int RG_BS = 128;      // one ray per lane, two waves per workgroup

struct RangeOut {
    uint8_t* hit;
    uint8_t* front;
    int32_t* tri;
    float* t;
    float* loc;
    float* uv;
};

}  // namespace

template <int Q>
__global__ __launch_bounds__(RG_BS) void k_range_query(tr_bvh_view b, RayFetch rf, const float* __restrict__ tmin,
                                                       const float* __restrict__ tmax, RangeOut out, int stack_entries) {
    __shared__ int32_t stack_lds[2 * TR_RANGE_STACK * RG_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, RG_BS};
    const int64_t i = (int64_t)blockIdx.x * RG_BS + threadIdx.x;
    const bool in_range = i < rf.n;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, lo = 0.0f, hi = TR_TMAX;
    if (in_range) {
        fetch_ray(rf, i, o, d);
        if (tmin) lo = tmin[i];
        if (tmax) hi = tmax[i];
    }
    tr_ray r;
    bool valid = tr_ray_setup(r, o[0], o[1], o[2], d[0], d[1], d[2]);
    valid = tr_range_bounds(lo, hi, lo, hi) && valid && in_range && b.num_tris > 0;
    tr_range_best best;
    tr_range_init(best);
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_RANGE_STACK);
        tr_range_state st;
        st.node = valid ? 0 : -1; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) tr_range_visit<Q>(b, r, lo, hi, st, best, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_range_lost(st.sp)) tr_rewalk(b, tr_range_probe<Q>{b, r, lo, hi, best});
    } else if (valid) {
        tr_counters* nc = nullptr;
        const tr_tri w = tr_load_tri<false, false>(b, 0, nc);      // no hierarchy below two triangles
        float tt;
        if (tr_range_tri(r, w.ax, w.ay, w.az, w.bx, w.by, w.bz, w.cx, w.cy, w.cz, lo, hi, tt)) tr_range_fold(tt, w.face, 0, best);
    }
    if (in_range)
        tr_range_outputs(b, r, valid, best, out.hit ? out.hit + i : nullptr, out.front ? out.front + i : nullptr,
                         out.tri ? out.tri + i : nullptr, out.t ? out.t + i : nullptr, out.loc ? out.loc + 3 * i : nullptr,
                         out.uv ? out.uv + 2 * i : nullptr);
}

namespace {

template <int Q>
int range_launch(const tr_bvh* bvh, const tr_rays* rays, const float* d_tmin, const float* d_tmax, const RangeOut& out,
                 const void* required, int stack_entries, void* stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    RayFetch rf;
    TR_TRY(make_fetch(rays, &rf));
    if (stack_entries < 0 || stack_entries > TR_RANGE_STACK)
        return tr_fail(TR_ERR_INVALID_ARG, "stack_entries must be 0 (all) or 1 .. " + std::to_string(TR_RANGE_STACK));
    if (rf.n > 0 && !required) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    const int64_t nblocks = (rf.n + RG_BS - 1) / RG_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many rays for one launch");
    if (rf.n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    hipLaunchKernelGGL((k_range_query<Q>), dim3((unsigned)nblocks), dim3(RG_BS), 0, (hipStream_t)stream, tr_view_of(bvh), rf, d_tmin, d_tmax,
                       out, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_range_abi_version(void) { return TR_RANGE_ABI_VERSION; }

int tr_range_stack_capacity(void) { return TR_RANGE_STACK; }

int tr_range_any(const tr_bvh* bvh, const tr_rays* rays, const float* d_tmin, const float* d_tmax, uint8_t* d_hit,
                 int stack_entries, void* stream) {
    const RangeOut out = {d_hit, nullptr, nullptr, nullptr, nullptr, nullptr};
    return range_launch<TR_Q_ANY>(bvh, rays, d_tmin, d_tmax, out, d_hit, stack_entries, stream);
}

int tr_range_closest(const tr_bvh* bvh, const tr_rays* rays, const float* d_tmin, const float* d_tmax, int32_t* d_tri, float* d_t,
                     uint8_t* d_hit, uint8_t* d_front, float* d_loc3, float* d_uv2, int stack_entries, void* stream) {
    const RangeOut out = {d_hit, d_front, d_tri, d_t, d_loc3, d_uv2};
    return range_launch<TR_Q_CLOSEST>(bvh, rays, d_tmin, d_tmax, out, d_tri, stack_entries, stream);
}

}  // extern "C"
