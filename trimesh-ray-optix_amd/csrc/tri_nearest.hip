// tri_nearest.hip -- libtriro_tri_nearest.so (include/triro_tri_nearest.h): the nearest face to each query triangle as one launch.
//
// The contract, the culling bound and the walk are csrc/tr_tri_nearest.h (host + device) on the per-triangle function and the
// far-child stack of csrc/tr_nearest.h and the overlap predicate of csrc/tr_tris.h; this file is the query load, the wave
// loops around tr_tn_seed and tr_tn_visit, the launch and the C entry.
//
//  * One query triangle per lane, block k takes triangles 128 k ... 128 k + 127 (64-bit index math), shaped like
//    k_closest_point.  The box of the query and its squared bound are computed once per lane.
//  * The far-child stack of a lane is a column of LDS: TR_NEAR_STACK = 32 entries of {node, float32 bound}, 32 KB per
//    workgroup.  A lane whose stack overflowed walks the tree again without one (tr_rewalk on a tr_tn_probe) after the wave's loop.
//  * One instantiation: a query without a bound carries max_distance = +Inf, which starts the best where tr_near_init does.
#include <string>

#include "tr_internal.h"
#include "tr_tri_nearest.h"
#include "../../include/triro_tri_nearest.h"

namespace {

constexpr int TN_BS = TR_LANE_BS;      // one query triangle per lane, two waves per workgroup

}  // namespace

// 32 KB of LDS per workgroup allow five workgroups, ten waves, per CU: three waves on a SIMD at the most, which 168 VGPRs allow
// (DESIGN.md 4.16).  Left to itself the allocator spreads to 202.
__global__ __launch_bounds__(TN_BS) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_triangles_nearest(tr_bvh_view b, const float* __restrict__ tri, int64_t n,
                                                             const float* __restrict__ radii, float radius, int32_t* __restrict__ out_tri,
                                                             float* __restrict__ distance, float* __restrict__ closest_mesh,
                                                             float* __restrict__ closest_query, int stack_entries) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t stack_lds[2 * TR_NEAR_STACK * TN_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, TN_BS};
    const int64_t i = (int64_t)blockIdx.x * TN_BS + threadIdx.x;
    const bool in_range = i < n;
    tr_tris_q q;
    q.px = 0.f; q.py = 0.f; q.pz = 0.f; q.qx = 0.f; q.qy = 0.f; q.qz = 0.f; q.rx = 0.f; q.ry = 0.f; q.rz = 0.f;
    float r = -1.f;
    if (in_range) {
        const float* p = tri + 9 * i;
        q.px = p[0]; q.py = p[1]; q.pz = p[2]; q.qx = p[3]; q.qy = p[4]; q.qz = p[5]; q.rx = p[6]; q.ry = p[7]; q.rz = p[8];
        r = radii ? radii[i] : radius;
    }
    const bool valid = in_range && tr_tn_valid(q, r) && b.num_tris > 0;
    tr_tn_query_t Q = tr_tn_make(q, r);
    tr_near_best best;
    tr_within_closest_init(best, Q.R2);
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
        tr_near_state st;
        st.node = valid ? 0 : -1; st.sp = 0;
        // the seed descent: a finite best before the first push (tr_tn_seed)
        for (int32_t node = st.node;;) {
            if (!TR_WAVE_ANY(node >= 0)) break;
            if (node >= 0) node = tr_tn_seed(b, node, Q, best);
            TR_CONVERGE();
        }
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) tr_tn_visit(b, Q, st, best, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_near_lost(st.sp)) tr_rewalk(b, tr_tn_probe{b, Q, best});
    } else if (valid) {
        tr_tn_leaf(b, 0, Q, best);      // no hierarchy below two triangles
    }
    if (in_range)
        tr_tn_outputs(b, Q, valid, best, out_tri + i, distance ? distance + i : nullptr, closest_mesh ? closest_mesh + 3 * i : nullptr,
                      closest_query ? closest_query + 3 * i : nullptr);
}

extern "C" {

int tr_tri_nearest_abi_version(void) { return TR_TRI_NEAREST_ABI_VERSION; }

int tr_tri_nearest_stack_capacity(void) { return TR_NEAR_STACK; }

int tr_triangles_nearest(const tr_bvh* bvh, const float* d_triangles, int64_t n, const float* d_max, float max_distance, int32_t* d_tri,
                         float* d_distance, float* d_closest_mesh, float* d_closest_query, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    TR_TRY(tr_lane_check(bvh, d_triangles != nullptr, n, d_tri, stack_entries, TR_NEAR_STACK, "triangles", nblocks));
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    hipLaunchKernelGGL(k_triangles_nearest, dim3((unsigned)nblocks), dim3(TN_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_triangles, n, d_max,
                       max_distance, d_tri, d_distance, d_closest_mesh, d_closest_query, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
