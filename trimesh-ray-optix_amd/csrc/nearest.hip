// nearest.hip -- libtriro_nearest.so (include/triro_nearest.h): closest_point as one launch.
//
// A nearest-triangle walk is not the ray walk: it is ordered by the children's box distances and pruned by the best
// squared distance found so far.  The contract, the culling bound and the walk are csrc/tr_nearest.h (host + device);
// this file is the wave loops around tr_near_seed and tr_near_visit, the launch and the C entry.
//
//  * One point per lane, block k takes points 128 k ... 128 k + 127 (64-bit index math).  No stealing, no learned launch
//    order, no grid nodes: the walk reads the exact 64-byte nodes (tr_node) and the triangle records.
//  * The far-child stack of a lane is a column of LDS: TR_NEAR_STACK = 32 entries of {node, float32 bound}, 32 KB per
//    workgroup.  A lane whose stack overflowed walks the tree again without one (tr_rewalk on a tr_near_probe) after the wave's loop.
//  * One instantiation, 64-bit address arithmetic.
#include <string>

#include "tr_internal.h"
#include "tr_nearest.h"
#include "../../include/triro_nearest.h"

namespace {

constexpr int NR_BS = TR_LANE_BS;      // one point per lane, two waves per workgroup

}  // namespace

__global__ __launch_bounds__(NR_BS) void k_closest_point(tr_bvh_view b, const float* __restrict__ points, int64_t n,
                                                         float* __restrict__ closest, float* __restrict__ distance,
                                                         int32_t* __restrict__ tri, int stack_entries) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t stack_lds[2 * TR_NEAR_STACK * NR_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, NR_BS};
    const int64_t i = (int64_t)blockIdx.x * NR_BS + threadIdx.x;
    const bool in_range = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (in_range) { px = points[3 * i]; py = points[3 * i + 1]; pz = points[3 * i + 2]; }
    const bool valid = in_range && tr_near_valid(px, py, pz) && b.num_tris > 0;
    tr_near_best best;
    tr_near_init(best);
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
        tr_near_state st;
        st.node = valid ? 0 : -1; st.sp = 0;
        // the seed descent: a finite best before the first push (tr_near_seed)
        for (int32_t node = st.node;;) {
            if (!TR_WAVE_ANY(node >= 0)) break;
            if (node >= 0) node = tr_near_seed(b, node, px, py, pz, best);
            TR_CONVERGE();
        }
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) tr_near_visit(b, px, py, pz, st, best, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_near_lost(st.sp)) tr_rewalk(b, tr_near_probe{b, px, py, pz, best});
    } else if (valid) {
        tr_near_leaf(b, 0, px, py, pz, best);      // no hierarchy below two triangles
    }
    if (in_range)
        tr_near_outputs(b, px, py, pz, valid, best, closest ? closest + 3 * i : nullptr, distance ? distance + i : nullptr, tri + i);
}

extern "C" {

int tr_nearest_abi_version(void) { return TR_NEAREST_ABI_VERSION; }

int tr_nearest_stack_capacity(void) { return TR_NEAR_STACK; }

int tr_closest_point(const tr_bvh* bvh, const float* d_points, int64_t n, float* d_closest, float* d_distance, int32_t* d_tri,
                     int stack_entries, void* stream) {
    int64_t nblocks = 0;
    TR_TRY(tr_lane_check(bvh, d_points != nullptr, n, d_tri, stack_entries, TR_NEAR_STACK, "points", nblocks));
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    hipLaunchKernelGGL(k_closest_point, dim3((unsigned)nblocks), dim3(NR_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_points, n,
                       d_closest, d_distance, d_tri, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
