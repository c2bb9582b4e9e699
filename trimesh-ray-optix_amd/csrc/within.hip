// within.hip -- libtriro_within.so (include/triro_within.h): the faces within a distance of each point.
//
// The contract, the culling argument and the walks are csrc/tr_within.h (host + device) on the per-triangle function and the
// box bound of csrc/tr_nearest.h; this file is the wave loops around the set walk (tr_within_probe) and tr_near_visit, the launches and the
// C entries.
//
//  * One point per lane, block k takes points 128 k ... 128 k + 127 (64-bit index math), shaped like k_closest_point.
//  * k_within<ANY | COUNT | FILL>: the stack of a lane is a column of LDS, TR_WITHIN_STACK = 32 node ids, 16 KB per
//    workgroup.  A lane whose stack overflowed drops what it found and walks the tree again without one (tr_rewalk)
//    after the wave's loop.  FILL leaves the rows of a point in walk order; k_within_rows (no LDS) orders them by face index
//    and evaluates the optional distance / closest rows.
//  * k_within_closest: k_closest_point with a best that starts at the radius (32 entries of {node, bound}, 32 KB).
#include <string>

#include "tr_internal.h"
#include "tr_within.h"
#include "../../include/triro_within.h"

namespace {

constexpr int WI_BS = TR_LANE_BS;      // one point per lane, two waves per workgroup

struct wi_query {
    float px, py, pz, r;
    bool in_range, valid;
};

__device__ __forceinline__ wi_query wi_load(const tr_bvh_view& b, const float* __restrict__ points, const float* __restrict__ radii,
                                            float radius, int64_t n, int64_t i) {
    wi_query q;
    q.in_range = i < n;
    q.px = 0.f; q.py = 0.f; q.pz = 0.f; q.r = -1.f;
    if (q.in_range) {
        q.px = points[3 * i]; q.py = points[3 * i + 1]; q.pz = points[3 * i + 2];
        q.r = radii ? radii[i] : radius;
    }
    q.valid = q.in_range && tr_within_valid(q.px, q.py, q.pz, q.r) && b.num_tris > 0;
    return q;
}

}  // namespace

// ANY: out8[i] = 0 / 1.  COUNT: out32[i] = the number of faces within.  FILL: the faces of point i, in walk order, at rows
// offsets[i] .. of face (and their arena slots at the same rows of slot, where given), at most tr_rows_limit of them.
// The body is tr_set_kernel (tr_walk.h) written out: called from here, the ANY instantiation allocates 114 VGPRs instead of
// 126 and gains 38 instructions, and a kernel whose allocation moves keeps its text.
template <int MODE>
__global__ __launch_bounds__(WI_BS) void k_within(tr_bvh_view b, const float* __restrict__ points, int64_t n,
                                                  const float* __restrict__ radii, float radius, uint8_t* __restrict__ out8,
                                                  int32_t* __restrict__ out32, const int32_t* __restrict__ count,
                                                  const int64_t* __restrict__ offsets, int64_t total, int32_t* __restrict__ face,
                                                  int32_t* __restrict__ slot, int stack_entries) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t stack_lds[TR_WITHIN_STACK * WI_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, WI_BS};
    const int64_t i = (int64_t)blockIdx.x * WI_BS + threadIdx.x;
    const wi_query q = wi_load(b, points, radii, radius, n, i);
    const double R2 = tr_within_r2(q.r);
    tr_within_acc acc;
    acc.count = 0; acc.limit = 0; acc.face = nullptr; acc.slot = nullptr;
    if (MODE == TR_WITHIN_FILL && q.in_range) {
        const int64_t off = offsets[i];
        acc.limit = tr_rows_limit(count[i], off, total);
        if (acc.limit > 0) { acc.face = face + off; acc.slot = slot ? slot + off : nullptr; }
    }
    const tr_within_probe<MODE> probe = {b, q.px, q.py, q.pz, R2, acc};
    const bool walk = q.valid && !probe.done();      // (FILL: a point without rows has nothing to do)
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_WITHIN_STACK);
        tr_walk_state st;
        st.node = walk ? 0 : -1; st.sp = 0;
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) probe.visit(st, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_walk_lost(st.sp) && !probe.done()) {      // cold: the partial result is dropped, not added to
            acc.count = 0;
            tr_rewalk(b, probe);
        }
    } else if (walk) {
        probe.leaf(0);      // no hierarchy below two triangles
    }
    if (q.in_range) {
        if (MODE == TR_WITHIN_ANY) out8[i] = acc.count > 0 ? 1 : 0;
        if (MODE == TR_WITHIN_COUNT) out32[i] = acc.count;
    }
}

// after k_within<FILL>: the rows of point i into ascending face order, then the optional outputs of each row
__global__ __launch_bounds__(WI_BS) void k_within_rows(tr_bvh_view b, const float* __restrict__ points, int64_t n,
                                                       const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                       int64_t total, int32_t* __restrict__ face, int32_t* __restrict__ slot,
                                                       float* __restrict__ distance, float* __restrict__ closest) {
    TR_VIEW_LIVE(b);
    const int64_t i = (int64_t)blockIdx.x * WI_BS + threadIdx.x;
    if (i >= n) return;
    const int64_t off = offsets[i];
    const int32_t m = tr_rows_limit(count[i], off, total);
    if (m <= 0) return;
    tr_within_rows(b, points[3 * i], points[3 * i + 1], points[3 * i + 2], face + off, slot ? slot + off : nullptr, m,
                   distance ? distance + off : nullptr, closest ? closest + 3 * off : nullptr);
}

__global__ __launch_bounds__(WI_BS) void k_within_closest(tr_bvh_view b, const float* __restrict__ points, int64_t n,
                                                          const float* __restrict__ radii, float radius, float* __restrict__ closest,
                                                          float* __restrict__ distance, int32_t* __restrict__ tri, int stack_entries) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t stack_lds[2 * TR_NEAR_STACK * WI_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, WI_BS};
    const int64_t i = (int64_t)blockIdx.x * WI_BS + threadIdx.x;
    const wi_query q = wi_load(b, points, radii, radius, n, i);
    tr_near_best best;
    tr_within_closest_init(best, tr_within_r2(q.r));
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
        tr_near_state st;
        st.node = q.valid ? 0 : -1; st.sp = 0;
        for (int32_t node = st.node;;) {      // the seed descent (tr_near_seed): its leaf counts only if it is within
            if (!TR_WAVE_ANY(node >= 0)) break;
            if (node >= 0) node = tr_near_seed(b, node, q.px, q.py, q.pz, best);
            TR_CONVERGE();
        }
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) tr_near_visit(b, q.px, q.py, q.pz, st, best, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_near_lost(st.sp)) tr_rewalk(b, tr_near_probe{b, q.px, q.py, q.pz, best});
    } else if (q.valid) {
        tr_near_leaf(b, 0, q.px, q.py, q.pz, best);
    }
    if (q.in_range)
        tr_near_outputs(b, q.px, q.py, q.pz, q.valid, best, closest ? closest + 3 * i : nullptr, distance ? distance + i : nullptr, tri + i);
}

namespace {

// the checks every entry shares; nblocks comes back
int wi_check(const tr_bvh* bvh, const float* d_points, int64_t n, const void* d_required, int stack_entries, int capacity,
             int64_t& nblocks) {
    return tr_lane_check(bvh, d_points != nullptr, n, d_required, stack_entries, capacity, "points", nblocks);
}

template <int MODE>
int wi_launch(const tr_bvh* bvh, const float* d_points, int64_t n, const float* d_radius, float radius, uint8_t* out8, int32_t* out32,
              const int32_t* d_count, const int64_t* d_offsets, int64_t total, int32_t* d_face, int32_t* d_slot, int stack_entries,
              int64_t nblocks, void* stream) {
    hipLaunchKernelGGL(k_within<MODE>, dim3((unsigned)nblocks), dim3(WI_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_points, n,
                       d_radius, radius, out8, out32, d_count, d_offsets, total, d_face, d_slot, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_within_abi_version(void) { return TR_WITHIN_ABI_VERSION; }

int tr_within_stack_capacity(void) { return TR_WITHIN_STACK; }

int tr_within_any(const tr_bvh* bvh, const float* d_points, int64_t n, const float* d_radius, float radius, uint8_t* d_any,
                  int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = wi_check(bvh, d_points, n, d_any, stack_entries, TR_WITHIN_STACK, nblocks)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return wi_launch<TR_WITHIN_ANY>(bvh, d_points, n, d_radius, radius, d_any, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                                    stack_entries, nblocks, stream);
}

int tr_within_count(const tr_bvh* bvh, const float* d_points, int64_t n, const float* d_radius, float radius, int32_t* d_count,
                    int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = wi_check(bvh, d_points, n, d_count, stack_entries, TR_WITHIN_STACK, nblocks)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return wi_launch<TR_WITHIN_COUNT>(bvh, d_points, n, d_radius, radius, nullptr, d_count, nullptr, nullptr, 0, nullptr, nullptr,
                                      stack_entries, nblocks, stream);
}

int tr_within_fill(const tr_bvh* bvh, const float* d_points, int64_t n, const float* d_radius, float radius, const int32_t* d_count,
                   const int64_t* d_offsets, int64_t total, int32_t* d_face, float* d_distance, float* d_closest3, int32_t* d_slot,
                   int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = wi_check(bvh, d_points, n, d_count, stack_entries, TR_WITHIN_STACK, nblocks)) return rc;
    TR_TRY(tr_fill_check(n, total, d_offsets, d_face && (d_slot || !(d_distance || d_closest3)),
                         "null pointer argument (d_face, or d_slot with d_distance / d_closest3)"));
    if (n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    if (!d_distance && !d_closest3) d_slot = nullptr;
    if (int rc = wi_launch<TR_WITHIN_FILL>(bvh, d_points, n, d_radius, radius, nullptr, nullptr, d_count, d_offsets, total, d_face,
                                           d_slot, stack_entries, nblocks, stream))
        return rc;
    hipLaunchKernelGGL(k_within_rows, dim3((unsigned)nblocks), dim3(WI_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_points, n, d_count,
                       d_offsets, total, d_face, d_slot, d_distance, d_closest3);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

int tr_within_closest(const tr_bvh* bvh, const float* d_points, int64_t n, const float* d_radius, float radius, float* d_closest,
                      float* d_distance, int32_t* d_tri, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = wi_check(bvh, d_points, n, d_tri, stack_entries, TR_NEAR_STACK, nblocks)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    hipLaunchKernelGGL(k_within_closest, dim3((unsigned)nblocks), dim3(WI_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_points, n,
                       d_radius, radius, d_closest, d_distance, d_tri, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
