// points.hip -- libtriro_points.so (include/triro_points.h): contains_points as ONE launch.
//
// The reference answers "is p inside the mesh" with two intersects_count launches on (p, d) and (p, -d) and tensor
// operations on the two count arrays (ray_optix.py:238-267).  k_contains_points traces both rays of a point in the
// SAME lane, one after the other, and writes the decision: 12 bytes in, 2 bytes out per point.
//
//  * Same lane, not lane pairs: neighbouring points with one direction walk the same nodes; two lanes with opposite
//    directions part at the root.
//  * Each pass is the wave loop of the unordered schedule (tr_unord_step, tr_bvh.h) over the 32-byte grid nodes, with the
//    count launch's LDS ring and leaf queue, declared once and used by both passes, and its leaf-phase vote.
//  * Every ray of a call has the same direction, and nothing here moves a ray to another lane (no stealing).  So what
//    tr_ray_setup derives from the direction alone -- d itself, the clamped reciprocals, kd, the three byte selectors --
//    is the same in every lane: it is computed once per pass and pinned to SGPRs (pt_uniform).  Per lane: the origin
//    (anchoring moves it along the ray, by a distance that depends on the point) and the constants of the fused box test
//    (tr_ray_fuse: their clamp and their margins depend on the origin).
//  * The counts are those of tr_intersects_count on the same rays, bit for bit: tr_ray_setup_q (anchoring included), the
//    predicate through tr_unord_step / tr_fold_leaf / tr_drain_exact, and the direct evaluation on meshes without a
//    hierarchy (fewer than two triangles).  The order of the leaf tests does not enter a count.
//  * No learned launch order, no split launch slots: block k takes points 128 k ... 128 k + 127.
#include <mutex>
#include <string>

#include "tr_internal.h"
#include "tr_points.h"
#include "../../include/triro_points.h"

namespace {

template <bool COMPACT, bool DEEP> struct pt_word { typedef uint64_t T; };
template <> struct pt_word<true, false> { typedef uint32_t T; };

// a value that is the same in every lane, held in an SGPR from here on (all lanes are active where this is called)
__device__ __forceinline__ float pt_uniform(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ uint32_t pt_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// hit count of the ray (p, d) for every lane of the wave; all 64 lanes call this together
template <bool COMPACT, bool DEEP>
__device__ __forceinline__ int32_t pt_count(const tr_bvh_view& b, float px, float py, float pz, float dx, float dy, float dz,
                                            bool in_range, const tr_ring ring, const tr_leafq lq, int leaf_min) {
    typedef typename pt_word<COMPACT, DEEP>::T W;
    tr_ray r;
    const bool valid = tr_ray_setup_q(r, b.frame, px, py, pz, dx, dy, dz) && in_range;
    r.dx = pt_uniform(r.dx); r.dy = pt_uniform(r.dy); r.dz = pt_uniform(r.dz);
    r.ix = pt_uniform(r.ix); r.iy = pt_uniform(r.iy); r.iz = pt_uniform(r.iz);
    r.kd = pt_uniform(r.kd);
    r.sel_n = pt_uniform(r.sel_n); r.sel_f = pt_uniform(r.sel_f); r.sel_z = pt_uniform(r.sel_z);
    tr_result res;
    tr_result_init(res);
    tr_topk<1> top;
    tr_counters* nc = nullptr;
    if (b.num_tris >= 2) {
        tr_ustate_t<W> st;
        tr_ustate_init(st);
        if (!valid) st.node = -1;
        for (;;) {
            const bool can_node = tr_ucan_node(st);
            const unsigned long long mn = __ballot(can_node), ml = __ballot(st.nq > 0);
            if ((mn | ml) == 0ull) break;
            const bool parked = st.node >= 0 && !can_node;
            const bool leaf_phase = mn == 0ull || __ballot(parked) != 0ull || (int)__popcll(ml) >= leaf_min;
            tr_unord_step<TR_Q_COUNT, 1, false, COMPACT, W>(b, r, can_node, leaf_phase, st, res, top, nc, ring, lq);
            TR_CONVERGE();
        }
    } else if (valid && b.num_tris == 1) {
        // no hierarchy below two triangles (wave-uniform): the whole predicate on the one triangle there may be
        const tr_tri t = tr_load_tri<false>(b, 0, nc);
        tr_hit h;
        if (tr_tri_test(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, h)) res.count = 1;
    }
    return res.count;
}

constexpr int PT_BS = 128;      // one point per lane, two waves per workgroup (the count launch's block)

template <bool COMPACT, bool DEEP>
__global__ __launch_bounds__(PT_BS) void k_contains_points(tr_bvh_view b, const float* __restrict__ points, int64_t n,
                                                           const float* __restrict__ dir3, const float* __restrict__ box_lo,
                                                           const float* __restrict__ box_hi, uint8_t* __restrict__ inside,
                                                           uint8_t* __restrict__ broken, int32_t* __restrict__ counts,
                                                           unsigned long long* __restrict__ summary, int leaf_min) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t ring_lds[TR_RING * PT_BS];
    __shared__ int32_t leafq_lds[TR_LEAFQ * PT_BS];
    const tr_ring ring = {ring_lds + threadIdx.x, PT_BS};
    const tr_leafq lq = {leafq_lds + threadIdx.x, PT_BS};
    const int64_t i = (int64_t)blockIdx.x * PT_BS + threadIdx.x;
    const bool in_range = i < n;
    // the box test first: what stays of it is a lane mask, and the point itself need not live through the traversals: each
    // pass loads it again (the same 12 bytes, a global load behind an index the compiler cannot see through, so that the
    // load stays inside the pass), which is three registers less while the passes run
    bool in_box = in_range;
    {
        float px = 0.f, py = 0.f, pz = 0.f;
        if (in_range) { px = points[3 * i]; py = points[3 * i + 1]; pz = points[3 * i + 2]; }
        if (box_lo != nullptr && box_hi != nullptr) {      // (uniform addresses: scalar loads)
            const float lo[3] = {box_lo[0], box_lo[1], box_lo[2]}, hi[3] = {box_hi[0], box_hi[1], box_hi[2]};
            in_box = in_range && tr_point_in_box(px, py, pz, lo, hi);
        }
    }
    const float d0 = dir3[0], d1 = dir3[1], d2 = dir3[2];      // (uniform again)
    int32_t cp = 0, cm = 0;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        int64_t j = in_range ? i : 0;
        __asm__ volatile("" : "+v"(j));       // (no instruction: the index is opaque, the load below is not hoisted out of the loop)
        float px = 0.f, py = 0.f, pz = 0.f;
        if (in_range) { px = points[3 * j]; py = points[3 * j + 1]; pz = points[3 * j + 2]; }
        const float s = pass ? -1.0f : 1.0f;        // (a product with +-1 is exact: -d is the reference's `-ray_directions`)
        const int32_t c = pt_count<COMPACT, DEEP>(b, px, py, pz, s * d0, s * d1, s * d2, in_range, ring, lq, leaf_min);
        if (pass) cm = c; else cp = c;
    }
    bool is_inside, is_broken;
    tr_point_decide(in_box, cp, cm, is_inside, is_broken);
    is_broken = is_broken && in_range;
    if (in_range) {
        inside[i] = is_inside ? 1 : 0;
        broken[i] = is_broken ? 1 : 0;
        if (counts) { counts[i] = cp; counts[n + i] = cm; }
    }
    // one ballot and one atomic per wave and total
    const unsigned long long mb = __ballot(in_box), mk = __ballot(is_broken);
    if ((threadIdx.x & 63) == 0) {
        if (mb) atomicAdd(&summary[0], (unsigned long long)__popcll(mb));
        if (mk) atomicAdd(&summary[1], (unsigned long long)__popcll(mk));
    }
}

// 32-bit offsets when both arrays are below 4 GiB, 32-bit trail words when the hierarchy is at most 32 levels high: the
// rule of the count launch (launch_policy.inc).  1 compact, 2 deep (32-bit offsets, 64-bit trail), 0 generic
int pt_addressing(const tr_bvh* bvh, const tr_options& opt) {
    const bool addr32 = opt.compact && bvh->num_nodes * (int64_t)sizeof(tr_node) < ((int64_t)1 << 32) &&
                        bvh->num_tris * (int64_t)sizeof(tr_tri) < ((int64_t)1 << 32);
    return addr32 ? (bvh->depth <= 32 ? 1 : 2) : 0;
}

// Sixteen bytes of zeros in the memory of each device, never written again: the summary is zeroed by a device-to-device
// COPY from them.  Not by hipMemsetAsync: the memset node of a captured call left two stale 8-byte values (they look like
// host addresses) in the summary on every replay, while the eager call zeroed it.  The root cause is not known (a property
// of memset nodes of this size in the runtime, as far as one observation goes); the copy node is what torch's own `copy_`
// into static buffers records, and replays correctly.  The block is made (one hipMalloc, one synchronous hipMemset) by
// tr_contains_addressing -- the call a binding makes when it sets a handle up -- or, failing that, by the first
// tr_contains_points on the device; it lives as long as the process.
constexpr int PT_MAX_DEVICES = 64;
std::mutex g_zero_mutex;
void* g_zero[PT_MAX_DEVICES] = {};
int pt_zeros(int device, const void** out) {
    if (device < 0 || device >= PT_MAX_DEVICES) return tr_fail(TR_ERR_INVALID_ARG, "device ordinal out of range");
    std::lock_guard<std::mutex> lock(g_zero_mutex);
    if (!g_zero[device]) {
        void* p = nullptr;
        TR_HIP_TRY(hipMalloc(&p, 64));
        if (hipMemset(p, 0, 64) != hipSuccess) { (void)hipFree(p); return tr_fail(TR_ERR_HIP, "hipMemset of the zero block failed"); }
        g_zero[device] = p;
    }
    *out = g_zero[device];
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_points_abi_version(void) { return TR_POINTS_ABI_VERSION; }

int tr_contains_addressing(const tr_bvh* bvh) {
    if (!bvh) return -1;
    {   // the init path of the zero block (pt_zeros): after this, tr_contains_points on this device allocates nothing
        tr_device_guard guard;
        const void* zeros = nullptr;
        if (guard.enter(bvh->device) == TR_OK) (void)pt_zeros(bvh->device, &zeros);
    }
    return pt_addressing(bvh, tr_opts());
}

int tr_contains_points(const tr_bvh* bvh, const float* d_points, int64_t n, const float* d_dir3, const float* d_box_lo3,
                       const float* d_box_hi3, uint8_t* d_inside, uint8_t* d_broken, int32_t* d_counts, int64_t* d_summary2,
                       int64_t* h_summary2, void* stream) {
    if (!bvh) return tr_fail(TR_ERR_INVALID_ARG, "bvh == NULL");
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    if (!d_summary2) return tr_fail(TR_ERR_INVALID_ARG, "d_summary2 == NULL");
    if ((d_box_lo3 == nullptr) != (d_box_hi3 == nullptr))
        return tr_fail(TR_ERR_INVALID_ARG, "d_box_lo3 and d_box_hi3 must both be given or both be NULL");
    if (n > 0 && (!d_points || !d_dir3 || !d_inside || !d_broken)) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    const int64_t nblocks = (n + PT_BS - 1) / PT_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many points for one launch");
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    hipStream_t s = (hipStream_t)stream;
    const void* zeros = nullptr;
    TR_TRY(pt_zeros(bvh->device, &zeros));
    TR_HIP_TRY(hipMemcpyAsync(d_summary2, zeros, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (n > 0) {
        const tr_options opt = tr_opts();   // one snapshot per call
        const tr_bvh_view view = tr_view_of(bvh);
        unsigned long long* sum = reinterpret_cast<unsigned long long*>(d_summary2);
        const dim3 grid((unsigned)nblocks), block(PT_BS);
        switch (pt_addressing(bvh, opt)) {
            case 1:
                hipLaunchKernelGGL((k_contains_points<true, false>), grid, block, 0, s, view, d_points, n, d_dir3, d_box_lo3,
                                   d_box_hi3, d_inside, d_broken, d_counts, sum, opt.leaf_vote);
                break;
            case 2:
                hipLaunchKernelGGL((k_contains_points<true, true>), grid, block, 0, s, view, d_points, n, d_dir3, d_box_lo3,
                                   d_box_hi3, d_inside, d_broken, d_counts, sum, opt.leaf_vote);
                break;
            default:
                hipLaunchKernelGGL((k_contains_points<false, false>), grid, block, 0, s, view, d_points, n, d_dir3, d_box_lo3,
                                   d_box_hi3, d_inside, d_broken, d_counts, sum, opt.leaf_vote);
        }
        TR_HIP_TRY(hipGetLastError());
    }
    if (h_summary2) {
        TR_HIP_TRY(hipMemcpyAsync(h_summary2, d_summary2, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        TR_HIP_TRY(hipStreamSynchronize(s));
    }
    return TR_OK;
}

}  // extern "C"
