// tris.hip -- libtriro_tris.so (include/triro_tris.h): the faces that meet each query triangle.
//
// The contract, the culling proof and the walk are csrc/tr_tris.h (host + device) on the box-culled set walk of csrc/tr_boxes.h
// and csrc/tr_walk.h and the ordering of csrc/tr_within.h; this file is the query load, the launches and the C entries (the
// kernel body: tr_set_kernel).
//
//  * One query triangle per lane, block k takes triangles 128 k ... 128 k + 127 (64-bit index math), shaped like k_boxes.
//  * k_tris<ANY | COUNT | FILL>: the stack of a lane is a column of LDS, TR_TRIS_STACK = 32 node ids, 16 KB per workgroup.
//    The box of the query is computed once per lane.  A lane whose stack overflowed drops what it found and walks the tree
//    again without one (tr_rewalk) after the wave's loop.  FILL leaves the rows of a query as face indices in walk order;
//    k_tris_rows (no LDS) orders them.
#include <string>

#include "tr_internal.h"
#include "tr_tris.h"
#include "../../include/triro_tris.h"

namespace {

constexpr int TQ_BS = TR_LANE_BS;      // one query triangle per lane, two waves per workgroup

struct tq_query {
    tr_tris_q q;
    tr_box box;
    bool in_range, live;
};

__device__ __forceinline__ tq_query tq_load(const tr_bvh_view& b, const float* __restrict__ tri, int64_t n, int64_t i) {
    tq_query r;
    r.in_range = i < n;
    r.q.px = 0.f; r.q.py = 0.f; r.q.pz = 0.f; r.q.qx = 0.f; r.q.qy = 0.f; r.q.qz = 0.f; r.q.rx = 0.f; r.q.ry = 0.f; r.q.rz = 0.f;  // (no area)
    if (r.in_range) {
        const float* p = tri + 9 * i;
        r.q.px = p[0]; r.q.py = p[1]; r.q.pz = p[2]; r.q.qx = p[3]; r.q.qy = p[4]; r.q.qz = p[5]; r.q.rx = p[6]; r.q.ry = p[7]; r.q.rz = p[8];
    }
    r.live = r.in_range && tr_tris_live(r.q) && b.num_tris > 0;
    r.box = tr_tris_box(r.q);
    return r;
}

}  // namespace

// ANY: out8[i] = 0 / 1.  COUNT: out32[i] = the number of faces met.  FILL: the faces of query i, in walk order, at rows
// offsets[i] .. of face, at most tr_rows_limit of them.
template <int MODE>
__global__ __launch_bounds__(TQ_BS) void k_tris(tr_bvh_view b, const float* __restrict__ tri, int64_t n, uint8_t* __restrict__ out8,
                                                int32_t* __restrict__ out32, const int32_t* __restrict__ count,
                                                const int64_t* __restrict__ offsets, int64_t total, int32_t* __restrict__ face,
                                                int stack_entries) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t stack_lds[TR_TRIS_STACK * TQ_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, TQ_BS};
    const int64_t i = (int64_t)blockIdx.x * TQ_BS + threadIdx.x;
    const tq_query q = tq_load(b, tri, n, i);
    tr_boxes_acc acc = {0, 0, nullptr};
    tr_set_kernel<MODE, TR_TRIS_STACK>(b, tr_tris_probe<MODE>(b, q.q, q.box, acc), stack, q.live, q.in_range, i, count, offsets, total,
                                       [&](int64_t off) { acc.key = face + off; }, stack_entries, out8, out32);
}

// after k_tris<FILL>: the rows of query i into ascending face order
__global__ __launch_bounds__(TQ_BS) void k_tris_rows(int64_t n, const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                     int64_t total, int32_t* __restrict__ face) {
    const int64_t i = (int64_t)blockIdx.x * TQ_BS + threadIdx.x;
    if (i >= n) return;
    const int64_t off = offsets[i];
    const int32_t m = tr_rows_limit(count[i], off, total);
    if (m <= 0) return;
    tr_tris_rows(face + off, m);
}

namespace {

// the checks every entry shares; nblocks comes back
int tq_check(const tr_bvh* bvh, const float* d_tri, int64_t n, const void* d_required, int stack_entries, int64_t& nblocks) {
    return tr_lane_check(bvh, d_tri != nullptr, n, d_required, stack_entries, TR_TRIS_STACK, "triangles", nblocks);
}

template <int MODE>
int tq_launch(const tr_bvh* bvh, const float* d_tri, int64_t n, uint8_t* out8, int32_t* out32, const int32_t* d_count,
              const int64_t* d_offsets, int64_t total, int32_t* d_face, int stack_entries, int64_t nblocks, void* stream) {
    hipLaunchKernelGGL(k_tris<MODE>, dim3((unsigned)nblocks), dim3(TQ_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_tri, n, out8, out32,
                       d_count, d_offsets, total, d_face, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_tris_abi_version(void) { return TR_TRIS_ABI_VERSION; }

int tr_tris_stack_capacity(void) { return TR_TRIS_STACK; }

int tr_tris_any(const tr_bvh* bvh, const float* d_tri, int64_t n, uint8_t* d_any, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = tq_check(bvh, d_tri, n, d_any, stack_entries, nblocks)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return tq_launch<TR_TRIS_ANY>(bvh, d_tri, n, d_any, nullptr, nullptr, nullptr, 0, nullptr, stack_entries, nblocks, stream);
}

int tr_tris_count(const tr_bvh* bvh, const float* d_tri, int64_t n, int32_t* d_count, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = tq_check(bvh, d_tri, n, d_count, stack_entries, nblocks)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return tq_launch<TR_TRIS_COUNT>(bvh, d_tri, n, nullptr, d_count, nullptr, nullptr, 0, nullptr, stack_entries, nblocks, stream);
}

int tr_tris_fill(const tr_bvh* bvh, const float* d_tri, int64_t n, const int32_t* d_count, const int64_t* d_offsets, int64_t total,
                 int32_t* d_face, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = tq_check(bvh, d_tri, n, d_count, stack_entries, nblocks)) return rc;
    TR_TRY(tr_fill_check(n, total, d_offsets, d_face != nullptr, "null pointer argument (d_face)"));
    if (n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    if (int rc = tq_launch<TR_TRIS_FILL>(bvh, d_tri, n, nullptr, nullptr, d_count, d_offsets, total, d_face, stack_entries, nblocks, stream))
        return rc;
    hipLaunchKernelGGL(k_tris_rows, dim3((unsigned)nblocks), dim3(TQ_BS), 0, (hipStream_t)stream, n, d_count, d_offsets, total, d_face);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
