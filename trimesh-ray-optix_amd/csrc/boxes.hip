// boxes.hip -- libtriro_boxes.so (include/triro_boxes.h): the faces that meet each axis-aligned box.
//
// The contract, the culling proof and the walk are csrc/tr_boxes.h (host + device) on the stack and the row limit of
// csrc/tr_walk.h and the ordering of csrc/tr_within.h; this file is the wave loop around tr_boxes_visit, the launches and the
// C entries.
//
//  * One box per lane, block k takes boxes 128 k ... 128 k + 127 (64-bit index math), shaped like k_within.
//  * k_boxes<ANY | COUNT | FILL>: the stack of a lane is a column of LDS, TR_BOXES_STACK = 32 node ids, 16 KB per
//    workgroup.  A lane whose stack overflowed drops what it found and walks the tree again without one (tr_boxes_rewalk)
//    after the wave's loop.  FILL leaves the rows of a box as keys in walk order; k_boxes_rows (no LDS) orders them by face
//    index and unpacks face and `inside`.
#include <string>

#include "tr_internal.h"
#include "tr_boxes.h"
#include "../../include/triro_boxes.h"

namespace {

constexpr int BX_BS = TR_LANE_BS;      // one box per lane, two waves per workgroup

struct bx_query {
    tr_box q;
    bool in_range, valid;
};

__device__ __forceinline__ bx_query bx_load(const tr_bvh_view& b, const float* __restrict__ lo, const float* __restrict__ hi, int64_t n,
                                            int64_t i) {
    bx_query r;
    r.in_range = i < n;
    r.q.lox = 0.f; r.q.loy = 0.f; r.q.loz = 0.f; r.q.hix = -1.f; r.q.hiy = -1.f; r.q.hiz = -1.f;      // (lo > hi: invalid)
    if (r.in_range) {
        r.q.lox = lo[3 * i]; r.q.loy = lo[3 * i + 1]; r.q.loz = lo[3 * i + 2];
        r.q.hix = hi[3 * i]; r.q.hiy = hi[3 * i + 1]; r.q.hiz = hi[3 * i + 2];
    }
    r.valid = r.in_range && tr_box_valid(r.q) && b.num_tris > 0;
    return r;
}

}  // namespace

// ANY: out8[i] = 0 / 1.  COUNT: out32[i] = the number of faces met.  FILL: the keys (tr_boxes_key) of the faces of box i, in
// walk order, at rows offsets[i] .. of face, at most tr_rows_limit of them.
template <int MODE>
__global__ __launch_bounds__(BX_BS) void k_boxes(tr_bvh_view b, const float* __restrict__ lo, const float* __restrict__ hi, int64_t n,
                                                 uint8_t* __restrict__ out8, int32_t* __restrict__ out32,
                                                 const int32_t* __restrict__ count, const int64_t* __restrict__ offsets, int64_t total,
                                                 int32_t* __restrict__ face, int stack_entries) {
    TR_VIEW_LIVE(b);
    __shared__ int32_t stack_lds[TR_BOXES_STACK * BX_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, BX_BS};
    const int64_t i = (int64_t)blockIdx.x * BX_BS + threadIdx.x;
    const bx_query q = bx_load(b, lo, hi, n, i);
    tr_boxes_acc acc;
    acc.count = 0; acc.limit = 0; acc.key = nullptr;
    if (MODE == TR_BOXES_FILL && q.in_range) {
        const int64_t off = offsets[i];
        acc.limit = tr_rows_limit(count[i], off, total);
        if (acc.limit > 0) acc.key = face + off;
    }
    const bool walk = q.valid && !tr_set_full<MODE>(acc);      // (FILL: a box without rows has nothing to do)
    if (b.num_tris >= 2) {      // (wave-uniform)
        const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_BOXES_STACK);
        tr_walk_state st;
        st.node = walk ? 0 : -1; st.sp = 0;
        for (;;) {
            if (!TR_WAVE_ANY(st.node >= 0)) break;
            if (st.node >= 0) tr_boxes_visit<MODE>(b, q.q, st, acc, stack, cap2);
            TR_CONVERGE();
        }
        if (tr_walk_lost(st.sp) && !tr_set_full<MODE>(acc)) {      // cold: the partial result is dropped, not added to
            acc.count = 0;
            tr_boxes_rewalk<MODE>(b, q.q, acc);
        }
    } else if (walk) {
        tr_boxes_leaf<MODE>(b, 0, q.q, acc);      // no hierarchy below two triangles
    }
    if (q.in_range) {
        if (MODE == TR_BOXES_ANY) out8[i] = acc.count > 0 ? 1 : 0;
        if (MODE == TR_BOXES_COUNT) out32[i] = acc.count;
    }
}

// after k_boxes<FILL>: the rows of box i into ascending face order, unpacked into face and (where given) inside
__global__ __launch_bounds__(BX_BS) void k_boxes_rows(int64_t n, const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                      int64_t total, int32_t* __restrict__ face, uint8_t* __restrict__ inside) {
    const int64_t i = (int64_t)blockIdx.x * BX_BS + threadIdx.x;
    if (i >= n) return;
    const int64_t off = offsets[i];
    const int32_t m = tr_rows_limit(count[i], off, total);
    if (m <= 0) return;
    tr_boxes_rows(face + off, inside ? inside + off : nullptr, m);
}

namespace {

// the checks every entry shares; nblocks comes back
int bx_check(const tr_bvh* bvh, const float* d_lo, const float* d_hi, int64_t n, const void* d_required, int stack_entries,
             int64_t& nblocks) {
    return tr_lane_check(bvh, d_lo && d_hi, n, d_required, stack_entries, TR_BOXES_STACK, "boxes", nblocks);
}

template <int MODE>
int bx_launch(const tr_bvh* bvh, const float* d_lo, const float* d_hi, int64_t n, uint8_t* out8, int32_t* out32, const int32_t* d_count,
              const int64_t* d_offsets, int64_t total, int32_t* d_face, int stack_entries, int64_t nblocks, void* stream) {
    hipLaunchKernelGGL(k_boxes<MODE>, dim3((unsigned)nblocks), dim3(BX_BS), 0, (hipStream_t)stream, tr_view_of(bvh), d_lo, d_hi, n, out8,
                       out32, d_count, d_offsets, total, d_face, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_boxes_abi_version(void) { return TR_BOXES_ABI_VERSION; }

int tr_boxes_stack_capacity(void) { return TR_BOXES_STACK; }

int tr_boxes_any(const tr_bvh* bvh, const float* d_lo, const float* d_hi, int64_t n, uint8_t* d_any, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = bx_check(bvh, d_lo, d_hi, n, d_any, stack_entries, nblocks)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return bx_launch<TR_BOXES_ANY>(bvh, d_lo, d_hi, n, d_any, nullptr, nullptr, nullptr, 0, nullptr, stack_entries, nblocks, stream);
}

int tr_boxes_count(const tr_bvh* bvh, const float* d_lo, const float* d_hi, int64_t n, int32_t* d_count, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = bx_check(bvh, d_lo, d_hi, n, d_count, stack_entries, nblocks)) return rc;
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    return bx_launch<TR_BOXES_COUNT>(bvh, d_lo, d_hi, n, nullptr, d_count, nullptr, nullptr, 0, nullptr, stack_entries, nblocks, stream);
}

int tr_boxes_fill(const tr_bvh* bvh, const float* d_lo, const float* d_hi, int64_t n, const int32_t* d_count, const int64_t* d_offsets,
                  int64_t total, int32_t* d_face, uint8_t* d_inside, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = bx_check(bvh, d_lo, d_hi, n, d_count, stack_entries, nblocks)) return rc;
    TR_TRY(tr_fill_check(n, total, d_offsets, d_face != nullptr, "null pointer argument (d_face)"));
    if (n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, bvh->device));
    if (int rc = bx_launch<TR_BOXES_FILL>(bvh, d_lo, d_hi, n, nullptr, nullptr, d_count, d_offsets, total, d_face, stack_entries, nblocks,
                                          stream))
        return rc;
    hipLaunchKernelGGL(k_boxes_rows, dim3((unsigned)nblocks), dim3(BX_BS), 0, (hipStream_t)stream, n, d_count, d_offsets, total, d_face,
                       d_inside);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
