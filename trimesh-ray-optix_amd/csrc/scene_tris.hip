// scene_tris.hip -- libtriro_scene_tris.so (include/triro_scene_tris.h): the (instance, face) pairs of the placed copies of a
// scene's members that meet each world triangle: any, count and the ordered list.
//
// The contract, the culling proof, the overflow rule and the row order are csrc/tr_scene_tris.h (host + device), on the placed
// box of csrc/tr_scene_nearest.h, the predicate of csrc/tr_tris.h and the set walk of csrc/tr_walk.h; this file is the query
// load, the wave-uniform instance loop around the wave loop of an instance's walk, the launches and the C entries.  The scene
// is libtriro_scene.so's: this library reads the committed table of the opaque handle (csrc/tr_scene_handle.h) and never
// changes it.
//
//  * One query triangle per lane, block k takes triangles 128 k ... 128 k + 127 (64-bit index math), the stack a column of LDS
//    (TR_TRIS_STACK node ids, 16 KB per workgroup): the shape of k_tris.  The box of the query is computed once per lane.
//  * THE INSTANCE LOOP IS WAVE-UNIFORM, as in k_scene_closest_point: every lane of a wave visits instance k at the same time,
//    so the record and the member's pointers are uniform loads and the twelve entries of M stay in SGPRs (st_uniform).  The
//    nine corner masks of the placed box (tr_scene_near_map), one v_bfi_b32 per chosen corner, are SPLIT between SGPRs and
//    VGPRs (ST_MASKS_IN_SGPRS): all nine in VGPRs the kernels need 130 / 132 / 138 VGPRs (ANY / COUNT / FILL), three waves per
//    SIMD; all nine in SGPRs 113 / 115 / 120 but 9 / 12 / 5 SGPRs spill.  Each mask moved to an SGPR frees two VGPRs; the
//    split below is the largest number of SGPR masks at which no instantiation spills: 122 / 124 / 126 VGPRs, four waves.
//  * The cull of an instance is the first visit of its root: the placed boxes of the root's children against the query's box.
//  * A lane that has nothing to find in an instance (an invalid or degenerate query, ANY with a pair, FILL with its rows full)
//    starts the walk without a node.  A lane whose stack overflowed drops what it found IN THAT INSTANCE and repeats that
//    instance without a stack before the wave moves on.
//  * k_scene_tris<FILL> leaves the rows of a query in walk order, the instance of each beside its face; k_scene_tris_rows (no
//    LDS) orders them by (instance, face).
//  * The loop is linear in the number of instances: there is no structure over them.
#include <string>

#include "tr_internal.h"
#include "tr_scene_tris.h"
#include "tr_scene_handle.h"
#include "../../include/triro_scene_tris.h"

namespace {

constexpr int ST_BS = TR_LANE_BS;      // one query triangle per lane, two waves per workgroup

// a value that is the same in every lane, held in an SGPR from here on (all lanes are active where this is called)
__device__ __forceinline__ float st_uniform(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ uint32_t st_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// a value that is the same in every lane, held in a VGPR all the same
__device__ __forceinline__ uint32_t st_lanes(uint32_t x) {
    asm volatile("" : "+v"(x));
    return x;
}
// how many of the nine corner masks sit in SGPRs (the first ones), the rest in VGPRs: see the head of this file
template <int MODE>
constexpr int ST_MASKS_IN_SGPRS = MODE == TR_TRIS_FILL ? 6 : 4;

}  // namespace

// ANY: out8[i] = 0 / 1.  COUNT: out32[i] = the number of pairs over all instances.  FILL: the pairs of query i, in walk
// order, at rows offsets[i] .. of inst and face, at most tr_rows_limit of them.
template <int MODE>
__global__ __launch_bounds__(ST_BS) void k_scene_tris(const tr_scene_member* __restrict__ members, const tr_scene_inst* __restrict__ insts,
                                                      int32_t ninst, const float* __restrict__ tri, int64_t n, uint8_t* __restrict__ out8,
                                                      int32_t* __restrict__ out32, const int32_t* __restrict__ count,
                                                      const int64_t* __restrict__ offsets, int64_t total, int32_t* __restrict__ inst,
                                                      int32_t* __restrict__ face, int stack_entries) {
    __shared__ int32_t stack_lds[TR_TRIS_STACK * ST_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, ST_BS};
    const int64_t i = (int64_t)blockIdx.x * ST_BS + threadIdx.x;
    const bool in_range = i < n;
    tr_tris_q q;
    q.px = 0.f; q.py = 0.f; q.pz = 0.f; q.qx = 0.f; q.qy = 0.f; q.qz = 0.f; q.rx = 0.f; q.ry = 0.f; q.rz = 0.f;      // (no area)
    if (in_range) {
        const float* p = tri + 9 * i;
        q.px = p[0]; q.py = p[1]; q.pz = p[2]; q.qx = p[3]; q.qy = p[4]; q.qz = p[5]; q.rx = p[6]; q.ry = p[7]; q.rz = p[8];
    }
    const bool live = in_range && tr_tris_live(q);
    const tr_box qb = tr_tris_box(q);
    tr_boxes_acc acc = {0, 0, nullptr};
    int32_t* irow = nullptr;
    if (MODE == TR_TRIS_FILL && in_range) {
        const int64_t off = offsets[i];
        acc.limit = tr_rows_limit(count[i], off, total);
        if (acc.limit > 0) { acc.key = face + off; irow = inst + off; }
    }
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_TRIS_STACK);
#pragma unroll 1
    for (int32_t k = 0; k < ninst; k++) {      // (wave-uniform)
        if (!TR_WAVE_ANY(live && !tr_set_full<MODE>(acc))) break;      // no lane has anything left to find
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        tr_scene_near_map M;
        tr_scene_near_map_make(rec.M, M);
#pragma unroll
        for (int j = 0; j < 12; j++) M.M[j] = st_uniform(M.M[j]);
#pragma unroll
        for (int j = 0; j < 9; j++) M.hi[j] = j < ST_MASKS_IN_SGPRS<MODE> ? st_uniform(M.hi[j]) : st_lanes(M.hi[j]);
        const tr_scene_tris_probe<MODE> probe = {b, M, q, qb, acc};
        const bool walk = live && !probe.done();
        const int32_t c0 = acc.count;
        if (b.num_tris >= 2) {      // (wave-uniform)
            tr_walk_state st;
            st.node = walk ? 0 : -1; st.sp = 0;
            for (;;) {
                if (!TR_WAVE_ANY(st.node >= 0)) break;
                if (st.node >= 0) probe.visit(st, stack, cap2);
                TR_CONVERGE();
            }
            tr_scene_tris_again<MODE>(b, probe, st.sp, c0);
        } else if (walk) {
            probe.leaf(0);      // no hierarchy below two triangles
        }
        if (MODE == TR_TRIS_FILL && irow) tr_scene_tris_mark(acc, irow, c0, k);
        TR_CONVERGE();
    }
    if (in_range) {
        if (MODE == TR_TRIS_ANY) out8[i] = acc.count > 0 ? 1 : 0;
        if (MODE == TR_TRIS_COUNT) out32[i] = acc.count;
    }
}

// after k_scene_tris<FILL>: the rows of query i into ascending (instance, face) order
__global__ __launch_bounds__(ST_BS) void k_scene_tris_rows(int64_t n, const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                           int64_t total, int32_t* __restrict__ inst, int32_t* __restrict__ face) {
    const int64_t i = (int64_t)blockIdx.x * ST_BS + threadIdx.x;
    if (i >= n) return;
    const int64_t off = offsets[i];
    const int32_t m = tr_rows_limit(count[i], off, total);
    if (m <= 0) return;
    tr_scene_tris_rows(inst + off, face + off, m);
}

namespace {

// the checks every entry shares (those of tr_lane_check on a scene, without the stale check: the caller makes it after its own
// argument checks); nblocks comes back
int st_check(const tr_scene* scene, const float* d_tri, int64_t n, const void* d_required, int stack_entries, int64_t& nblocks) {
    if (!scene) return tr_fail(TR_ERR_INVALID_ARG, "scene == NULL");
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    if (stack_entries < 0 || stack_entries > TR_TRIS_STACK)
        return tr_fail(TR_ERR_INVALID_ARG, "stack_entries must be 0 (all) or 1 .. " + std::to_string(TR_TRIS_STACK));
    if (n > 0 && (!d_tri || !d_required)) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    nblocks = (n + ST_BS - 1) / ST_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many triangles for one launch");
    return TR_OK;
}

template <int MODE>
int st_launch(const tr_scene* scene, const float* d_tri, int64_t n, uint8_t* out8, int32_t* out32, const int32_t* d_count,
              const int64_t* d_offsets, int64_t total, int32_t* d_instance, int32_t* d_face, int stack_entries, int64_t nblocks, void* stream) {
    hipLaunchKernelGGL(k_scene_tris<MODE>, dim3((unsigned)nblocks), dim3(ST_BS), 0, (hipStream_t)stream, scene->d_members, scene->d_insts,
                       (int32_t)scene->ninst, d_tri, n, out8, out32, d_count, d_offsets, total, d_instance, d_face, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_scene_tris_abi_version(void) { return TR_SCENE_TRIS_ABI_VERSION; }

int tr_scene_tris_stack_capacity(void) { return TR_TRIS_STACK; }

int tr_scene_tris_any(const tr_scene* scene, const float* d_tri, int64_t n, uint8_t* d_any, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = st_check(scene, d_tri, n, d_any, stack_entries, nblocks)) return rc;
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    return st_launch<TR_TRIS_ANY>(scene, d_tri, n, d_any, nullptr, nullptr, nullptr, 0, nullptr, nullptr, stack_entries, nblocks, stream);
}

int tr_scene_tris_count(const tr_scene* scene, const float* d_tri, int64_t n, int32_t* d_count, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = st_check(scene, d_tri, n, d_count, stack_entries, nblocks)) return rc;
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    return st_launch<TR_TRIS_COUNT>(scene, d_tri, n, nullptr, d_count, nullptr, nullptr, 0, nullptr, nullptr, stack_entries, nblocks, stream);
}

int tr_scene_tris_fill(const tr_scene* scene, const float* d_tri, int64_t n, const int32_t* d_count, const int64_t* d_offsets, int64_t total,
                       int32_t* d_instance, int32_t* d_face, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = st_check(scene, d_tri, n, d_count, stack_entries, nblocks)) return rc;
    TR_TRY(tr_fill_check(n, total, d_offsets, d_instance != nullptr && d_face != nullptr, "null pointer argument (d_instance, d_face)"));
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    if (int rc = st_launch<TR_TRIS_FILL>(scene, d_tri, n, nullptr, nullptr, d_count, d_offsets, total, d_instance, d_face, stack_entries, nblocks,
                                         stream))
        return rc;
    hipLaunchKernelGGL(k_scene_tris_rows, dim3((unsigned)nblocks), dim3(ST_BS), 0, (hipStream_t)stream, n, d_count, d_offsets, total, d_instance,
                       d_face);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
