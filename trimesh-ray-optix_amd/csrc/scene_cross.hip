// scene_cross.hip -- libtriro_scene_cross.so (include/triro_scene_cross.h): every crossing of a world ray over placed copies
// of several meshes on a per-ray interval [tmin, tmax]: the count, and the uncapped ordered list.
//
// The contract, the overflow rule and the row order are csrc/tr_scene_cross.h (host + device), on the instance records and
// the transform of csrc/tr_scene.h and the crossing walk of csrc/tr_cross.h; this file is the wave-uniform instance loop
// around the wave loop of tr_cross_visit, the launches and the C entries.  The scene is libtriro_scene.so's: this library
// reads the committed table of the opaque handle (csrc/tr_scene_handle.h) and never changes it.
//
//  * One ray per lane, block k takes rays 128 k ... 128 k + 127 (64-bit index math), rays read through RayFetch / fetch_ray
//    of kernels_common.inc, the stack a column of LDS (TR_CROSS_STACK node ids, 16 KB per workgroup): the shape of k_cross.
//  * THE INSTANCE LOOP IS WAVE-UNIFORM, as in k_scene_query: every lane of a wave visits instance k at the same time, so the
//    instance record and the member's pointers are uniform loads and the member walk is the wave loop of cross.hip.  A lane
//    that cannot cross the instance (an invalid ray, a transformed ray out of the float32 range, a FILL ray whose rows are
//    full) starts the walk without a node.  A lane whose stack overflowed drops what it found IN THAT INSTANCE and repeats
//    that instance without a stack before the wave moves on.
//  * k_scene_cross<FILL> leaves the rows of a ray in walk order, the instance of each beside its face; k_scene_cross_rows
//    (no LDS) orders them by (t, instance, face) and evaluates the optional front / loc / uv / ray rows.
//  * The loop is linear in the number of instances: there is no structure over them.
#include <string>

#include "tr_internal.h"
#include "tr_scene_cross.h"
#include "tr_scene_handle.h"
#include "../../include/triro_scene_cross.h"

namespace {

#include "kernels_common.inc"

constexpr int SX_BS = 128;      // one ray per lane, two waves per workgroup

}  // namespace

// COUNT: out32[i] = the number of crossings over all instances.  FILL: the crossings of ray i, in walk order, at rows
// offsets[i] .. of inst, face and t (and their arena slots at the same rows of slot, where given), at most tr_rows_limit.
template <int MODE>
__global__ __launch_bounds__(SX_BS) void k_scene_cross(const tr_scene_member* __restrict__ members,
                                                       const tr_scene_inst* __restrict__ insts, int32_t ninst, RayFetch rf,
                                                       const float* __restrict__ tmin, const float* __restrict__ tmax,
                                                       int32_t* __restrict__ out32, const int32_t* __restrict__ count,
                                                       const int64_t* __restrict__ offsets, int64_t total,
                                                       int32_t* __restrict__ inst, int32_t* __restrict__ face, float* __restrict__ t,
                                                       int32_t* __restrict__ slot, int stack_entries) {
    __shared__ int32_t stack_lds[TR_CROSS_STACK * SX_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, SX_BS};
    const int64_t i = (int64_t)blockIdx.x * SX_BS + threadIdx.x;
    const bool in_range = i < rf.n;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, lo = 0.0f, hi = TR_TMAX;
    if (in_range) {
        fetch_ray(rf, i, o, d);
        if (tmin) lo = tmin[i];
        if (tmax) hi = tmax[i];
    }
    bool valid;
    {
        tr_ray rw;
        valid = tr_ray_setup(rw, o[0], o[1], o[2], d[0], d[1], d[2]);
    }
    valid = tr_range_bounds(lo, hi, lo, hi) && valid && in_range;
    tr_cross_acc acc;
    acc.count = 0; acc.limit = 0; acc.face = nullptr; acc.t = nullptr; acc.slot = nullptr;
    int32_t* irow = nullptr;
    if (MODE == TR_CROSS_FILL && in_range) {
        const int64_t off = offsets[i];
        acc.limit = tr_rows_limit(count[i], off, total);
        if (acc.limit > 0) { acc.face = face + off; acc.t = t + off; acc.slot = slot ? slot + off : nullptr; irow = inst + off; }
    }
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_CROSS_STACK);
#pragma unroll 1
    for (int32_t k = 0; k < ninst; k++) {      // (wave-uniform)
        if (!TR_WAVE_ANY(valid && !tr_cross_full<MODE>(acc))) break;      // no lane is valid with rows left
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        tr_ray r;
        const bool live = tr_scene_ray(rec, o[0], o[1], o[2], d[0], d[1], d[2], r) && valid && !tr_cross_full<MODE>(acc);
        const int32_t c0 = acc.count;
        if (b.num_tris >= 2) {      // (wave-uniform)
            tr_cross_state st;
            st.node = live ? 0 : -1; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
            for (;;) {
                if (!TR_WAVE_ANY(st.node >= 0)) break;
                if (st.node >= 0) tr_cross_visit<MODE>(b, r, lo, hi, st, acc, stack, cap2);
                TR_CONVERGE();
            }
            if (tr_walk_lost(st.sp) && !tr_cross_full<MODE>(acc)) {      // cold: this instance's part is dropped, not added to
                acc.count = c0;
                tr_rewalk(b, tr_cross_probe<MODE>{b, r, lo, hi, acc});
            }
        } else if (live) {
            tr_scene_cross_single<MODE>(b, r, lo, hi, acc);      // no hierarchy below two triangles
        }
        if (MODE == TR_CROSS_FILL && irow) tr_scene_cross_mark(acc, irow, c0, k);
        TR_CONVERGE();
    }
    if (MODE == TR_CROSS_COUNT && in_range) out32[i] = acc.count;
}

// after k_scene_cross<FILL>: the rows of ray i into ascending (t, instance, face) order, then the optional outputs of each row
__global__ __launch_bounds__(SX_BS) void k_scene_cross_rows(const tr_scene_member* __restrict__ members,
                                                            const tr_scene_inst* __restrict__ insts, int32_t ninst, RayFetch rf,
                                                            const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                            int64_t total, int32_t* __restrict__ inst, int32_t* __restrict__ face,
                                                            float* __restrict__ t, int32_t* __restrict__ slot, uint8_t* __restrict__ front,
                                                            float* __restrict__ loc, float* __restrict__ uv, int64_t* __restrict__ ray,
                                                            int64_t ray_base) {
    const int64_t i = (int64_t)blockIdx.x * SX_BS + threadIdx.x;
    if (i >= rf.n) return;
    const int64_t off = offsets[i];
    const int32_t m = tr_rows_limit(count[i], off, total);
    if (m <= 0) return;
    float o[3], d[3];
    fetch_ray(rf, i, o, d);
    tr_scene_cross_rows(members, insts, ninst, o[0], o[1], o[2], d[0], d[1], d[2], inst + off, face + off, t + off, slot ? slot + off : nullptr,
                        m, front ? front + off : nullptr, loc ? loc + 3 * off : nullptr, uv ? uv + 2 * off : nullptr, ray ? ray + off : nullptr,
                        i + ray_base);
}

namespace {

// the checks every entry shares (those of cross_check and scene_launch, without the stale check: the caller makes it after
// its own argument checks); the RayFetch and nblocks come back
int scene_cross_check(const tr_scene* scene, const tr_rays* rays, const void* required, int stack_entries, RayFetch& rf, int64_t& nblocks) {
    if (!scene) return tr_fail(TR_ERR_INVALID_ARG, "scene == NULL");
    TR_TRY(make_fetch(rays, &rf));
    if (stack_entries < 0 || stack_entries > TR_CROSS_STACK)
        return tr_fail(TR_ERR_INVALID_ARG, "stack_entries must be 0 (all) or 1 .. " + std::to_string(TR_CROSS_STACK));
    if (rf.n > 0 && !required) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    nblocks = (rf.n + SX_BS - 1) / SX_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many rays for one launch");
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_scene_cross_abi_version(void) { return TR_SCENE_CROSS_ABI_VERSION; }

int tr_scene_cross_stack_capacity(void) { return TR_CROSS_STACK; }

int tr_scene_cross_count(const tr_scene* scene, const tr_rays* rays, const float* d_tmin, const float* d_tmax, int32_t* d_count,
                         int stack_entries, void* stream) {
    RayFetch rf;
    int64_t nblocks = 0;
    if (int rc = scene_cross_check(scene, rays, d_count, stack_entries, rf, nblocks)) return rc;
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (rf.n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    hipLaunchKernelGGL((k_scene_cross<TR_CROSS_COUNT>), dim3((unsigned)nblocks), dim3(SX_BS), 0, (hipStream_t)stream, scene->d_members,
                       scene->d_insts, (int32_t)scene->ninst, rf, d_tmin, d_tmax, d_count, nullptr, nullptr, (int64_t)0, nullptr, nullptr,
                       nullptr, nullptr, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

int tr_scene_cross_fill(const tr_scene* scene, const tr_rays* rays, const float* d_tmin, const float* d_tmax, const int32_t* d_count,
                        const int64_t* d_offsets, int64_t total, int32_t* d_instance, int32_t* d_face, float* d_t, uint8_t* d_front,
                        float* d_loc3, float* d_uv2, int64_t* d_ray, int64_t ray_base, int32_t* d_slot, int stack_entries, void* stream) {
    RayFetch rf;
    int64_t nblocks = 0;
    if (int rc = scene_cross_check(scene, rays, d_count, stack_entries, rf, nblocks)) return rc;
    if (total < 0) return tr_fail(TR_ERR_INVALID_ARG, "total < 0");
    if (rf.n > 0 && !d_offsets) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    const bool evaluate = d_front || d_loc3 || d_uv2;
    if (rf.n > 0 && total > 0 && (!d_instance || !d_face || !d_t || (evaluate && !d_slot)))
        return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument (d_instance, d_face, d_t, or d_slot with d_front / d_loc3 / d_uv2)");
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (rf.n == 0 || total == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    if (!evaluate) d_slot = nullptr;
    hipLaunchKernelGGL((k_scene_cross<TR_CROSS_FILL>), dim3((unsigned)nblocks), dim3(SX_BS), 0, (hipStream_t)stream, scene->d_members,
                       scene->d_insts, (int32_t)scene->ninst, rf, d_tmin, d_tmax, nullptr, d_count, d_offsets, total, d_instance, d_face,
                       d_t, d_slot, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_scene_cross_rows, dim3((unsigned)nblocks), dim3(SX_BS), 0, (hipStream_t)stream, scene->d_members, scene->d_insts,
                       (int32_t)scene->ninst, rf, d_count, d_offsets, total, d_instance, d_face, d_t, d_slot, d_front, d_loc3, d_uv2, d_ray,
                       ray_base);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
