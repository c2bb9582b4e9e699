// scene_points.hip -- libtriro_scene_points.so (include/triro_scene_points.h): which placed copies of a scene's members hold a
// point: any, count, and the ascending list of instance indices.
//
// The contract, the shortcut and the overflow rule are csrc/tr_scene_points.h (host + device), on the instance records and
// the transform of csrc/tr_scene.h, the crossing walk of csrc/tr_cross.h and the parity rule of csrc/tr_points.h; this file is
// the wave-uniform instance loop around the two passes of a point, the launches and the C entries.  The scene is
// libtriro_scene.so's: this library reads the committed table of the opaque handle (csrc/tr_scene_handle.h) and never
// changes it.
//
//  * One point per lane, block k takes points 128 k ... 128 k + 127 (64-bit index math), the stack a column of LDS
//    (TR_CROSS_STACK node ids, 16 KB per workgroup): the shape of k_scene_cross.
//  * THE INSTANCE LOOP IS WAVE-UNIFORM, as in k_scene_cross: every lane of a wave visits instance k at the same time, so the
//    instance record and the member's pointers are uniform loads.  Both rays of a point run in the SAME lane, +d then -d
//    (points.hip: neighbouring points with one direction walk the same nodes), each pass the wave loop of cross.hip with a
//    counter of its own.  A lane enters the second pass without a node unless its first count is odd; a wave in which no
//    lane's first count is odd skips the pass.
//  * Every point of a call has the same world direction, so the object-space direction W_lin (+-d) and everything
//    tr_ray_setup derives from it alone are the same in every lane: computed once per instance and pass and pinned to SGPRs
//    (sp_uniform, as pt_uniform of points.hip).  Only the origin differs per lane.
//  * A lane whose stack overflowed in a pass drops that pass's count and repeats that pass without a stack before the wave
//    moves on.
//  * FILL writes a containing instance straight into the point's rows: instances are visited in ascending order, so the rows
//    are ascending as written and there is no ordering launch.
//  * The loop is linear in the number of instances: there is no structure over them.
#include <string>

#include "tr_internal.h"
#include "tr_scene_points.h"
#include "tr_scene_handle.h"
#include "../../include/triro_scene_points.h"

namespace {

constexpr int SP_BS = 128;      // one point per lane, two waves per workgroup

// a value that is the same in every lane, held in an SGPR from here on (all lanes are active where this is called)
__device__ __forceinline__ float sp_uniform(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

}  // namespace

// ANY: out8[i] = the point is inside some instance.  COUNT: out32[i] = the number of instances it is inside.  FILL: those
// instances, ascending, at rows offsets[i] .. of inst, at most tr_rows_limit(count[i], offsets[i], total) of them.
template <int MODE>
__global__ __launch_bounds__(SP_BS) void k_scene_points(const tr_scene_member* __restrict__ members,
                                                        const tr_scene_inst* __restrict__ insts, int32_t ninst,
                                                        const float* __restrict__ points, int64_t n, const float* __restrict__ dir3,
                                                        uint8_t* __restrict__ out8, int32_t* __restrict__ out32,
                                                        const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                        int64_t total, int32_t* __restrict__ inst, int stack_entries) {
    __shared__ int32_t stack_lds[TR_CROSS_STACK * SP_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, SP_BS};
    const int64_t i = (int64_t)blockIdx.x * SP_BS + threadIdx.x;
    const bool in_range = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (in_range) { px = points[3 * i]; py = points[3 * i + 1]; pz = points[3 * i + 2]; }
    const float d0 = dir3[0], d1 = dir3[1], d2 = dir3[2];      // (uniform addresses: scalar loads)
    const bool valid = tr_scene_points_valid(px, py, pz, d0, d1, d2) && in_range;
    tr_scene_points_acc acc;
    acc.count = 0; acc.limit = 0; acc.inst = nullptr;
    if (MODE == TR_SCENE_POINTS_FILL && in_range) {
        const int64_t off = offsets[i];
        acc.limit = tr_rows_limit(count[i], off, total);
        if (acc.limit > 0) acc.inst = inst + off;
    }
    float lo, hi;
    (void)tr_range_bounds(0.0f, TR_TMAX, lo, hi);
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_CROSS_STACK);
#pragma unroll 1
    for (int32_t k = 0; k < ninst; k++) {      // (wave-uniform)
        if (!TR_WAVE_ANY(valid && !tr_scene_points_done<MODE>(acc))) break;      // no lane is unfinished
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        bool go = valid && !tr_scene_points_done<MODE>(acc);
        int32_t cp = 0, cm = 0;
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {      // (wave-uniform)
            tr_ray r;
            const bool live = tr_scene_points_ray(rec, px, py, pz, d0, d1, d2, pass, r) && go;
            r.dx = sp_uniform(r.dx); r.dy = sp_uniform(r.dy); r.dz = sp_uniform(r.dz);
            r.ix = sp_uniform(r.ix); r.iy = sp_uniform(r.iy); r.iz = sp_uniform(r.iz);
            r.kd = sp_uniform(r.kd);
            tr_cross_acc ca;      // the counter of this instance and this pass
            ca.count = 0; ca.limit = 0; ca.face = nullptr; ca.t = nullptr; ca.slot = nullptr;
            if (b.num_tris >= 2) {      // (wave-uniform)
                tr_cross_state st;
                st.node = live ? 0 : -1; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
                for (;;) {
                    if (!TR_WAVE_ANY(st.node >= 0)) break;
                    if (st.node >= 0) tr_cross_visit<TR_CROSS_COUNT>(b, r, lo, hi, st, ca, stack, cap2);
                    TR_CONVERGE();
                }
                if (tr_walk_lost(st.sp)) {      // cold: this pass's count is dropped, not added to
                    ca.count = 0;
                    tr_rewalk(b, tr_cross_probe<TR_CROSS_COUNT>{b, r, lo, hi, ca});
                }
            } else if (live) {
                tr_scene_cross_single<TR_CROSS_COUNT>(b, r, lo, hi, ca);      // no hierarchy below two triangles
            }
            TR_CONVERGE();
            if (pass == 0) {
                cp = ca.count;
                go = go && tr_scene_points_second(cp);      // THE SHORTCUT: an even first count decides
                if (!TR_WAVE_ANY(go)) break;
            } else {
                cm = ca.count;
            }
        }
        if (tr_scene_points_inside(cp, cm)) tr_scene_points_record<MODE>(acc, k);
        TR_CONVERGE();
    }
    if (in_range) {
        if (MODE == TR_SCENE_POINTS_ANY) out8[i] = acc.count > 0 ? 1 : 0;
        if (MODE == TR_SCENE_POINTS_COUNT) out32[i] = acc.count;
    }
}

namespace {

// the checks every entry shares (without the stale check: the caller makes it after its own argument checks)
int scene_points_check(const tr_scene* scene, const float* d_points, int64_t n, const float* d_dir3, const void* required, int stack_entries,
                       int64_t& nblocks) {
    if (!scene) return tr_fail(TR_ERR_INVALID_ARG, "scene == NULL");
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    nblocks = (n + SP_BS - 1) / SP_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many points for one launch");
    if (n > 0 && (!d_points || !d_dir3 || !required)) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    if (stack_entries < 0 || stack_entries > TR_CROSS_STACK)
        return tr_fail(TR_ERR_INVALID_ARG, "stack_entries must be 0 (all) or 1 .. " + std::to_string(TR_CROSS_STACK));
    return TR_OK;
}

template <int MODE>
int scene_points_launch(const tr_scene* scene, const float* d_points, int64_t n, const float* d_dir3, uint8_t* d_any, int32_t* d_out,
                        const int32_t* d_count, const int64_t* d_offsets, int64_t total, int32_t* d_instance, int stack_entries,
                        int64_t nblocks, void* stream) {
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    hipLaunchKernelGGL((k_scene_points<MODE>), dim3((unsigned)nblocks), dim3(SP_BS), 0, (hipStream_t)stream, scene->d_members,
                       scene->d_insts, (int32_t)scene->ninst, d_points, n, d_dir3, d_any, d_out, d_count, d_offsets, total, d_instance,
                       stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_scene_points_abi_version(void) { return TR_SCENE_POINTS_ABI_VERSION; }

int tr_scene_points_stack_capacity(void) { return TR_CROSS_STACK; }

int tr_scene_points_any(const tr_scene* scene, const float* d_points, int64_t n, const float* d_dir3, uint8_t* d_any, int stack_entries,
                        void* stream) {
    int64_t nblocks = 0;
    if (int rc = scene_points_check(scene, d_points, n, d_dir3, d_any, stack_entries, nblocks)) return rc;
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (n == 0) return TR_OK;
    return scene_points_launch<TR_SCENE_POINTS_ANY>(scene, d_points, n, d_dir3, d_any, nullptr, nullptr, nullptr, 0, nullptr, stack_entries,
                                                    nblocks, stream);
}

int tr_scene_points_count(const tr_scene* scene, const float* d_points, int64_t n, const float* d_dir3, int32_t* d_count, int stack_entries,
                          void* stream) {
    int64_t nblocks = 0;
    if (int rc = scene_points_check(scene, d_points, n, d_dir3, d_count, stack_entries, nblocks)) return rc;
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (n == 0) return TR_OK;
    return scene_points_launch<TR_SCENE_POINTS_COUNT>(scene, d_points, n, d_dir3, nullptr, d_count, nullptr, nullptr, 0, nullptr,
                                                      stack_entries, nblocks, stream);
}

int tr_scene_points_fill(const tr_scene* scene, const float* d_points, int64_t n, const float* d_dir3, const int32_t* d_count,
                         const int64_t* d_offsets, int64_t total, int32_t* d_instance, int stack_entries, void* stream) {
    int64_t nblocks = 0;
    if (int rc = scene_points_check(scene, d_points, n, d_dir3, d_count, stack_entries, nblocks)) return rc;
    if (total < 0) return tr_fail(TR_ERR_INVALID_ARG, "total < 0");
    if (n > 0 && !d_offsets) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    if (n > 0 && total > 0 && !d_instance) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument (d_instance)");
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (n == 0 || total == 0) return TR_OK;
    return scene_points_launch<TR_SCENE_POINTS_FILL>(scene, d_points, n, d_dir3, nullptr, nullptr, d_count, d_offsets, total, d_instance,
                                                     stack_entries, nblocks, stream);
}

}  // extern "C"
