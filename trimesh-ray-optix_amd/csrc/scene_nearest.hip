// scene_nearest.hip -- libtriro_scene_nearest.so (include/triro_scene_nearest.h): closest_point over the placed copies of a
// scene's members as one launch: the nearest placed triangle, which instance it belongs to, the closest point and the distance.
//
// The contract, the culling bound with its proof and the rule that carries the best between instances are
// csrc/tr_scene_nearest.h (host + device), on the instance records and the placement chain of csrc/tr_scene.h and the
// per-triangle function, box bound and far-child stack of csrc/tr_nearest.h; this file is the wave-uniform instance loop
// around the wave loops of an instance's walk, the launch and the C entry.  The scene is libtriro_scene.so's: this library
// reads the committed table of the opaque handle (csrc/tr_scene_handle.h) and never changes it.
//
//  * One point per lane, block k takes points 128 k ... 128 k + 127 (64-bit index math), the far-child stack a column of LDS
//    (TR_NEAR_STACK entries of {node, float32 bound}, 32 KB per workgroup): the shape of k_closest_point.
//  * THE INSTANCE LOOP IS WAVE-UNIFORM, as in k_scene_query: every lane of a wave visits instance k at the same time, so the
//    record and the member's pointers are uniform loads and the twelve entries of M stay in SGPRs (sn_uniform).  The nine
//    corner masks of the placed bound (tr_scene_near_map) are kept in VGPRs (sn_lanes): one v_bfi_b32 per chosen corner.
//  * The cull of an instance is the first visit of its root: the placed boxes of the root's children against the best so far.
//  * The seed descent runs only for lanes whose best is still +Inf (the first instance that offers anything, unbounded).
//  * A lane whose stack overflowed in an instance walks that instance again without a stack before the wave moves on.
//  * The loop is linear in the number of instances: there is no structure over them.
#include <string>

#include "tr_internal.h"
#include "tr_scene_nearest.h"
#include "tr_scene_handle.h"
#include "../../include/triro_scene_nearest.h"

namespace {

constexpr int SN_BS = 128;      // one point per lane, two waves per workgroup

// a value that is the same in every lane, held in an SGPR from here on (all lanes are active where this is called)
__device__ __forceinline__ float sn_uniform(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
// a value that is the same in every lane, held in a VGPR all the same: the nine corner masks are the third operand of a
// v_bfi_b32 there.  As conditions in SGPRs they are nine 64-bit lane masks, eighteen SGPRs that the kernel does not have.
__device__ __forceinline__ uint32_t sn_lanes(uint32_t x) {
    asm volatile("" : "+v"(x));
    return x;
}

}  // namespace

__global__ __launch_bounds__(SN_BS) void k_scene_closest_point(const tr_scene_member* __restrict__ members,
                                                               const tr_scene_inst* __restrict__ insts, int32_t ninst,
                                                               const float* __restrict__ points, int64_t n,
                                                               const float* __restrict__ max_distance, float max_distance_all,
                                                               float* __restrict__ closest, float* __restrict__ distance,
                                                               int32_t* __restrict__ inst, int32_t* __restrict__ tri, int stack_entries) {
    __shared__ int32_t stack_lds[2 * TR_NEAR_STACK * SN_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, SN_BS};
    const int64_t i = (int64_t)blockIdx.x * SN_BS + threadIdx.x;
    const bool in_range = i < n;
    float px = 0.f, py = 0.f, pz = 0.f, r = max_distance_all;
    if (in_range) {
        px = points[3 * i]; py = points[3 * i + 1]; pz = points[3 * i + 2];
        if (max_distance) r = max_distance[i];
    }
    const bool valid = in_range && tr_scene_near_valid(px, py, pz, r);
    tr_scene_near_best g;
    tr_scene_near_init(g, tr_within_r2(r));
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_NEAR_STACK);
    if (TR_WAVE_ANY(valid)) {
#pragma unroll 1
        for (int32_t k = 0; k < ninst; k++) {      // (wave-uniform)
            const tr_scene_inst& rec = insts[k];
            if (!(rec.flags & TR_SCENE_VALID)) continue;
            const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
            tr_scene_near_map M;
            tr_scene_near_map_make(rec.M, M);
#pragma unroll
            for (int j = 0; j < 12; j++) M.M[j] = sn_uniform(M.M[j]);
#pragma unroll
            for (int j = 0; j < 9; j++) M.hi[j] = sn_lanes(M.hi[j]);
            tr_near_best best;
            tr_scene_near_seed_best(g, k, best);
            if (b.num_tris >= 2) {      // (wave-uniform)
                // the seed descent: a finite best before the first push, for the lanes that have none yet
                for (int32_t node = (valid && best.d2 == INFINITY) ? 0 : -1;;) {
                    if (!TR_WAVE_ANY(node >= 0)) break;
                    if (node >= 0) node = tr_scene_near_seed(b, M, node, px, py, pz, best);
                    TR_CONVERGE();
                }
                tr_near_state st;
                st.node = valid ? 0 : -1; st.sp = 0;
                for (;;) {
                    if (!TR_WAVE_ANY(st.node >= 0)) break;
                    if (st.node >= 0) tr_scene_near_visit(b, M, px, py, pz, st, best, stack, cap2);
                    TR_CONVERGE();
                }
                if (tr_near_lost(st.sp)) tr_rewalk(b, tr_scene_near_probe{b, M, px, py, pz, best});      // cold
            } else if (valid) {
                tr_scene_near_leaf(b, M, 0, px, py, pz, best);      // no hierarchy below two triangles
            }
            TR_CONVERGE();
            tr_scene_near_take(best, k, g);
        }
    }
    if (in_range)
        tr_scene_near_outputs(members, insts, px, py, pz, valid, g, closest ? closest + 3 * i : nullptr, distance ? distance + i : nullptr,
                              inst + i, tri + i);
}

extern "C" {

int tr_scene_nearest_abi_version(void) { return TR_SCENE_NEAREST_ABI_VERSION; }

int tr_scene_nearest_stack_capacity(void) { return TR_NEAR_STACK; }

int tr_scene_closest_point(const tr_scene* scene, const float* d_points, int64_t n, const float* d_max_distance, float max_distance,
                           float* d_closest, float* d_distance, int32_t* d_instance, int32_t* d_tri, int stack_entries, void* stream) {
    if (!scene) return tr_fail(TR_ERR_INVALID_ARG, "scene == NULL");
    if (n < 0) return tr_fail(TR_ERR_INVALID_ARG, "n < 0");
    const int64_t nblocks = (n + SN_BS - 1) / SN_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many points for one launch");
    if (n > 0 && (!d_points || !d_instance || !d_tri)) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    if (stack_entries < 0 || stack_entries > TR_NEAR_STACK)
        return tr_fail(TR_ERR_INVALID_ARG, "stack_entries must be 0 (all) or 1 .. " + std::to_string(TR_NEAR_STACK));
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    hipLaunchKernelGGL(k_scene_closest_point, dim3((unsigned)nblocks), dim3(SN_BS), 0, (hipStream_t)stream, scene->d_members, scene->d_insts,
                       (int32_t)scene->ninst, d_points, n, d_max_distance, max_distance, d_closest, d_distance, d_instance, d_tri,
                       stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // extern "C"
