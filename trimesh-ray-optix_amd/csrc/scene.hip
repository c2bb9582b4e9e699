// scene.hip -- libtriro_scene.so (include/triro_scene.h): any / closest over placed copies of several meshes, one launch each.
//
// The contract, the inverse, the transform and the argument for carrying the best hit from instance to instance are
// csrc/tr_scene.h (host + device); the walk of one instance is csrc/tr_range.h's.  This file is the wave-uniform instance
// loop around it, the launch, the commit and the C entries.
//
//  * One ray per lane, block k takes rays 128 k ... 128 k + 127 (64-bit index math), rays read through RayFetch / fetch_ray
//    of kernels_common.inc, the far-child stack a column of LDS (TR_RANGE_STACK entries, 32 KB per workgroup): the shape
//    of k_range_query.
//  * THE INSTANCE LOOP IS WAVE-UNIFORM: every lane of a wave visits instance k at the same time, so the instance record and
//    the member's pointers are uniform loads and the member walk is the wave loop of range.hip.  A lane that cannot hit
//    the instance (an invalid ray, a transformed ray out of the float32 range, an any-ray that has its hit) starts the walk
//    without a node.  A lane whose stack overflowed repeats THAT instance without a stack before the wave moves on.
//  * Instances that cannot be hit (tr_scene.h, contract 2) are skipped by a flag computed at commit.
//  * There is no world-space structure over the instances: the cull of an instance is the first visit's test of the root's
//    two child boxes against the object-space ray.  The loop is linear in the number of instances.
#include <string.h>
#include <string>
#include <vector>

#include "tr_internal.h"
#include "tr_scene.h"
#include "tr_scene_handle.h"      // struct tr_scene and scene_stale
#include "../../include/triro_scene.h"

namespace {

#include "kernels_common.inc"

constexpr int SC_BS = 128;      // one ray per lane, two waves per workgroup

struct SceneOut {
    uint8_t* hit;
    uint8_t* front;
    int32_t* inst;
    int32_t* tri;
    float* t;
    float* loc;
    float* uv;
};

}  // namespace

template <int Q>
__global__ __launch_bounds__(SC_BS) void k_scene_query(const tr_scene_member* __restrict__ members,
                                                       const tr_scene_inst* __restrict__ insts, int32_t ninst, RayFetch rf,
                                                       const float* __restrict__ tmin, const float* __restrict__ tmax,
                                                       SceneOut out, int stack_entries) {
    __shared__ int32_t stack_lds[2 * TR_RANGE_STACK * SC_BS];
    const tr_ring stack = {stack_lds + threadIdx.x, SC_BS};
    const int64_t i = (int64_t)blockIdx.x * SC_BS + threadIdx.x;
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
    tr_scene_best g;
    tr_scene_init(g);
    const uint32_t cap2 = 2u * (uint32_t)(stack_entries > 0 ? stack_entries : TR_RANGE_STACK);
#pragma unroll 1
    for (int32_t k = 0; k < ninst; k++) {      // (wave-uniform)
        if (!TR_WAVE_ANY(valid && !(Q == TR_Q_ANY && g.slot >= 0))) break;      // nothing left to find for this wave
        const tr_scene_inst& rec = insts[k];
        if (!(rec.flags & TR_SCENE_VALID)) continue;
        const tr_bvh_view b = tr_scene_view(members[rec.mesh]);
        tr_ray r;
        const bool live = tr_scene_ray(rec, o[0], o[1], o[2], d[0], d[1], d[2], r) && valid && !(Q == TR_Q_ANY && g.slot >= 0);
        tr_range_best best;
        tr_scene_seed<Q>(g, k, best);
        if (b.num_tris >= 2) {
            tr_range_state st;
            st.node = live ? 0 : -1; st.sp = 0; st.pe0 = -1; st.pe1 = -1;
            for (;;) {
                if (!TR_WAVE_ANY(st.node >= 0)) break;
                if (st.node >= 0) tr_range_visit<Q>(b, r, lo, hi, st, best, stack, cap2);
                TR_CONVERGE();
            }
            if (tr_range_lost(st.sp)) tr_rewalk(b, tr_range_probe<Q>{b, r, lo, hi, best});
        } else if (live) {
            tr_scene_single(b, r, lo, hi, best);      // no hierarchy below two triangles
        }
        tr_scene_take(best, k, g);
        TR_CONVERGE();
    }
    if (in_range)
        tr_scene_outputs(members, insts, o[0], o[1], o[2], d[0], d[1], d[2], valid, g, out.hit ? out.hit + i : nullptr,
                         out.front ? out.front + i : nullptr, out.inst ? out.inst + i : nullptr, out.tri ? out.tri + i : nullptr,
                         out.t ? out.t + i : nullptr, out.loc ? out.loc + 3 * i : nullptr, out.uv ? out.uv + 2 * i : nullptr);
}

namespace {

tr_scene_member member_of(const tr_bvh* b) {
    tr_scene_member m;
    m.nodes = b->nodes; m.links = b->links; m.tris = b->tris; m.num_tris = b->num_tris;
    return m;
}

template <int Q>
int scene_launch(const tr_scene* scene, const tr_rays* rays, const float* d_tmin, const float* d_tmax, const SceneOut& out,
                 const void* required, int stack_entries, void* stream) {
    if (!scene) return tr_fail(TR_ERR_INVALID_ARG, "scene == NULL");
    RayFetch rf;
    TR_TRY(make_fetch(rays, &rf));
    if (stack_entries < 0 || stack_entries > TR_RANGE_STACK)
        return tr_fail(TR_ERR_INVALID_ARG, "stack_entries must be 0 (all) or 1 .. " + std::to_string(TR_RANGE_STACK));
    if (rf.n > 0 && !required) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    const int64_t nblocks = (rf.n + SC_BS - 1) / SC_BS;
    if (nblocks > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many rays for one launch");
    if (scene_stale(scene)) return tr_fail(TR_ERR_INVALID_ARG, "scene is stale: commit it again");
    if (rf.n == 0) return TR_OK;
    tr_device_guard guard;
    TR_TRY(tr_enter_device(&guard, scene->device));
    hipLaunchKernelGGL((k_scene_query<Q>), dim3((unsigned)nblocks), dim3(SC_BS), 0, (hipStream_t)stream, scene->d_members,
                       scene->d_insts, (int32_t)scene->ninst, rf, d_tmin, d_tmax, out, stack_entries);
    TR_HIP_TRY(hipGetLastError());
    return TR_OK;
}

}  // namespace

extern "C" {

int tr_scene_abi_version(void) { return TR_SCENE_ABI_VERSION; }

int tr_scene_create(int device, tr_scene** out) {
    if (!out) return tr_fail(TR_ERR_INVALID_ARG, "out == NULL");
    *out = nullptr;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return tr_fail(TR_ERR_NO_DEVICE, "hipGetDevice failed");
    tr_scene* s = new tr_scene();
    s->device = device;
    *out = s;
    return TR_OK;
}

int tr_scene_destroy(tr_scene* scene) {
    if (!scene) return TR_OK;
    int status = TR_OK;
    if (scene->table) {
        tr_device_guard guard;
        if (guard.enter(scene->device) != TR_OK || hipFree(scene->table) != hipSuccess) status = tr_fail(TR_ERR_HIP, "hipFree(scene table)");
    }
    delete scene;
    return status;
}

int tr_scene_commit(tr_scene* scene, const tr_bvh* const* members, int64_t nmesh, const int32_t* mesh_of_instance, const float* M,
                    int64_t ninst, void* stream) {
    if (!scene) return tr_fail(TR_ERR_INVALID_ARG, "scene == NULL");
    if (nmesh < 0 || ninst < 0) return tr_fail(TR_ERR_INVALID_ARG, "negative count");
    if (ninst > 0x7fffffffll) return tr_fail(TR_ERR_INVALID_ARG, "too many instances");
    if (nmesh > 0 && !members) return tr_fail(TR_ERR_INVALID_ARG, "members == NULL");
    if (ninst > 0 && (!mesh_of_instance || !M)) return tr_fail(TR_ERR_INVALID_ARG, "mesh_of_instance or M == NULL");
    for (int64_t k = 0; k < nmesh; k++) {
        if (!members[k]) return tr_fail(TR_ERR_INVALID_ARG, "member " + std::to_string(k) + " == NULL");
        if (members[k]->device != scene->device)
            return tr_fail(TR_ERR_INVALID_ARG, "member " + std::to_string(k) + " lives on device " + std::to_string(members[k]->device) +
                                                   ", the scene on device " + std::to_string(scene->device));
    }
    for (int64_t k = 0; k < ninst; k++)
        if (mesh_of_instance[k] < 0 || mesh_of_instance[k] >= nmesh)
            return tr_fail(TR_ERR_INVALID_ARG, "instance " + std::to_string(k) + " names member " + std::to_string(mesh_of_instance[k]) +
                                                   " outside [0, " + std::to_string(nmesh) + ")");
    // the table on the host: members | instances
    const size_t mbytes = sizeof(tr_scene_member) * (size_t)nmesh, bytes = mbytes + sizeof(tr_scene_inst) * (size_t)ninst;
    std::vector<char> host(bytes);
    std::vector<tr_scene_member> committed((size_t)nmesh);
    for (int64_t k = 0; k < nmesh; k++) committed[(size_t)k] = member_of(members[k]);
    if (mbytes) memcpy(host.data(), committed.data(), mbytes);
    int64_t nvalid = 0;
    tr_scene_inst* recs = reinterpret_cast<tr_scene_inst*>(host.data() + mbytes);
    for (int64_t k = 0; k < ninst; k++) {
        tr_scene_inst rec;
        tr_scene_record(M + 12 * k, rec);
        rec.mesh = mesh_of_instance[k];
        if (committed[(size_t)rec.mesh].num_tris <= 0) rec.flags &= ~TR_SCENE_VALID;
        nvalid += (rec.flags & TR_SCENE_VALID) ? 1 : 0;
        memcpy(recs + k, &rec, sizeof(rec));
    }
    tr_device_guard guard;
    if (bytes > 0) TR_TRY(tr_enter_device(&guard, scene->device));
    if (bytes > scene->table_bytes) {
        // the new table first: if it cannot be had, the scene keeps its old one
        void* fresh = nullptr;
        TR_HIP_TRY(hipMalloc(&fresh, bytes));
        if (scene->table) (void)hipFree(scene->table);      // hipFree synchronises: no launch still reads it
        scene->table = fresh;
        scene->table_bytes = bytes;
        scene->ninst = 0;                                    // (until the copy below has succeeded)
    }
    if (bytes > 0) {
        hipError_t e = hipMemcpyAsync(scene->table, host.data(), bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) {
            scene->ninst = 0; scene->nvalid = 0;             // a half-written table is never walked: the scene is empty
            return tr_fail(TR_ERR_HIP, std::string("upload of the scene table: ") + hipGetErrorName(e));
        }
    }
    scene->members.assign(members, members + nmesh);
    scene->committed.swap(committed);
    scene->ninst = ninst; scene->nvalid = nvalid; scene->commits++;
    scene->d_members = reinterpret_cast<const tr_scene_member*>(scene->table);
    scene->d_insts = reinterpret_cast<const tr_scene_inst*>(reinterpret_cast<const char*>(scene->table) + mbytes);
    return TR_OK;
}

int tr_scene_info(const tr_scene* scene, tr_scene_info_t* info) {
    if (!scene || !info) return tr_fail(TR_ERR_INVALID_ARG, "null pointer argument");
    info->device = scene->device;
    info->stack_capacity = TR_RANGE_STACK;
    info->num_members = (int64_t)scene->members.size();
    info->num_instances = scene->ninst;
    info->valid_instances = scene->nvalid;
    info->table_bytes = (int64_t)scene->table_bytes;
    info->commits = scene->commits;
    return TR_OK;
}

int tr_scene_any(const tr_scene* scene, const tr_rays* rays, const float* d_tmin, const float* d_tmax, uint8_t* d_hit, int stack_entries,
                 void* stream) {
    const SceneOut out = {d_hit, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return scene_launch<TR_Q_ANY>(scene, rays, d_tmin, d_tmax, out, d_hit, stack_entries, stream);
}

int tr_scene_closest(const tr_scene* scene, const tr_rays* rays, const float* d_tmin, const float* d_tmax, int32_t* d_instance,
                     int32_t* d_tri, float* d_t, uint8_t* d_hit, uint8_t* d_front, float* d_loc3, float* d_uv2, int stack_entries,
                     void* stream) {
    const SceneOut out = {d_hit, d_front, d_instance, d_tri, d_t, d_loc3, d_uv2};
    return scene_launch<TR_Q_CLOSEST>(scene, rays, d_tmin, d_tmax, out, d_tri, stack_entries, stream);
}

}  // extern "C"
