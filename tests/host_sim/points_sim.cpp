// points_sim.cpp -- TEST-ONLY: the host simulation (host_sim.cpp, included whole: same builder, same views, same entry
// points) plus the per-point routine of contains_points as k_contains_points (csrc/points.hip) runs it, point by point:
// tr_ray_setup_q and the unordered schedule (tr_traverse_unordered<TR_Q_COUNT>) for (p, d), the same for (p, -d), then
// the decision function of csrc/tr_points.h.  Meshes of fewer than two triangles have no hierarchy: the whole predicate
// on the one triangle, as the kernel does.  A library of its own (libpoints_sim.so, tests/host_sim/points_sim.py).
#include "host_sim.cpp"

#include "../../trimesh-ray-optix_amd/csrc/tr_points.h"

static int32_t count_one(const tr_bvh_view& v, const float* p, float dx, float dy, float dz) {
    tr_ray r;
    const bool valid = tr_ray_setup_q(r, v.frame, p[0], p[1], p[2], dx, dy, dz);
    tr_result res;
    tr_topk<1> top;
    tr_counters* nc = nullptr;
    if (v.num_tris >= 2) {
        int32_t ring_mem[TR_RING], leaf_mem[TR_LEAFQ];
        const tr_ring ring = {ring_mem, 1};
        const tr_leafq lq = {leaf_mem, 1};
        tr_traverse_unordered<TR_Q_COUNT, 1, false>(v, r, valid, res, top, nc, ring, lq);
        return res.count;
    }
    if (!valid || v.num_tris < 1) return 0;
    const tr_tri& t = v.tris[0];
    tr_hit h;
    return tr_tri_test(r, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, h) ? 1 : 0;
}

extern "C" {
// lo3 / hi3 both NULL: no box test.  counts = [2, n] (+d row, then -d row); summary2 = {points in the box, broken points}.
// The grid nodes come from sim_set_qnodes.
void sim_contains_points(const void* nodes, const void* links, const void* tris, int64_t nf, const float* points, int64_t n,
                         const float* dir3, const float* lo3, const float* hi3, uint8_t* inside, uint8_t* broken,
                         int32_t* counts, int64_t* summary2) {
    const tr_bvh_view v = view_of((const tr_node*)nodes, (const tr_link*)links, (const tr_tri*)tris, nf);
    summary2[0] = 0; summary2[1] = 0;
    for (int64_t i = 0; i < n; i++) {
        const float* p = points + 3 * i;
        const int32_t cp = count_one(v, p, dir3[0], dir3[1], dir3[2]);
        const int32_t cm = count_one(v, p, -dir3[0], -dir3[1], -dir3[2]);
        const bool in_box = tr_point_in_box(p[0], p[1], p[2], lo3, hi3);
        bool in, br;
        tr_point_decide(in_box, cp, cm, in, br);
        inside[i] = in; broken[i] = br;
        counts[i] = cp; counts[n + i] = cm;
        summary2[0] += in_box; summary2[1] += br;
    }
}
}

#ifdef POINTS_SIM_MAIN
// a stand-alone program around the same routine (for a sanitizer build of host code: g++ -fsanitize=... -DPOINTS_SIM_MAIN):
// an octahedron, a lattice of points through and around it, the known answer of its centre
#include <cstdio>
int main() {
    const float vs[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const int32_t fs[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    SimBvh* b = (SimBvh*)sim_build(vs, 6, fs, 8, -1, 0);
    std::vector<float> q(6);
    sim_get_qnodes(b, nullptr, q.data());
    sim_set_qnodes(b->qnodes.data(), q.data());
    std::vector<float> pts;
    for (int x = -4; x <= 4; x++) for (int y = -4; y <= 4; y++) for (int z = -4; z <= 4; z++) { pts.push_back(0.3f * x); pts.push_back(0.3f * y); pts.push_back(0.3f * z); }
    const int64_t n = (int64_t)pts.size() / 3;
    std::vector<uint8_t> in(n), br(n);
    std::vector<int32_t> cnt(2 * n);
    int64_t sum[2];
    const float dir[3] = {0.4395064455f, 0.617598629942f, 0.652231566745f}, lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1};
    sim_contains_points(b->nodes.data(), b->links.data(), b->tris.data(), 8, pts.data(), n, dir, lo, hi, in.data(), br.data(), cnt.data(), sum);
    int64_t inside = 0;
    for (int64_t i = 0; i < n; i++) inside += in[i];
    const int64_t centre = (4 * 9 + 4) * 9 + 4;
    printf("points %lld in box %lld broken %lld inside %lld centre %d\n", (long long)n, (long long)sum[0], (long long)sum[1], (long long)inside, (int)in[centre]);
    sim_destroy(b);
    // (a point whose two rays both miss counts as broken, like every point outside the octahedron's shadow: ray_optix.py:268)
    return (in[centre] == 1 && sum[0] == 343 && sum[1] > 0 && inside > 0 && inside < sum[0]) ? 0 : 1;
}
#endif
