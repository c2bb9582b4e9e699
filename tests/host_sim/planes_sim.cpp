// planes_sim.cpp -- TEST-ONLY: csrc/tr_planes.h built for the host (libplanes_sim.so, tests/host_sim/planes_sim.py).
// The brute force: the predicates tr_plane_meets / tr_plane_cut over every active triangle of a mesh, in face order -- counts,
// lists and segments: the oracle of the GPU tests.  And the walk of k_planes<> for a SIMULATED WAVE of 64 lanes over the arrays of
// a hierarchy (sim.SimBVH: built on the host, or downloaded from the GPU builder), plane by plane: the loop of planes.hip line for
// line, its ballots taken by a loop over the lanes, on the very same per-lane functions (tr_planes_visit, tr_planes_sub_next,
// tr_planes_leaf, tr_planes_rank), followed by the ordering network (tr_planes_step, one worker) and tr_planes_row per row.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_planes.h"

static tr_plane sim_plane(const float* o, const float* n) {
    tr_plane q;
    q.ox = o[0]; q.oy = o[1]; q.oz = o[2]; q.nx = n[0]; q.ny = n[1]; q.nz = n[2];
    return q;
}

static tr_bvh_view sim_view(const void* nodes, const void* links, const void* tris, int64_t nf) {
    tr_bvh_view v;
    memset(&v, 0, sizeof(v));
    v.nodes = (const tr_node*)nodes; v.links = (const tr_link*)links; v.tris = (const tr_tri*)tris; v.num_tris = nf;
    return v;
}

// the ordering network on m keys, one worker; ride (may be null): a word per key, stride words apart
static void sim_order(int32_t* f, int32_t* ride, int64_t stride, uint32_t m) {
    for (uint32_t k = 1u; k < m; k <<= 1) {
        tr_planes_step(f, ride, stride, m, k, 0u, 0u, 1u);
        for (uint32_t j = k >> 1; j >= 1u; j >>= 1) tr_planes_step(f, ride, stride, m, k, j, 0u, 1u);
    }
}

namespace {

// what the wave of one plane shares
struct sim_wave {
    tr_bvh_view b;
    tr_plane q;
    int cut, mode;
    int32_t cursor, limit;
    int32_t* face;      // FILL: the rows of the plane
    int32_t* seg;       // FILL: their segments as words (slot in word 0), or null
    int64_t rounds, sub_steps, overflows;
};

// pl_record of planes.hip: the candidates of the 64 lanes, evaluated and recorded at the cursor
void sim_record(sim_wave& w, const int32_t* cand) {
    uint64_t any = 0, mh = 0;
    int32_t f[TR_PLANES_WAVE];
    for (int l = 0; l < TR_PLANES_WAVE; l++) any |= (uint64_t)(cand[l] >= 0) << l;
    if (any == 0) return;
    for (int l = 0; l < TR_PLANES_WAVE; l++) {
        f[l] = 0;
        const bool hit = cand[l] >= 0 && tr_planes_leaf(w.b, cand[l], w.q, w.cut, f[l]);
        mh |= (uint64_t)hit << l;
    }
    if (w.mode == TR_PLANES_FILL)
        for (int l = 0; l < TR_PLANES_WAVE; l++) {
            const int32_t pos = w.cursor + tr_planes_rank(mh, l);
            if (((mh >> l) & 1) && pos < w.limit) {
                w.face[pos] = f[l];
                if (w.seg) w.seg[6 * (int64_t)pos] = cand[l];
            }
        }
    w.cursor += tr_planes_popc(mh);
}

bool sim_full(const sim_wave& w) {
    return w.mode == TR_PLANES_ANY ? tr_planes_full<TR_PLANES_ANY>(w.cursor, w.limit)
                                   : (w.mode == TR_PLANES_FILL ? tr_planes_full<TR_PLANES_FILL>(w.cursor, w.limit) : false);
}

// k_planes of planes.hip for one plane
void sim_walk_one(sim_wave& w, int frontier_entries) {
    const int32_t cap = frontier_entries > 0 ? frontier_entries : TR_PLANES_FRONTIER;
    std::vector<int32_t> frontier(TR_PLANES_FRONTIER);
    int32_t cand[TR_PLANES_WAVE];
    w.cursor = 0;
    const bool walk = tr_plane_valid(w.q) && w.b.num_tris > 0 && !(w.mode == TR_PLANES_FILL && w.limit <= 0);
    if (walk && w.b.num_tris < 2) {
        for (int l = 0; l < TR_PLANES_WAVE; l++) cand[l] = l == 0 ? 0 : -1;
        sim_record(w, cand);
    } else if (walk) {
        int32_t top = 1;
        frontier[0] = 0;
        tr_planes_sub sub[TR_PLANES_WAVE];
        for (int l = 0; l < TR_PLANES_WAVE; l++) tr_planes_sub_init(sub[l]);
        for (;;) {
            bool any_sub = false;
            for (int l = 0; l < TR_PLANES_WAVE; l++) any_sub = any_sub || sub[l].node >= 0;
            if (any_sub) {
                for (int l = 0; l < TR_PLANES_WAVE; l++) cand[l] = sub[l].node >= 0 ? tr_planes_sub_next(w.b, w.q, sub[l]) : -1;
                w.sub_steps++;
                sim_record(w, cand);
                if (sim_full(w)) break;
                continue;
            }
            if (top == 0) break;
            w.rounds++;
            const int32_t take = top < TR_PLANES_WAVE ? top : TR_PLANES_WAVE;
            int32_t node[TR_PLANES_WAVE];
            for (int l = 0; l < TR_PLANES_WAVE; l++) node[l] = l < take ? frontier[top - 1 - l] : -1;
            top -= take;
            tr_planes_found fd[TR_PLANES_WAVE];
            uint64_t m0 = 0, m1 = 0;
            for (int l = 0; l < TR_PLANES_WAVE; l++) {
                fd[l] = tr_planes_visit(w.b, node[l], w.q);
                m0 |= (uint64_t)(fd[l].push0 >= 0) << l;
                m1 |= (uint64_t)(fd[l].push1 >= 0) << l;
            }
            for (int l = 0; l < TR_PLANES_WAVE; l++) {
                const int32_t at0 = top + tr_planes_rank(m0, l), at1 = top + tr_planes_popc(m0) + tr_planes_rank(m1, l);
                if (fd[l].push0 >= 0) { if (at0 < cap) frontier[at0] = fd[l].push0; else { tr_planes_sub_start(sub[l], fd[l].push0); w.overflows++; } }
                if (fd[l].push1 >= 0) { if (at1 < cap) frontier[at1] = fd[l].push1; else { tr_planes_sub_start(sub[l], fd[l].push1); w.overflows++; } }
            }
            top += tr_planes_popc(m0) + tr_planes_popc(m1);
            top = top < cap ? top : cap;
            for (int l = 0; l < TR_PLANES_WAVE; l++) cand[l] = fd[l].leaf0;
            sim_record(w, cand);
            if (sim_full(w)) break;
            for (int l = 0; l < TR_PLANES_WAVE; l++) cand[l] = fd[l].leaf1;
            sim_record(w, cand);
            if (sim_full(w)) break;
        }
    }
}

}  // namespace

extern "C" {

int sim_planes_frontier_capacity(void) { return TR_PLANES_FRONTIER; }

// pass 1 (face == null): count [n].  pass 2: the rows of plane i at offsets[i] ..: face, and segments [rows, 2, 3] where given
// (cut != 0 only).  vertices [nv, 3], faces [nf, 3], origins / normals [n, 3]
void sim_planes_brute(const float* verts, const int32_t* faces, int64_t nf, const float* org, const float* nrm, int64_t n, int cut,
                      int32_t* count, const int64_t* offsets, int32_t* face, float* segments) {
    for (int64_t i = 0; i < n; i++) {
        const tr_plane q = sim_plane(org + 3 * i, nrm + 3 * i);
        const bool valid = tr_plane_valid(q);
        int32_t k = 0;
        for (int64_t f = 0; valid && f < nf; f++) {
            const float *a = verts + 3 * faces[3 * f], *b = verts + 3 * faces[3 * f + 1], *c = verts + 3 * faces[3 * f + 2];
            if (!tr_near_active(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2])) continue;
            const double s0 = tr_plane_s(q, a[0], a[1], a[2]), s1 = tr_plane_s(q, b[0], b[1], b[2]), s2 = tr_plane_s(q, c[0], c[1], c[2]);
            if (!(cut ? tr_plane_cut(s0, s1, s2) : tr_plane_meets(s0, s1, s2))) continue;
            if (face) {
                const int64_t row = offsets[i] + k;
                face[row] = (int32_t)f;
                if (segments) {
                    tr_tri t;
                    memset(&t, 0, sizeof(t));
                    t.ax = a[0]; t.ay = a[1]; t.az = a[2]; t.bx = b[0]; t.by = b[1]; t.bz = b[2]; t.cx = c[0]; t.cy = c[1]; t.cz = c[2];
                    tr_plane_segment(q, t, segments + 6 * row, segments + 6 * row + 3);
                }
            }
            k++;
        }
        if (count) count[i] = k;
    }
}

// the signed values of the three vertices of every face for every plane: s [n, nf, 3] float64
void sim_planes_signed(const float* verts, const int32_t* faces, int64_t nf, const float* org, const float* nrm, int64_t n, double* s) {
    for (int64_t i = 0; i < n; i++) {
        const tr_plane q = sim_plane(org + 3 * i, nrm + 3 * i);
        for (int64_t f = 0; f < nf; f++)
            for (int c = 0; c < 3; c++) {
                const float* v = verts + 3 * faces[3 * f + c];
                s[(i * nf + f) * 3 + c] = tr_plane_s(q, v[0], v[1], v[2]);
            }
    }
}

// the walk of a simulated wave on (nodes, links, tris) of nf triangles; frontier_entries: 0 = all, 1 .. TR_PLANES_FRONTIER.
// mode 0: any [n] (as 0 / 1 in out); 1: count [n] in out; 2: the fill -- count / offsets / total as tr_planes_fill takes them, rows
// into face (and segments, which may be null), ordered.  stats [n, 3] (may be null): rounds, subtree-walk steps and pushes that
// did not fit, per plane.
void sim_planes_walk(const void* nodes, const void* links, const void* tris, int64_t nf, const float* org, const float* nrm, int64_t n,
                     int cut, int frontier_entries, int mode, int32_t* out, const int32_t* count, const int64_t* offsets, int64_t total,
                     int32_t* face, float* segments, int64_t* stats) {
    sim_wave w;
    memset(&w, 0, sizeof(w));
    w.b = sim_view(nodes, links, tris, nf);
    w.cut = cut; w.mode = mode;
    for (int64_t i = 0; i < n; i++) {
        w.q = sim_plane(org + 3 * i, nrm + 3 * i);
        w.limit = 0; w.face = nullptr; w.seg = nullptr;
        w.rounds = 0; w.sub_steps = 0; w.overflows = 0;
        if (mode == TR_PLANES_FILL) {
            const int64_t off = offsets[i];
            w.limit = tr_within_limit(count[i], off, total);
            if (w.limit > 0) {
                w.face = face + off;
                w.seg = segments ? reinterpret_cast<int32_t*>(segments) + 6 * off : nullptr;
            }
        }
        sim_walk_one(w, frontier_entries);
        if (mode == TR_PLANES_ANY) out[i] = w.cursor > 0 ? 1 : 0;
        if (mode == TR_PLANES_COUNT) out[i] = w.cursor;
        if (mode == TR_PLANES_FILL && w.limit > 0) {
            sim_order(w.face, w.seg, 6, (uint32_t)w.limit);      // k_planes_rows
            if (segments && nf > 0)                              // k_planes_segments
                for (int32_t r = 0; r < w.limit; r++) {
                    const int64_t row = offsets[i] + r;
                    if (tr_planes_owner(offsets, n, row) != i) continue;      // (rows of overlapping, misdirected planes)
                    tr_planes_row(w.b, w.q, w.seg[6 * (int64_t)r], segments + 6 * row);
                }
        }
        if (stats) { stats[3 * i] = w.rounds; stats[3 * i + 1] = w.sub_steps; stats[3 * i + 2] = w.overflows; }
    }
}

// the ordering network alone: segment i = keys[offsets[i] .. offsets[i] + tr_within_limit(count[i], ..)), in place
void sim_planes_order(int64_t n, const int32_t* count, const int64_t* offsets, int64_t total, int32_t* keys) {
    for (int64_t i = 0; i < n; i++) {
        const int32_t m = tr_within_limit(count[i], offsets[i], total);
        if (m > 1) sim_order(keys + offsets[i], nullptr, 1, (uint32_t)m);
    }
}

// every (i, p) the network forms for m keys, the largest index in *max_index (the claim: below m) and the number of pairs
int64_t sim_planes_network_pairs(uint32_t m, uint32_t* max_index) {
    int64_t pairs = 0;
    uint32_t mx = 0;
    for (uint32_t k = 1u; k < m; k <<= 1) {
        uint32_t j = 0u;
        for (;;) {
            for (uint32_t t = 0;; t++) {
                uint32_t i, p;
                tr_planes_pair(t, k, j, i, p);
                if (i >= m) break;
                if (p < m) { pairs++; mx = p > mx ? p : mx; }
            }
            j = j == 0u ? k >> 1 : j >> 1;
            if (j == 0u) break;
        }
    }
    *max_index = mx;
    return pairs;
}

}  // extern "C"
