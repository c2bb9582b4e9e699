// stack_model.cpp -- TEST-ONLY: the far-child stack of tr_bvh.h (tr_push_far / tr_pop_far / tr_bottom_slot) driven by a
// random sequence of pushes, descents, pops and HAND-OVERS (the stealing launches' removal of the shallowest entry, which the
// ray-by-ray host simulation never performs) against a plain vector of owed entries.  tests/test_dense_stack_cpu.py builds
// and calls it.
#include <cstdint>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_bvh.h"

namespace {
struct Owed { uint32_t depth; int32_t node; bool recorded; };

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

// out[0] mismatches, [1] recorded pushes, [2] pushes onto a full stack, [3] hand-overs, [4] pushes whose slot wrapped
// (rank >= N: ghosts below), [5] pops of an unrecorded entry that cleared a ghost above it, [6] pops served from the stack
template <typename W>
void run(uint64_t seed, int steps, int64_t* out) {
    constexpr uint32_t N = TR_RING;
    constexpr uint32_t TOP = 8 * sizeof(W) - 1;           // deepest depth that still has a trail bit
    Rng rng{seed};
    int32_t mem[TR_RING];
    const tr_ring ring = {mem, 1};
    std::vector<Owed> ref;                                 // by increasing depth
    W trail = 0, owned = 0;
    uint32_t depth = 0;
    int32_t next_node = 1;
    auto live = [&]() { uint32_t n = 0; for (const Owed& e : ref) n += e.recorded ? 1u : 0u; return n; };
    for (int s = 0; s < steps; s++) {
        const uint32_t r = rng.next() % 100u;
        if (r < 45 && depth <= TOP) {                      // both children hit: push the far one, go down
            const bool fits = live() < N;
            const W before = owned;
            tr_push_far(ring, trail, owned, depth, next_node);
            trail |= W(1) << depth;
            const bool rec = ((owned >> depth) & W(1)) != 0;
            if (rec != fits || (owned & ~(W(1) << depth)) != before) out[0]++;
            out[rec ? 1 : 2]++;
            if (rec && tr_popc(before) >= N) out[4]++;
            ref.push_back({depth, next_node++, rec});
            depth++;
        } else if (r < 58 && depth <= TOP) {               // one child hit: go down
            depth++;
        } else if (r < 75 && (trail & owned) != 0) {       // hand the shallowest recorded entry to another lane
            uint32_t j = 0;
            const uint32_t slot = tr_bottom_slot<W>(trail, owned, j);
            size_t k = 0;
            while (k < ref.size() && !ref[k].recorded) k++;
            if (k == ref.size() || ref[k].depth != j || slot >= N || mem[slot] != ref[k].node) out[0]++;
            if (k < ref.size()) ref.erase(ref.begin() + (long)k);
            trail &= ~(W(1) << j);
            out[3]++;
        } else if (trail == 0) {                           // no child hit, nothing owed: the next ray (tr_state_init)
            if (!ref.empty()) out[0]++;
            owned = 0; depth = 0;
        } else {                                           // no child hit: pay the deepest far child
            uint32_t j = 0;
            int32_t node = -1;
            const W owned_before = owned;
            const bool got = tr_pop_far(ring, trail, owned, j, node);
            if (ref.empty()) { out[0]++; continue; }
            const Owed e = ref.back();
            ref.pop_back();
            if (got != e.recorded || j != e.depth || (got && node != e.node)) out[0]++;
            if (got) out[6]++;
            if (!got && (owned_before >> j) != 0) out[5]++;            // (a ghost above an entry that was never recorded)
            if ((owned >> j) != 0) out[0]++;                           // nothing at or above the popped depth stays owned
            depth = j + 1;
        }
        W t = 0;
        for (const Owed& e : ref) t |= W(1) << e.depth;
        if (t != trail) out[0]++;
    }
}
}  // namespace

extern "C" void stack_model(int bits, uint64_t seed, int steps, int64_t* out) {
    for (int k = 0; k < 8; k++) out[k] = 0;
    if (bits == 32) run<uint32_t>(seed, steps, out);
    else run<uint64_t>(seed, steps, out);
}
