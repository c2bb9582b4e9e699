// plain_stack_model.cpp -- TEST-ONLY: the plain far-child stack of tr_bvh.h (tr_plain_push / tr_plain_pop / tr_plain_give)
// driven by a random sequence of pushes, pops and HAND-OVERS (the stealing launch's removal of the shallowest entry, which
// the ray-by-ray host simulation never performs) against a plain vector of owed entries.  tests/test_plain_stack_cpu.py
// builds and calls it.
//
// The vector's rules, which are the walk's contract (tr_bvh.h, "plain far-child stack"):
//   * a push is recorded while given + live < TR_RING (slots given away stay in use until the walk ends); one that is not
//     recorded sets the sticky lost flag and changes nothing else;
//   * a pop returns the youngest recorded entry, or -1 when none is left -- whether the stack is empty or every slot below
//     the top was given away: the walk is over, the next one starts from tr_state_init and bot = 0;
//   * a hand-over returns the OLDEST recorded entry and is possible exactly when there is one.
#include <cstdint>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_bvh.h"

namespace {
struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};
}  // namespace

// out[0] mismatches, [1] recorded pushes, [2] pushes onto a full stack (16 live entries), [3] pushes that did not fit because
// of slots given away (fewer than 16 live), [4] hand-overs, [5] pops served from the stack, [6] pops served after a hand-over
// of the same walk, [7] walks ended by a given-away slot (the pop read -1 below live slots), [8] walks ended on an empty
// stack, [9] walks that ended with the lost flag set
extern "C" void plain_stack_model(uint64_t seed, int steps, int64_t* out) {
    for (int k = 0; k < 10; k++) out[k] = 0;
    Rng rng{seed};
    int32_t mem[TR_RING + 2];
    // guard words on both sides of the lane's TR_RING slots: nothing may ever touch them
    mem[0] = 0x5a5a5a5a; mem[TR_RING + 1] = 0x5a5a5a5a;
    const tr_ring ring = {mem + 1, 1};
    std::vector<int32_t> ref;          // recorded entries, oldest first
    uint32_t given = 0;                // hand-overs of this walk
    bool lost = false;
    tr_pstate st;
    tr_state_init(st);
    uint32_t bot = 0;
    int32_t next_node = 1;
    uint32_t push_pct = 55;
    for (int s = 0; s < steps; s++) {
        if ((s & 255) == 0) push_pct = 35u + rng.next() % 40u;       // phases that fill the stack and phases that drain it
        const uint32_t r = rng.next() % 100u;
        if (tr_plain_can_give(st.sp, bot) != !ref.empty()) out[0]++;
        if (tr_plain_lost(st.sp) != lost) out[0]++;
        if (r < push_pct) {                                            // both children hit: owe the far one
            const bool fits = given + ref.size() < TR_RING;
            const uint32_t before = st.sp;
            tr_plain_push(ring, st.sp, next_node);
            if (fits) {
                if (st.sp != before + 2u) out[0]++;
                ref.push_back(next_node);
                out[1]++;
            } else {
                if (st.sp != (before | 1u)) out[0]++;
                lost = true;
                out[ref.size() == TR_RING ? 2 : 3]++;
            }
            next_node++;
        } else if (r < push_pct + 12u && !ref.empty()) {               // hand the shallowest entry to another lane
            const int32_t node = tr_plain_give(ring, bot);
            if (node != ref.front()) out[0]++;
            ref.erase(ref.begin());
            given++;
            if (bot != given) out[0]++;
            out[4]++;
        } else {                                                       // no child hit: pay the youngest far child
            const int32_t node = tr_plain_pop(ring, st.sp);
            if (!ref.empty()) {
                if (node != ref.back()) out[0]++;
                ref.pop_back();
                out[5]++;
                if (given) out[6]++;
            } else {
                if (node != -1) out[0]++;
                out[given ? 7 : 8]++;
                if (lost) out[9]++;
                tr_state_init(st);                                     // the next walk
                bot = 0; given = 0; lost = false;
            }
        }
        if (mem[0] != 0x5a5a5a5a || mem[TR_RING + 1] != 0x5a5a5a5a) out[0]++;
    }
}
