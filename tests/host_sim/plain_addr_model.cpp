// plain_addr_model.cpp -- TEST-ONLY: the plain far-child stack by LDS byte address (tr_bvh.h: tr_addr_push / tr_addr_pop /
// tr_addr_give / tr_addr_bottom, what the stealing kernels run) side by side with the shipped slot-count form
// (tr_plain_push / tr_plain_pop / tr_plain_give, sp = 2 * slots | lost) and with a plain vector of owed entries, under
// a random sequence of pushes, pops, hand-overs and fresh walks.  tests/test_plain_addr_cpu.py builds and calls it.
//
// The address form works on one lane of a "block" of LANES lanes whose slots interleave as in LDS (slot s of lane t at
// byte 4 * t + s * stride, stride = 4 * LANES), between guard words; every word that is not one of the lane's TR_RING
// slots must keep its pattern.  A fresh walk starts where a thief starts: sa = tr_addr_bottom(sa), bot = 0.
//
// The two forms agree on every node handed out, on the lost flag and on can-give UNTIL a push is lost.  From there the
// slot-count form walks on and the address form drops every further child and ends at its next pop (tr_bvh.h); the ray is
// traversed again either way.  The model checks exactly that: after a loss the address form gives nothing away, stores
// nothing, keeps its flag, and its next pop returns -1.
#include <cstdint>
#include <vector>

#include "../../trimesh-ray-optix_amd/csrc/tr_bvh.h"

namespace {
struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};
constexpr int LANES = 4, GUARD = 3, WORDS = 2 * GUARD + TR_RING * LANES;
int32_t pattern(int i) { return (int32_t)(0x5a000000u + (uint32_t)i * 2654435761u % 0x00ffffffu) | 0x40000000; }
}  // namespace

// out[0] mismatches, [1] recorded pushes, [2] pushes onto a full stack (16 live entries), [3] pushes that did not fit because
// of slots given away (fewer than 16 live), [4] hand-overs, [5] pops served from the stack, [6] pops straight after a
// hand-over of the bottom slot (slot 0), [7] walks ended by a given-away slot, [8] walks ended on an empty stack, [9] walks
// of the address form ended by the pop after a loss, [10] fresh walks whose first operation was a push, [11] pops straight
// after such a push, [12] operations after a loss in which the address form had to stay put
extern "C" void plain_addr_model(uint64_t seed, int steps, int64_t* out) {
    for (int k = 0; k < 13; k++) out[k] = 0;
    Rng rng{seed};
    const int lane = (int)(seed % LANES);
    // the slot-count form: its own words, as tests/host_sim/plain_stack_model.cpp holds them
    int32_t mem_p[TR_RING + 2];
    mem_p[0] = 0x5a5a5a5a; mem_p[TR_RING + 1] = 0x5a5a5a5a;
    const tr_ring ring_p = {mem_p + 1, 1};
    // the address form: a block's worth of interleaved slots between guards
    int32_t mem_a[WORDS];
    for (int i = 0; i < WORDS; i++) mem_a[i] = pattern(i);
    const tr_ring ring_a = {mem_a + GUARD + lane, LANES, mem_a + GUARD};
    const tr_aring ar = tr_aring_of(ring_a);
    auto foreign_intact = [&]() {
        for (int i = 0; i < WORDS; i++) {
            const int w = i - GUARD;
            const bool mine = w >= 0 && w < TR_RING * LANES && w % LANES == lane;
            if (!mine && mem_a[i] != pattern(i)) return false;
        }
        return true;
    };
    std::vector<int32_t> ref;          // recorded entries, oldest first
    uint32_t given = 0;
    bool lost = false;
    tr_pstate sp_st;
    tr_state_init(sp_st);
    tr_astate ad_st;
    tr_state_init(ad_st, tr_addr_start(ring_a));
    if (ad_st.sa != 4u * (uint32_t)lane) out[0]++;
    uint32_t bot_p = 0, bot_a = 0;
    int32_t next_node = 1;
    uint32_t push_pct = 55;
    int since_fresh = 0;               // operations of this walk so far
    bool last_give_bottom = false, last_first_push = false;
    auto fresh = [&]() {
        tr_state_init(sp_st);
        tr_state_init(ad_st, tr_addr_bottom(ar, ad_st.sa));     // as a thief starts
        if (ad_st.sa != 4u * (uint32_t)lane) out[0]++;
        bot_p = 0; bot_a = 0; given = 0; lost = false;
        ref.clear();
        since_fresh = 0;
    };
    for (int s = 0; s < steps; s++) {
        if ((s & 255) == 0) push_pct = 35u + rng.next() % 40u;       // phases that fill the stack and phases that drain it
        const uint32_t r = rng.next() % 100u;
        if (tr_plain_lost(sp_st.sp) != lost || tr_addr_lost(ad_st.sa) != lost) out[0]++;
        if (tr_plain_can_give(sp_st.sp, bot_p) != !ref.empty()) out[0]++;
        if (tr_addr_can_give(ar, ad_st.sa, bot_a) != (!lost && !ref.empty())) out[0]++;
        const bool was_give_bottom = last_give_bottom, was_first_push = last_first_push;
        last_give_bottom = false; last_first_push = false;
        if (r < push_pct) {                                            // both children hit: owe the far one
            const bool fits = given + ref.size() < TR_RING;
            const uint32_t before = ad_st.sa;
            tr_plain_push(ring_p, sp_st.sp, next_node);
            tr_addr_push(ar, ad_st.sa, next_node);
            if (lost) {                                                // the address form drops it whether it would fit or not
                if (ad_st.sa != before) out[0]++;
                if (fits) ref.push_back(next_node);
                out[12]++;
            } else if (fits) {
                if (ad_st.sa != before + ar.stride) out[0]++;
                if (tr_addr_get(ar, before) != next_node) out[0]++;
                ref.push_back(next_node);
                out[1]++;
                if (since_fresh == 0) { out[10]++; last_first_push = true; }
            } else {
                if (ad_st.sa != (before | TR_ADDR_LOST)) out[0]++;
                lost = true;
                out[ref.size() == TR_RING ? 2 : 3]++;
            }
            next_node++;
        } else if (r < push_pct + 12u && !ref.empty() && !lost) {      // hand the shallowest entry to another lane
            const int32_t np = tr_plain_give(ring_p, bot_p);
            const int32_t na = tr_addr_give(ar, ad_st.sa, bot_a);
            if (np != ref.front() || na != ref.front()) out[0]++;
            last_give_bottom = given == 0;
            ref.erase(ref.begin());
            given++;
            if (bot_p != given || bot_a != given) out[0]++;
            out[4]++;
        } else {                                                       // no child hit: pay the youngest far child
            const int32_t np = tr_plain_pop(ring_p, sp_st.sp);
            const int32_t na = tr_addr_pop(ar, ad_st.sa);
            if (lost) {                                                // the address form's walk ends here
                if (na != -1 || !tr_addr_lost(ad_st.sa)) out[0]++;
                if (np != (ref.empty() ? -1 : ref.back())) out[0]++;
                out[9]++;
                fresh();
                continue;
            }
            if (!ref.empty()) {
                if (np != ref.back() || na != ref.back()) out[0]++;
                ref.pop_back();
                out[5]++;
                if (was_give_bottom) out[6]++;
                if (was_first_push) out[11]++;
            } else {
                if (np != -1 || na != -1) out[0]++;
                out[given ? 7 : 8]++;
                if (was_give_bottom) out[6]++;
                fresh();
                continue;
            }
        }
        since_fresh++;
        if (mem_p[0] != 0x5a5a5a5a || mem_p[TR_RING + 1] != 0x5a5a5a5a) out[0]++;
        if (!foreign_intact()) out[0]++;
    }
}
