// gmw.h — internal types of the GMW party engine (gmw_plan.cpp, gmw_engine.cpp, gmw_kernels.hip).
//
// A pass of one party is cut into exchange rounds.  Round r (0 <= r <= R, R = AND levels) first closes the AND level of
// round r - 1 (z fold), then evaluates the free gates of the levels after it up to and including level l_r, in the
// reference's bucketed order, then opens d / e of the ANDs of l_r.  Round R has no AND level: it ends with the outputs.
// Wires are renamed to single-assignment slots along that order, so every slot is written once per pass.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/gcengine.h"

namespace gc {

// one free gate of a step: slots in0, in1 (in0 again for INV), out, op (GC_XOR / GC_XNOR / GC_INV)
struct GmwGate {
    uint32_t in0, in1, out, op;
};

struct GmwRound {
    uint32_t level;       // AND level l_r opened by this round (nlevels for the last round)
    uint32_t and_n;       // ANDs of l_r (0 for the last round)
    uint32_t and_W;       // first triple word of l_r
    uint32_t and_w;       // ceil(and_n / 64)
    uint32_t and_in;      // offset in GmwPlan::idx: in0 slots [and_n], then in1 slots [and_n]
    uint32_t and_out;     // offset in GmwPlan::idx: out slots [and_n] (written when round r + 1 closes the level)
    uint32_t gate_first;  // first gate of the round in GmwPlan::gates
    uint32_t nsub;        // free-gate sub-rounds (chain depth inside the round)
    uint32_t sub_first;   // offset in GmwPlan::sub: nsub + 1 gate offsets relative to gate_first
};

struct GmwPlan {
    gc_gmw_info info{};
    uint32_t nslots = 0;                  // ninputs + ngates
    std::vector<uint32_t> level_of_gate;  // original order
    std::vector<uint32_t> and_index_of_gate;
    std::vector<uint32_t> words_of_level;
    std::vector<GmwRound> rounds;         // R + 1
    std::vector<GmwGate> gates;           // free gates, round by round, sub-round by sub-round
    std::vector<uint32_t> sub;            // sub-round offsets
    std::vector<uint32_t> idx;            // AND input / output slot lists
    std::vector<uint32_t> out_slots;      // slots of the last noutputs wires at the end of the pass
};

int build_gmw_plan(const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs, uint32_t noutputs, GmwPlan *out);

// kernel arguments of one step (gmw_kernels.hip)
struct GmwStepArgs {
    uint64_t *slots;             // [nslots][bw]: instance-bit-sliced shares
    const GmwGate *gates;        // free gates of the round
    const uint32_t *sub;         // nsub + 1 offsets into gates
    uint32_t nsub;
    // closing the previous AND level
    const uint32_t *close_out;   // [close_n] output slots
    uint32_t close_n, close_w, close_W;
    const uint64_t *own_prev;    // [2][close_w][batch]: this party's d, e of that level
    const uint64_t *peers;       // [npeers][2][close_w][batch]
    uint32_t npeers;
    // opening the round's AND level
    const uint32_t *and_in;      // [2][and_n] input slots
    uint32_t and_n, and_w, and_W;
    uint64_t *own_next;          // [2][and_w][batch]
    uint64_t *msg_out;           // [2][and_w][batch]
    const uint64_t *ta, *tb, *tc;  // triples [TW][batch]
    // outputs (last round)
    const uint32_t *out_slots;
    uint32_t nout;
    uint64_t *out;               // [ceil(nout/64)][batch]
    uint32_t batch, bw, party0;
};

hipError_t gmw_launch_inputs(hipStream_t s, uint64_t *slots, const uint64_t *in, uint32_t ninputs, uint32_t batch, uint32_t bw);
hipError_t gmw_launch_step(hipStream_t s, const GmwStepArgs &a);
hipError_t gmw_launch_fold(hipStream_t s, int kind, uint32_t delta_bit, const uint64_t *x, const uint64_t *y,
                           const uint64_t *z, uint64_t *c, size_t words);

}  // namespace gc
