// gmw_plan.cpp — host-only plan of the GMW party engine (no GPU needed): AssignLevels(TargetGMW), the reference's
// bucketed execution order, single-assignment slots along it, and the exchange rounds the device steps walk.
//
// Order (gmw/network.go:563-618): for every level ascending, first the XOR / XNOR / INV gates of the level in circuit
// order, then the AND gates of the level, all of which read their inputs before any of them writes (andBatchFlush packs
// every input bit before the z fold sets the outputs, network.go:680-756).  With wire reuse this order and circuit order
// read different values; renaming along the bucketed order gives every read the value the reference reads.
#include <algorithm>
#include <new>

#include "gmw.h"
#include "plan.h"

namespace gc {

int build_gmw_plan(const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs, uint32_t noutputs, GmwPlan *out) {
    if ((!gates && ngates) || !out) return GC_E_ARG;
    if (ninputs > nwires || noutputs > nwires) return GC_E_ARG;
    if ((uint64_t)ninputs + ngates >= 0xffffffffull) return GC_E_ARG;
    const uint32_t NONE = 0xffffffffu;
    GmwPlan &p = *out;
    p = GmwPlan{};
    p.info.ngates = ngates;
    p.info.nwires = nwires;
    p.info.ninputs = ninputs;
    p.info.noutputs = noutputs;
    p.nslots = ninputs + ngates;

    // AssignLevels(TargetGMW) (circuit/circuit.go:206-254), with the checks of gc_plan_create (plan.cpp: build_plan)
    std::vector<uint32_t> wire_level(nwires, 0);
    std::vector<uint8_t> set(nwires, 0);
    for (uint32_t w = 0; w < ninputs; w++) set[w] = 1;
    p.level_of_gate.resize(ngates);
    uint32_t max_level = 0;
    for (uint32_t g = 0; g < ngates; g++) {
        const gc_gate &G = gates[g];
        if (G.op > GC_INV || G.op == GC_OR) return GC_E_GATE;  // "gate OR not supported" (network.go:609)
        const bool unary = (G.op == GC_INV);
        if (G.in0 >= nwires || G.out >= nwires || (!unary && G.in1 >= nwires)) return GC_E_WIRE;
        if (!set[G.in0] || (!unary && !set[G.in1])) return GC_E_WIRE;
        uint32_t level = wire_level[G.in0];
        if (!unary) level = std::max(level, wire_level[G.in1]);
        p.level_of_gate[g] = level;
        if (G.op == GC_AND) level++;
        wire_level[G.out] = level;
        set[G.out] = 1;
        max_level = std::max(max_level, level);
        switch (G.op) {
        case GC_AND: p.info.n_and++; break;
        case GC_INV: p.info.n_inv++; break;
        case GC_XOR: p.info.n_xor++; break;
        default: p.info.n_xnor++; break;
        }
    }
    const uint32_t nlevels = max_level + 1;  // Stats[NumLevels] + 1 (network.go:564)
    p.info.nlevels = nlevels;

    // buckets (network.go:565-576)
    std::vector<uint32_t> cnt_rest(nlevels + 1, 0), cnt_and(nlevels + 1, 0);
    for (uint32_t g = 0; g < ngates; g++) (gates[g].op == GC_AND ? cnt_and : cnt_rest)[p.level_of_gate[g] + 1]++;
    for (uint32_t l = 0; l < nlevels; l++) {
        cnt_rest[l + 1] += cnt_rest[l];
        cnt_and[l + 1] += cnt_and[l];
    }
    std::vector<uint32_t> rest(cnt_rest[nlevels]), ands(cnt_and[nlevels]);
    {
        std::vector<uint32_t> fr(cnt_rest.begin(), cnt_rest.end() - 1), fa(cnt_and.begin(), cnt_and.end() - 1);
        for (uint32_t g = 0; g < ngates; g++) {
            if (gates[g].op == GC_AND) ands[fa[p.level_of_gate[g]]++] = g;
            else rest[fr[p.level_of_gate[g]]++] = g;
        }
    }

    // triple words: whole words per level (TriplePool.Get / Triples.Append, triples.go:60-90,130-142)
    p.words_of_level.assign(nlevels, 0);
    std::vector<uint32_t> W_of_level(nlevels, 0);
    p.and_index_of_gate.assign(ngates, NONE);
    uint32_t tw = 0;
    for (uint32_t l = 0; l < nlevels; l++) {
        const uint32_t n = cnt_and[l + 1] - cnt_and[l];
        for (uint32_t k = 0; k < n; k++) p.and_index_of_gate[ands[cnt_and[l] + k]] = k;
        p.words_of_level[l] = (n + 63) / 64;
        W_of_level[l] = tw;
        tw += p.words_of_level[l];
        p.info.max_level_words = std::max(p.info.max_level_words, p.words_of_level[l]);
        if (n) p.info.n_and_levels++;
    }
    p.info.triple_words = tw;

    // slots along the bucketed order, rounds, and the free-gate sub-rounds of every round
    std::vector<uint32_t> slot_of_wire(nwires, NONE);
    for (uint32_t w = 0; w < ninputs; w++) slot_of_wire[w] = w;
    std::vector<uint32_t> slot_round(p.nslots, NONE), slot_depth(p.nslots, 0);
    uint32_t next = ninputs;
    std::vector<GmwGate> rg;
    std::vector<uint32_t> rdepth;
    for (uint32_t l = 0; l < nlevels; l++) {
        const uint32_t r = (uint32_t)p.rounds.size();
        for (uint32_t i = cnt_rest[l]; i < cnt_rest[l + 1]; i++) {
            const gc_gate &G = gates[rest[i]];
            const uint32_t s0 = slot_of_wire[G.in0], s1 = G.op == GC_INV ? s0 : slot_of_wire[G.in1];
            if (s0 == NONE || s1 == NONE) return GC_E_WIRE;
            uint32_t d = 0;
            if (slot_round[s0] == r) d = std::max(d, slot_depth[s0]);
            if (slot_round[s1] == r) d = std::max(d, slot_depth[s1]);
            const uint32_t s = next++;
            slot_round[s] = r;
            slot_depth[s] = d + 1;
            rg.push_back(GmwGate{s0, s1, s, G.op});
            rdepth.push_back(d);
            slot_of_wire[G.out] = s;
        }
        const uint32_t n = cnt_and[l + 1] - cnt_and[l];
        if (!n && l + 1 < nlevels) continue;
        // close the round: its free gates sorted by depth (stable), then its AND level (none for the last round)
        GmwRound R{};
        R.level = n ? l : nlevels;
        R.gate_first = (uint32_t)p.gates.size();
        R.sub_first = (uint32_t)p.sub.size();
        uint32_t nsub = 0;
        for (uint32_t d : rdepth) nsub = std::max(nsub, d + 1);
        R.nsub = nsub;
        std::vector<uint32_t> cnt(nsub + 1, 0);
        for (uint32_t d : rdepth) cnt[d + 1]++;
        for (uint32_t d = 0; d < nsub; d++) cnt[d + 1] += cnt[d];
        for (uint32_t d = 0; d <= nsub; d++) p.sub.push_back(cnt[d]);
        std::vector<GmwGate> sorted(rg.size());
        for (size_t i = 0; i < rg.size(); i++) sorted[cnt[rdepth[i]]++] = rg[i];
        p.gates.insert(p.gates.end(), sorted.begin(), sorted.end());
        p.info.max_free_depth = std::max(p.info.max_free_depth, nsub);
        rg.clear();
        rdepth.clear();
        if (n) {
            R.and_n = n;
            R.and_W = W_of_level[l];
            R.and_w = p.words_of_level[l];
            R.and_in = (uint32_t)p.idx.size();
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t s = slot_of_wire[gates[ands[cnt_and[l] + k]].in0];
                if (s == NONE) return GC_E_WIRE;
                p.idx.push_back(s);
            }
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t s = slot_of_wire[gates[ands[cnt_and[l] + k]].in1];
                if (s == NONE) return GC_E_WIRE;
                p.idx.push_back(s);
            }
            // every AND of the level has read its inputs: now the outputs (network.go:754-756)
            R.and_out = (uint32_t)p.idx.size();
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t s = next++;
                p.idx.push_back(s);
                slot_of_wire[gates[ands[cnt_and[l] + k]].out] = s;
            }
        }
        p.rounds.push_back(R);
    }
    if (p.rounds.empty() || p.rounds.back().and_n) {  // the last level had ANDs: an empty closing round follows
        GmwRound R{};
        R.level = nlevels;
        R.gate_first = (uint32_t)p.gates.size();
        R.sub_first = (uint32_t)p.sub.size();
        p.sub.push_back(0);
        p.rounds.push_back(R);
    }
    p.out_slots.resize(noutputs);
    for (uint32_t j = 0; j < noutputs; j++) {
        const uint32_t s = slot_of_wire[nwires - noutputs + j];
        if (s == NONE) return GC_E_WIRE;
        p.out_slots[j] = s;
    }
    return GC_OK;
}

}  // namespace gc

extern "C" int gc_gmw_plan_describe(const gc_gate *gates, uint32_t ngates, uint32_t nwires, uint32_t ninputs, uint32_t noutputs,
                                    gc_gmw_info *info, uint32_t *level_of_gate, uint32_t *and_index_of_gate,
                                    uint32_t *words_of_level) try {
    gc::GmwPlan p;
    const int rc = gc::build_gmw_plan(gates, ngates, nwires, ninputs, noutputs, &p);
    if (rc != GC_OK) return rc;
    if (info) *info = p.info;
    if (level_of_gate) std::copy(p.level_of_gate.begin(), p.level_of_gate.end(), level_of_gate);
    if (and_index_of_gate) std::copy(p.and_index_of_gate.begin(), p.and_index_of_gate.end(), and_index_of_gate);
    if (words_of_level) std::copy(p.words_of_level.begin(), p.words_of_level.end(), words_of_level);
    return GC_OK;
} catch (...) {
    return gc::on_exception();
}
