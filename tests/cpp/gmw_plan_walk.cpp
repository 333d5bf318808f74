// gmw_plan_walk.cpp — host walk of gc::GmwPlan (mpc_amd/csrc/gmw_plan.cpp), built by tests/test_gmw_plan_walk.py with the
// host compiler from gmw_plan.cpp itself.  No GPU, no libgcengine.so: the plan's vectors are not part of the ABI.
//
// For every case of the input file it builds the plan and walks it as gmw_kernels.hip does, every party in lockstep over n
// <= 64 instances held one per bit of a u64 (the device's slot words): input load; per round the close of the previous AND
// level from the XOR of every party's d / e, the free gates sub-round by sub-round, the open of the round's AND level with
// zero padding bits, the outputs in the last round.  It prints what the engine would send and return, and checks what the
// device relies on: every barrier-separated stretch is a phase (the input launch; a close; each sub-round; the open and the
// output reads of a round), a slot is written at most once per pass, and every read is of a slot written in a strictly
// earlier phase.  Between two wg_sync() of k_gmw_step no wave may read a slot another wave writes: that is this check.
//
// Input, little endian, case after case:  u32 ngates, nwires, ninputs, noutputs, P, n, tw;  gc_gate[ngates];  then per party
// inputs u64 [ceil(ninputs/64)][n] and a, b, c u64 [tw][n] each.  tw is the caller's count of triple words (the restated
// reference's); a plan that counts differently is reported.
// Output, one line each:  "case K rc RC" (nothing more for RC != 0), "plan nslots nrounds nlevels n_and_levels",
// "round R LEVEL WORDS", "msg Q hex.." ([2][WORDS][n]), "out Q hex.." ([ceil(noutputs/64)][n]), "bad TEXT", "end K NBAD".
// A second argument "merge-sub-rounds" spoils every plan on purpose (host only), so the test can see the checks fire.
#include <algorithm>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gmw.h"

namespace gc {
int on_exception() noexcept { return GC_E_ARG; }
}  // namespace gc

using namespace gc;

namespace {

int g_bad = 0;

void bad(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::printf("bad ");
    std::vprintf(fmt, ap);
    std::printf("\n");
    va_end(ap);
    g_bad++;
}

template <class T>
bool rd(FILE *f, std::vector<T> *v, size_t n) {
    v->resize(n);
    return !n || std::fread(v->data(), sizeof(T), n, f) == n;
}

struct Party {
    std::vector<uint64_t> in, ta, tb, tc;  // [words][n]
    std::vector<uint64_t> S;               // [nslots]: bit i = instance i
    std::vector<uint64_t> own;             // [2][w][n] of the level being opened
};

void put(const char *tag, uint32_t q, const std::vector<uint64_t> &v) {
    std::printf("%s %u", tag, q);
    for (uint64_t x : v) std::printf(" %016" PRIx64, x);
    std::printf("\n");
}

// the structure the engine indexes by (gmw_engine.cpp: gc_gmw_step_dev) before any value is walked
bool check_structure(const GmwPlan &p, uint32_t tw) {
    const int before = g_bad;
    const gc_gmw_info &I = p.info;
    if (p.nslots != I.ninputs + I.ngates) bad("nslots %u != ninputs + ngates", p.nslots);
    if (p.rounds.size() != (size_t)I.n_and_levels + 1) bad("rounds %zu != n_and_levels + 1 = %u", p.rounds.size(), I.n_and_levels + 1);
    if (p.words_of_level.size() != I.nlevels) bad("words_of_level has %zu entries, nlevels %u", p.words_of_level.size(), I.nlevels);
    if (I.triple_words != tw) bad("triple_words %u, the reference counts %u", I.triple_words, tw);
    if (p.out_slots.size() != I.noutputs) bad("out_slots has %zu entries, noutputs %u", p.out_slots.size(), I.noutputs);
    if (p.rounds.empty()) return false;
    std::vector<uint32_t> W(p.words_of_level.size() + 1, 0);  // prefix sum of words_of_level
    uint32_t maxw = 0;
    for (size_t l = 0; l < p.words_of_level.size(); l++) {
        W[l + 1] = W[l] + p.words_of_level[l];
        maxw = std::max(maxw, p.words_of_level[l]);
    }
    if (W.back() != I.triple_words) bad("sum of words_of_level %u != triple_words %u", W.back(), I.triple_words);
    if (maxw != I.max_level_words) bad("max_level_words %u, levels give %u", I.max_level_words, maxw);
    size_t gate_next = 0, sub_next = 0, idx_next = 0, n_and = 0;
    uint32_t max_nsub = 0;
    for (size_t r = 0; r < p.rounds.size(); r++) {
        const GmwRound &R = p.rounds[r];
        const bool last = r + 1 == p.rounds.size();
        if (r && R.level <= p.rounds[r - 1].level) bad("round %zu: level %u not above round %zu's %u", r, R.level, r - 1, p.rounds[r - 1].level);
        if (last) {
            if (R.level != I.nlevels) bad("last round's level %u != nlevels %u", R.level, I.nlevels);
            if (R.and_n || R.and_w) bad("last round opens %u ANDs", R.and_n);
        } else {
            if (R.level >= I.nlevels) bad("round %zu: level %u >= nlevels %u", r, R.level, I.nlevels);
            if (!R.and_n) bad("round %zu is not the last and opens no AND", r);
        }
        if (R.and_w != (R.and_n + 63) / 64) bad("round %zu: and_w %u for %u ANDs", r, R.and_w, R.and_n);
        if (R.and_n && R.level < I.nlevels) {
            if (R.and_w != p.words_of_level[R.level]) bad("round %zu: and_w %u != words_of_level[%u] = %u", r, R.and_w, R.level, p.words_of_level[R.level]);
            if (R.and_W != W[R.level]) bad("round %zu: and_W %u != prefix sum %u", r, R.and_W, W[R.level]);
            if ((uint64_t)R.and_W + R.and_w > tw) bad("round %zu: triple words [%u, +%u) past %u", r, R.and_W, R.and_w, tw);
            if (R.and_in != idx_next) bad("round %zu: and_in %u, expected %zu", r, R.and_in, idx_next);
            if (R.and_out != (size_t)R.and_in + 2 * (size_t)R.and_n) bad("round %zu: and_out %u does not follow the inputs", r, R.and_out);
            idx_next = (size_t)R.and_out + R.and_n;
            if (idx_next > p.idx.size()) bad("round %zu: slot lists end at %zu past idx (%zu)", r, idx_next, p.idx.size());
            n_and += R.and_n;
        }
        if (R.gate_first != gate_next) bad("round %zu: gate_first %u, expected %zu", r, R.gate_first, gate_next);
        if (R.sub_first != sub_next) bad("round %zu: sub_first %u, expected %zu", r, R.sub_first, sub_next);
        if ((size_t)R.sub_first + R.nsub + 1 > p.sub.size()) {
            bad("round %zu: sub offsets past the end of sub (%zu)", r, p.sub.size());
            return false;
        }
        const uint32_t *sub = p.sub.data() + R.sub_first;
        if (sub[0] != 0) bad("round %zu: first sub offset %u", r, sub[0]);
        for (uint32_t s = 0; s < R.nsub; s++)
            if (sub[s + 1] < sub[s]) bad("round %zu: sub offsets fall at %u", r, s);
        gate_next = (size_t)R.gate_first + sub[R.nsub];
        sub_next = (size_t)R.sub_first + R.nsub + 1;
        max_nsub = std::max(max_nsub, R.nsub);
        if (R.nsub > I.max_free_depth) bad("round %zu: nsub %u > max_free_depth %u", r, R.nsub, I.max_free_depth);
    }
    if (gate_next != p.gates.size()) bad("rounds close %zu free gates, the plan holds %zu", gate_next, p.gates.size());
    if (p.gates.size() != (size_t)I.n_xor + I.n_xnor + I.n_inv) bad("%zu free gates, info counts %u", p.gates.size(), I.n_xor + I.n_xnor + I.n_inv);
    if (sub_next != p.sub.size()) bad("rounds use %zu sub offsets of %zu", sub_next, p.sub.size());
    if (idx_next != p.idx.size()) bad("rounds use %zu idx entries of %zu", idx_next, p.idx.size());
    if (n_and != I.n_and) bad("rounds open %zu ANDs, info counts %u", n_and, I.n_and);
    if (max_nsub != I.max_free_depth) bad("max_free_depth %u, rounds give %u", I.max_free_depth, max_nsub);
    return g_bad == before;
}

void walk(const GmwPlan &p, std::vector<Party> &party, uint32_t n) {
    const uint32_t P = (uint32_t)party.size(), ni = p.info.ninputs, no = p.info.noutputs;
    const uint64_t live = n == 64 ? ~0ull : (1ull << n) - 1;
    std::vector<int64_t> at(p.nslots, -1);  // phase that wrote the slot
    int64_t phase = 0;
    auto W = [&](uint32_t s) {
        if (s >= p.nslots) { bad("write of slot %u >= nslots %u in phase %" PRId64, s, p.nslots, phase); return false; }
        if (at[s] >= 0) { bad("slot %u written in phase %" PRId64 " and again in phase %" PRId64, s, at[s], phase); return false; }
        at[s] = phase;
        return true;
    };
    auto R = [&](uint32_t s) {
        if (s >= p.nslots) { bad("read of slot %u >= nslots %u in phase %" PRId64, s, p.nslots, phase); return false; }
        if (at[s] < 0) { bad("slot %u read in phase %" PRId64 " before any write", s, phase); return false; }
        if (at[s] >= phase) { bad("slot %u read in phase %" PRId64 ", the phase that writes it", s, phase); return false; }
        return true;
    };
    // the input launch (k_gmw_inputs): wire w of instance i is bit w % 64 of word w / 64
    for (Party &q : party) q.S.assign(p.nslots, 0);
    for (uint32_t w = 0; w < ni; w++) {
        if (!W(w)) continue;
        for (Party &q : party)
            for (uint32_t i = 0; i < n; i++) q.S[w] |= ((q.in[(size_t)(w / 64) * n + i] >> (w % 64)) & 1) << i;
    }
    phase++;
    for (size_t r = 0; r < p.rounds.size(); r++) {
        const GmwRound &Rr = p.rounds[r];
        // (1) close the previous AND level: z = c ^ d&b ^ e&a (^ d&e on party 0) from every party's d, e
        if (r && p.rounds[r - 1].and_n) {
            const GmwRound &pv = p.rounds[r - 1];
            for (uint32_t g = 0; g < pv.and_n; g++) {
                const uint32_t s = p.idx[pv.and_out + g];
                if (!W(s)) continue;
                const uint32_t k = g / 64, b = g % 64;
                for (uint32_t i = 0; i < n; i++) {
                    uint64_t d = 0, e = 0;
                    for (const Party &q : party) {
                        d ^= q.own[(size_t)k * n + i];
                        e ^= q.own[(size_t)(pv.and_w + k) * n + i];
                    }
                    for (uint32_t q = 0; q < P; q++) {
                        const size_t t = (size_t)(pv.and_W + k) * n + i;
                        const uint64_t z = party[q].tc[t] ^ (d & party[q].tb[t]) ^ (e & party[q].ta[t]) ^ (q == 0 ? d & e : 0);
                        party[q].S[s] |= ((z >> b) & 1) << i;
                    }
                }
            }
            phase++;
        }
        // (2) the free gates, a phase per sub-round
        for (uint32_t s = 0; s < Rr.nsub; s++) {
            const uint32_t b = p.sub[Rr.sub_first + s], e = p.sub[Rr.sub_first + s + 1];
            for (uint32_t i = b; i < e; i++) {
                const GmwGate &G = p.gates[Rr.gate_first + i];
                if (G.op != GC_XOR && G.op != GC_XNOR && G.op != GC_INV) { bad("free gate %u of round %zu has op %u", i, r, G.op); continue; }
                bool ok = R(G.in0);
                if (G.op != GC_INV) ok &= R(G.in1);
                else if (G.in1 != G.in0) bad("INV gate %u of round %zu: in1 %u != in0 %u", i, r, G.in1, G.in0);
                ok &= W(G.out);
                if (!ok) continue;
                for (uint32_t q = 0; q < P; q++) {
                    const uint64_t p0 = q == 0 ? live : 0;
                    uint64_t v = party[q].S[G.in0];
                    if (G.op == GC_INV) v ^= p0;
                    else {
                        v ^= party[q].S[G.in1];
                        if (G.op == GC_XNOR) v ^= p0;
                    }
                    party[q].S[G.out] = v;
                }
            }
            phase++;
        }
        // (3) open the round's AND level: d = x ^ a, e = y ^ b, padding bits 0 before the XOR
        std::printf("round %zu %u %u\n", r, Rr.level, Rr.and_w);
        for (uint32_t q = 0; q < P; q++) {
            Party &Q = party[q];
            Q.own.assign((size_t)2 * Rr.and_w * n, 0);
            for (uint32_t g = 0; g < Rr.and_n; g++) {
                const uint32_t s0 = p.idx[Rr.and_in + g], s1 = p.idx[Rr.and_in + Rr.and_n + g];
                if (q == 0 ? !(R(s0) & R(s1)) : (s0 >= p.nslots || s1 >= p.nslots)) continue;
                for (uint32_t i = 0; i < n; i++) {
                    Q.own[(size_t)(g / 64) * n + i] |= ((Q.S[s0] >> i) & 1) << (g % 64);
                    Q.own[(size_t)(Rr.and_w + g / 64) * n + i] |= ((Q.S[s1] >> i) & 1) << (g % 64);
                }
            }
            for (uint32_t k = 0; k < Rr.and_w; k++)
                for (uint32_t i = 0; i < n; i++) {
                    Q.own[(size_t)k * n + i] ^= Q.ta[(size_t)(Rr.and_W + k) * n + i];
                    Q.own[(size_t)(Rr.and_w + k) * n + i] ^= Q.tb[(size_t)(Rr.and_W + k) * n + i];
                }
            put("msg", q, Q.own);
        }
        // (4) the outputs, read in the phase of the open
        if (r + 1 == p.rounds.size()) {
            for (uint32_t q = 0; q < P; q++) {
                std::vector<uint64_t> o((size_t)((no + 63) / 64) * n, 0);
                for (uint32_t j = 0; j < no; j++) {
                    const uint32_t s = p.out_slots[j];
                    if (q == 0 ? !R(s) : s >= p.nslots) continue;
                    for (uint32_t i = 0; i < n; i++) o[(size_t)(j / 64) * n + i] |= ((party[q].S[s] >> i) & 1) << (j % 64);
                }
                put("out", q, o);
            }
        }
        phase++;  // the launch ends
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2 && argc != 3) return 2;
    // self-test of the checks: fold the second sub-round of every round into the first, as a planner that drops a barrier would
    const bool merge = argc == 3 && std::string(argv[2]) == "merge-sub-rounds";
    if (argc == 3 && !merge) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[7];
    int total_bad = 0;
    for (int K = 0; std::fread(h, 4, 7, f) == 7; K++) {
        const uint32_t ng = h[0], nw = h[1], ni = h[2], no = h[3], P = h[4], n = h[5], tw = h[6];
        if (P < 2 || n < 1 || n > 64) return 2;
        std::vector<gc_gate> gates;
        if (!rd(f, &gates, ng)) return 2;
        std::vector<Party> party(P);
        const size_t iw = (size_t)((ni + 63) / 64) * n, tws = (size_t)tw * n;
        for (Party &q : party)
            if (!rd(f, &q.in, iw) || !rd(f, &q.ta, tws) || !rd(f, &q.tb, tws) || !rd(f, &q.tc, tws)) return 2;
        GmwPlan p;
        const int rc = build_gmw_plan(gates.data(), ng, nw, ni, no, &p);
        std::printf("case %d rc %d\n", K, rc);
        if (rc != GC_OK) continue;
        if (merge)
            for (const GmwRound &R : p.rounds)
                if (R.nsub >= 2) p.sub[R.sub_first + 1] = p.sub[R.sub_first + 2];
        g_bad = 0;
        std::printf("plan %u %zu %u %u\n", p.nslots, p.rounds.size(), p.info.nlevels, p.info.n_and_levels);
        if (check_structure(p, tw)) walk(p, party, n);
        std::printf("end %d %d\n", K, g_bad);
        total_bad += g_bad;
    }
    std::fclose(f);
    return total_bad ? 1 : 0;
}
