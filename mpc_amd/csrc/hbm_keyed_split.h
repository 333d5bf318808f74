// hbm_keyed_split.h — the index arithmetic of the split form of the keyed HBM-wire kernels (fused_hbm_keyed_split_kernels.hip):
// which levels split the workgroup into hash waves and free waves, how many hash waves a level gets, and which column lane J
// or free lane u a (wave, pass, lane of the wave) of a role handles.  The kernels use these functions and nothing else for
// that arithmetic.  Plain C++ without HIP types: hipcc compiles it for host and device, g++ for the walk of
// tests/test_hbm_keyed_split_index_host.py.
//
// A level in column form (col_lanes.h): four lanes per AES block, lane J = 4 * (hash lane of the wide form) + column; the
// level's AND, OR and INV gate-instances come first, in that order, each a row of 4 << LQ lanes (garbler: AND 16, OR 16,
// INV 8; evaluator: AND 8, OR 4, INV 4), the free lanes u = (gate - nonfree) << ti_log2 | inst behind them.  A level of at
// most kHksThreads lanes is ONE pass of the whole workgroup (the plain form's single pass).  A wider level is split:
//   hash waves  the first H waves; pass p of wave w, lane l: J = (p * H + w) * 64 + l while J < e_hash, idle beyond.  Rows
//               start at multiples of their length and a wave's pass is 64 consecutive lanes from a multiple of 64, so every
//               row lies in one wave and one pass: the DPP partners of a lane (q ^ 1, q ^ 2, the columns of its block) are in
//               its pass.  An idle lane answers kHksIdle, which col_classify turns into K_NONE with gate 0 and instance 0: it
//               re-reads the level's first descriptor and that gate's operands, addresses inside the tile's arrays.
//   free waves  the other 16 - H; pass p of wave w >= H, lane l: u = (p * (16 - H) + (w - H)) * 64 + l while u < n_free.
// H depends on the Step alone (and the developer's fixed value), so it is wave-uniform and known before the level's barrier.
#pragma once

#include <cstdint>

#include "plan.h"

#if defined(__HIPCC__)
#define GC_HKS_FN __host__ __device__ inline
#else
#define GC_HKS_FN inline
#endif

namespace gc {

constexpr uint32_t kHksThreads = 1024;  // lanes of the workgroup
constexpr uint32_t kHksWaves = 16;
constexpr uint32_t kHksFreeGroup = 4;       // passes a free wave keeps in flight
constexpr uint32_t kHksIdle = 0xffffffffu;  // no lane of the level
// free lanes that cost a wave what one column lane costs it, in tenths, per role: where the H sweep of the synthetic row
// (W = 1 024, f = 0.17, x 1 024, tiles of four: 11 136 garbler / 5 568 evaluator column lanes beside 3 400 free lanes a level)
// had its optimum, H = 14 for the garbler (any value from 1.7 to 2.9 gives it) and H = 12 for the evaluator (1.6 to 2.1):
// profiles/batch_keyed_hbm_split_hsweep.txt.  A quarter of an AES block with its round keys read from LDS costs a wave about
// what two 64-byte XOR lanes cost it.
constexpr uint32_t kHksFreePerHashGarble10 = 21;
constexpr uint32_t kHksFreePerHashEval10 = 18;
// the rule takes the split form when the plan's wide levels hold at least this many passes of 1 024 lanes on average: a hash
// wave's pipeline spends one pass filling, so a level of two passes gains little or loses (aes_128 x 1 024, 2.3 / 1.7 passes a
// wide level: the garbler 5 % slower than the plain form, the evaluator 2 % faster; the synthetic row, 14 / 9 passes, 1.5 times
// as fast)
constexpr uint32_t kHksRulePasses = 3;

// column lanes of a level's hashed gates / its free lanes; with both below 2^32 as for col_lanes
GC_HKS_FN uint32_t hks_hash_lanes(const Step &st, uint32_t ti_log2, bool eval) {
    const uint32_t blocks = eval ? (st.n_and << 1) + st.n_or + st.n_inv : (st.n_and << 2) + (st.n_or << 2) + (st.n_inv << 1);
    return (blocks << ti_log2) << 2;
}
GC_HKS_FN uint32_t hks_free_lanes(const Step &st, uint32_t ti_log2) { return (st.count - st.nonfree) << ti_log2; }
// the level takes the split: more lanes than one pass of the workgroup
GC_HKS_FN bool hks_level_wide(const Step &st, uint32_t ti_log2, bool eval) {
    return (uint64_t)hks_hash_lanes(st, ti_log2, eval) + hks_free_lanes(st, ti_log2) > kHksThreads;
}

// hash waves of a wide level.  No free gates -> 16, no hashed gates -> 0, never more hash waves than the level has lanes for;
// else the waves are shared out in proportion to the work, at least one and at most eight of them free.  tune 1 .. 15: fixed.
GC_HKS_FN uint32_t hks_hash_waves(uint32_t e_hash, uint32_t n_free, bool eval, uint32_t tune) {
    if (n_free == 0) return kHksWaves;
    if (e_hash == 0) return 0;
    const uint32_t need = (uint32_t)(((uint64_t)e_hash + 63) >> 6);
    if (tune) return need < tune ? need : tune;
    const uint64_t k = eval ? kHksFreePerHashEval10 : kHksFreePerHashGarble10;
    const uint64_t den = 10ull * n_free + k * e_hash;
    uint32_t F = (uint32_t)((160ull * n_free + (den >> 1)) / den);
    F = F < 1 ? 1 : F > 8 ? 8 : F;
    const uint32_t H = kHksWaves - F;
    return need < H ? need : H;
}

// passes of the two roles (H hash waves, 16 - H free waves)
GC_HKS_FN uint32_t hks_hash_passes(uint32_t e_hash, uint32_t H) {
    return H ? (uint32_t)(((uint64_t)e_hash + (H << 6) - 1) / (H << 6)) : 0;
}
GC_HKS_FN uint32_t hks_free_passes(uint32_t n_free, uint32_t H) {
    const uint32_t lp = (kHksWaves - H) << 6;
    return lp ? (uint32_t)(((uint64_t)n_free + lp - 1) / lp) : 0;
}
// column lane of hash wave `wave` < H, its pass and lane; kHksIdle: none (a free wave asks this for its prefetch, too)
GC_HKS_FN uint32_t hks_hash_lane(uint32_t e_hash, uint32_t H, uint32_t wave, uint32_t pass, uint32_t lane) {
    if (wave >= H) return kHksIdle;
    const uint64_t J = (((uint64_t)pass * H + wave) << 6) + lane;
    return J < e_hash ? (uint32_t)J : kHksIdle;
}
// free lane of wave `wave` >= H
GC_HKS_FN uint32_t hks_free_lane(uint32_t n_free, uint32_t H, uint32_t wave, uint32_t pass, uint32_t lane) {
    if (wave < H) return kHksIdle;
    const uint64_t u = (((uint64_t)pass * (kHksWaves - H) + (wave - H)) << 6) + lane;
    return u < n_free ? (uint32_t)u : kHksIdle;
}

// the form rule: which kernels a keyed path-2 pass runs.  setting: gc_batch_set_keyed_hbm_form (0 the rule, 1 plain, 2 split);
// the rule: the plan has wide levels in this role's lane count and they average kHksRulePasses passes or more
inline bool hks_plan_splits(const Step *levels, uint32_t nsteps, uint32_t ti_log2, bool eval) {
    uint64_t nwide = 0, lanes = 0;
    for (uint32_t i = 0; i < nsteps; i++)
        if (hks_level_wide(levels[i], ti_log2, eval)) {
            nwide++;
            lanes += (uint64_t)hks_hash_lanes(levels[i], ti_log2, eval) + hks_free_lanes(levels[i], ti_log2);
        }
    return nwide != 0 && lanes >= nwide * kHksRulePasses * kHksThreads;
}
inline int hks_form(int setting, bool plan_splits) { return setting == 1 || setting == 2 ? setting : plan_splits ? 2 : 1; }

}  // namespace gc
