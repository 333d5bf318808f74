// fused_hbm_keyed_split_kernels.hip — the SPLIT FORM of the keyed HBM-wire kernels (path 2 of gc_batch_keyed_path, one AES key
// per instance): the geometry, layouts, LDS map and launch of fused_hbm_keyed_kernels.hip and the same bytes, with the wide
// levels of fused_kernels.hip ("wide levels: hash waves and free waves").
//
// A level of at most 1 024 column lanes runs the plain single pass.  On a wider level the first H waves hash and the other
// 16 - H stream the free gates (hbm_keyed_split.h: which levels, how many waves, which lane does what):
//   hash waves  walk the AND / OR / INV column lanes, 64 H per pass, as a software pipeline of depth one: the label words,
//               the evaluator's table word and the descriptor of pass p + 1 (the descriptor of p + 2) are in flight under the
//               AES of pass p, the one vmcnt(0) sits behind the hash and the stores behind that.  R and the round keys come
//               from LDS.  The two word sets alternate (A, B) so that no loaded register is copied, and every load of the
//               pipeline is unconditional: an idle lane re-reads the level's first descriptor and its operands, nothing is
//               zero-filled (the reasons are in fused_kernels.hip).  The table row of an evaluator's OR lane depends on two
//               loaded select bits and is read in front of its hash, as in the one-key kernels.
//   free waves  stream the XOR / XNOR lanes in groups of four passes; the garbler adds R for XNOR.
// No barrier inside a role; every wave reaches the level's one __syncthreads().  The Step, H, this lane's descriptor of pass 0
// and a hash wave's descriptor of pass 1 of the NEXT level are fetched before the barrier.
#include "hbm_keyed_pass.h"
#include "hbm_keyed_split.h"

namespace gc {

namespace {

// lane position in one register (the pipeline keeps three alive): kind | q << 3 | c << 5 | inst << 8
__device__ __forceinline__ uint32_t hks_pack(const ColPos &p) { return p.kind | (p.q << 3) | (p.c << 5) | (p.inst << 8); }
__device__ __forceinline__ ColPos hks_unpack(uint32_t pos, uint32_t g) {
    return ColPos{pos & 7u, g, pos >> 8, (pos >> 3) & 3u, (pos >> 5) & 3u};
}

struct HksDesc {
    uint32_t pos, g;
    GateDesc d;
};
template <bool EVAL>
struct HksIn;
template <>
struct HksIn<false> {
    uint32_t pos, g, tweak, row_op;
    GarbleColWords w;
};
template <>
struct HksIn<true> {
    uint32_t pos, g, tweak, row_op;
    EvalColWords w;
};

template <bool EVAL, bool HAS_OR>
__device__ __forceinline__ ColPos hks_classify(const Step &st, uint32_t J, uint32_t ti_log2, uint32_t tim) {
    if constexpr (EVAL) return col_classify<1, 0, HAS_OR, 0>(st, J, ti_log2, tim);
    else return col_classify<2, 1, HAS_OR, 2>(st, J, ti_log2, tim);
}

// position and descriptor of column lane J of a hash wave (kHksIdle: K_NONE, the level's first descriptor)
template <bool EVAL, bool HAS_OR>
__device__ __forceinline__ void hks_fetch_desc(HksDesc &o, const Step &st, uint32_t J, const GateDesc *__restrict__ descs,
                                               uint32_t ti_log2, uint32_t tim) {
    ColPos p = hks_classify<EVAL, HAS_OR>(st, J, ti_log2, tim);
    if (J == kHksIdle) p.kind = K_NONE;
    o.pos = hks_pack(p);
    o.g = p.g;
    o.d = descs[st.first + p.g];
}

template <bool EVAL, bool HAS_OR>
__device__ __forceinline__ void hks_issue(HksIn<EVAL> &o, const HksDesc &dn, uint32_t ti_log2, uint32_t TI, const uint4 *Wt,
                                          const uint4 *Tt) {
    o.pos = dn.pos;
    o.g = dn.g;
    o.tweak = dn.d.tweak;
    o.row_op = dn.d.row_op;
    // (fields first, selection after: a select between two struct fields becomes a select between two addresses)
    const uint32_t in0 = dn.d.in0, in1 = dn.d.in1;
    const ColPos p = hks_unpack(dn.pos, dn.g);
    if constexpr (EVAL) eval_hbm_keyed_issue<HAS_OR>(o.w, p, in0, in1, dn.d.row_op, ti_log2, TI, Wt, Tt);
    else garble_hbm_keyed_issue<HAS_OR>(o.w, p, in0, in1, ti_log2, Wt);
}

// one pass of a hash wave: cur holds the words of this pass, nxt receives those of the next one, dn the descriptor after that
template <int NR, bool EVAL, bool HAS_OR, typename TT>
__device__ __forceinline__ void hks_hash_step(const Step &st, uint32_t J_next2, HksDesc &dn, const HksIn<EVAL> &cur,
                                              HksIn<EVAL> &nxt, const GateDesc *__restrict__ descs, uint32_t ninputs,
                                              uint32_t ti_log2, uint32_t tim, uint32_t TI, uint4 *Wt, TT *Tt, const uint4 *Rt,
                                              uint32_t lo) {
    hks_issue<EVAL, HAS_OR>(nxt, dn, ti_log2, TI, Wt, Tt);
    hks_fetch_desc<EVAL, HAS_OR>(dn, st, J_next2, descs, ti_log2, tim);
    const ColPos p = hks_unpack(cur.pos, cur.g);
    if (p.kind == K_NONE) return;
    if constexpr (EVAL) eval_hbm_keyed_finish<NR, HAS_OR, true>(st, p, cur.w, cur.tweak, cur.row_op, ninputs, ti_log2, Wt, Tt, lo);
    else garble_hbm_keyed_finish<NR, HAS_OR, true>(st, p, cur.w, cur.tweak, cur.row_op, ninputs, ti_log2, TI, Wt, Tt, Rt, lo);
}

// the hash waves of a wide level.  d0 / pre1: the descriptors of passes 0 and 1, fetched before the previous level's barrier
template <int NR, bool EVAL, bool HAS_OR, typename TT>
__device__ __forceinline__ void hks_hash_role(const Step &st, uint32_t e_hash, uint32_t H, uint32_t wave, uint32_t pos0,
                                              uint32_t g0, const GateDesc &d0, const HksDesc &pre1, const GateDesc *__restrict__ descs, uint32_t ninputs,
                                              uint32_t ti_log2, uint32_t tim, uint32_t TI, uint4 *Wt, TT *Tt, const uint4 *Rt,
                                              uint32_t lo) {
    const uint32_t NP = hks_hash_passes(e_hash, H), lane = threadIdx.x & 63u;
    HksIn<EVAL> A, B;
    HksDesc dn;
    dn.pos = pos0;
    dn.g = g0;
    dn.d = d0;
    hks_issue<EVAL, HAS_OR>(A, dn, ti_log2, TI, Wt, Tt);
    dn = pre1;
    for (uint32_t p = 0; p < NP; p += 2) {
        hks_hash_step<NR, EVAL, HAS_OR>(st, hks_hash_lane(e_hash, H, wave, p + 2, lane), dn, A, B, descs, ninputs, ti_log2, tim, TI,
                                        Wt, Tt, Rt, lo);
        if (p + 1 < NP)
            hks_hash_step<NR, EVAL, HAS_OR>(st, hks_hash_lane(e_hash, H, wave, p + 3, lane), dn, B, A, descs, ninputs, ti_log2, tim,
                                            TI, Wt, Tt, Rt, lo);
    }
}

// the free waves: groups of kHksFreeGroup passes, descriptors, then operands, then the stores (free_role of fused_kernels.hip).
// A lane without a gate re-reads the level's first descriptor.
template <bool GARBLE>
__device__ __forceinline__ void hks_free_role(const Step &st, uint32_t n_free, uint32_t H, uint32_t wave,
                                              const GateDesc *__restrict__ descs, uint32_t ninputs, uint32_t ti_log2, uint32_t tim,
                                              uint4 *Wt, const uint4 *Rt) {
    const uint32_t NP = hks_free_passes(n_free, H), lane = threadIdx.x & 63u;
    for (uint32_t p0 = 0; p0 < NP; p0 += kHksFreeGroup) {
        uint32_t gate[kHksFreeGroup], inst[kHksFreeGroup];
        bool on[kHksFreeGroup];
        GateDesc d[kHksFreeGroup];
        uint4 va[kHksFreeGroup], vb[kHksFreeGroup];
#pragma unroll
        for (uint32_t p = 0; p < kHksFreeGroup; p++) {
            const uint32_t u = hks_free_lane(n_free, H, wave, p0 + p, lane);
            on[p] = u != kHksIdle;
            gate[p] = on[p] ? st.nonfree + (u >> ti_log2) : 0u;
            inst[p] = on[p] ? u & tim : 0u;
            d[p] = descs[st.first + gate[p]];
        }
#pragma unroll
        for (uint32_t p = 0; p < kHksFreeGroup; p++) {
            va[p] = Wt[((size_t)d[p].in0 << ti_log2) + inst[p]];
            vb[p] = Wt[((size_t)d[p].in1 << ti_log2) + inst[p]];
        }
#pragma unroll
        for (uint32_t p = 0; p < kHksFreeGroup; p++) {
            uint4 v = lxor(va[p], vb[p]);
            if (GARBLE && (d[p].row_op >> kOpShift) == GC_XNOR) v = lxor(v, Rt[inst[p]]);
            if (on[p]) Wt[((size_t)(ninputs + st.first + gate[p]) << ti_log2) + inst[p]] = v;
        }
    }
}

// what a lane knows of a level before the barrier in front of it: the Step, the split (H: hash waves of a wide level), its
// position and descriptor in pass 0 (a narrow level: lane threadIdx.x of the single pass) and, in a hash wave, those of pass 1
// (scalars and not one record: a record of these goes to scratch)
#define GC_HKS_LEVEL(v) Step v##_st; uint32_t v##_eh, v##_nf, v##_H, v##_pos0, v##_g0; bool v##_wide; GateDesc v##_d0; HksDesc v##_d1
template <bool EVAL, bool HAS_OR>
__device__ __forceinline__ void hks_prefetch(Step &st, uint32_t &e_hash, uint32_t &n_free, uint32_t &H, bool &wide, uint32_t &pos0,
                                             uint32_t &g0, GateDesc &d0, HksDesc &d1, const Step *__restrict__ steps, uint32_t lv,
                                             const GateDesc *__restrict__ descs, uint32_t ti_log2, uint32_t tim, uint32_t wave,
                                             uint32_t tune) {
    st = steps[lv];
    e_hash = hks_hash_lanes(st, ti_log2, EVAL);
    n_free = hks_free_lanes(st, ti_log2);
    wide = hks_level_wide(st, ti_log2, EVAL);
    H = wide ? hks_hash_waves(e_hash, n_free, EVAL, tune) : 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t J0 = wide ? hks_hash_lane(e_hash, H, wave, 0, lane) : threadIdx.x;
    ColPos p = hks_classify<EVAL, HAS_OR>(st, J0, ti_log2, tim);
    if (J0 == kHksIdle) p.kind = K_NONE;
    pos0 = hks_pack(p);
    g0 = p.g;
    d0 = descs[st.first + p.g];
    if (wide && wave < H) hks_fetch_desc<EVAL, HAS_OR>(d1, st, hks_hash_lane(e_hash, H, wave, 1, lane), descs, ti_log2, tim);
}
#define GC_HKS_PREFETCH(EVAL, v, lv) \
    hks_prefetch<EVAL, HAS_OR>(v##_st, v##_eh, v##_nf, v##_H, v##_wide, v##_pos0, v##_g0, v##_d0, v##_d1, steps, lv, descs, ti_log2, tim, wave, tune)

}  // namespace

// rk: the expanded keys of the whole batch (k_expand_keys); tune: hash waves of every split level (0: the rule)
template <int NR, bool HAS_OR>
__global__ __launch_bounds__(kHbmKeyedThreads) void k_garble_hbm_keyed_split(const GateDesc *__restrict__ descs,
                                                                             const Step *__restrict__ steps, uint32_t nsteps,
                                                                             uint32_t ninputs, uint32_t ti_log2, uint32_t batch,
                                                                             size_t w_tile, size_t t_tile, uint4 *__restrict__ W,
                                                                             const uint4 *__restrict__ Rv, uint4 *__restrict__ T,
                                                                             const uint32_t *__restrict__ rk,
                                                                             const uint32_t *__restrict__ g_te0, uint32_t tune) {
    extern __shared__ uint4 smem[];
    uint32_t *te = (uint32_t *)smem;
    uint4 *Rt = smem + kHbmKeyedR16;
    load_te_dual(te, g_te0);
    load_tile_keys<NR>(te + kHbmKeyedKeyTab / 4, rk, ti_log2, batch);
    const uint32_t TI = 1u << ti_log2, tim = TI - 1;
    if (threadIdx.x < TI) Rt[threadIdx.x] = Rv[(size_t)blockIdx.x * TI + threadIdx.x];
    __syncthreads();
    const uint32_t lo = te_lane_off();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint4 *Wt = W + (size_t)blockIdx.x * w_tile;
    uint4 *Tt = T + (size_t)blockIdx.x * t_tile;
    GC_HKS_LEVEL(nx);
    GC_HKS_PREFETCH(false, nx, 0);
    for (uint32_t lv = 0; lv < nsteps; lv++) {
        const Step st = nx_st;
        const uint32_t e_hash = nx_eh, n_free = nx_nf, H = nx_H;
        if (!nx_wide)
            garble_hbm_keyed_pass<NR, HAS_OR>(st, hks_unpack(nx_pos0, nx_g0), nx_d0, ninputs, ti_log2, TI, Wt, Tt, Rt, lo);
        else if (wave < H)
            hks_hash_role<NR, false, HAS_OR>(st, e_hash, H, wave, nx_pos0, nx_g0, nx_d0, nx_d1, descs, ninputs, ti_log2, tim, TI, Wt,
                                             Tt, Rt, lo);
        else
            hks_free_role<true>(st, n_free, H, wave, descs, ninputs, ti_log2, tim, Wt, Rt);
        if (lv + 1 < nsteps) GC_HKS_PREFETCH(false, nx, lv + 1);
        __syncthreads();
    }
}

template <int NR, bool HAS_OR>
__global__ __launch_bounds__(kHbmKeyedThreads) void k_eval_hbm_keyed_split(const GateDesc *__restrict__ descs,
                                                                           const Step *__restrict__ steps, uint32_t nsteps,
                                                                           uint32_t ninputs, uint32_t ti_log2, uint32_t batch,
                                                                           size_t w_tile, size_t t_tile, uint4 *__restrict__ W,
                                                                           const uint4 *__restrict__ T,
                                                                           const uint32_t *__restrict__ rk,
                                                                           const uint32_t *__restrict__ g_te0, uint32_t tune) {
    extern __shared__ uint4 smem[];
    uint32_t *te = (uint32_t *)smem;
    load_te_dual(te, g_te0);
    load_tile_keys<NR>(te + kHbmKeyedKeyTab / 4, rk, ti_log2, batch);
    __syncthreads();
    const uint32_t TI = 1u << ti_log2, tim = TI - 1;
    const uint32_t lo = te_lane_off();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint4 *Wt = W + (size_t)blockIdx.x * w_tile;
    const uint4 *Tt = T + (size_t)blockIdx.x * t_tile;
    GC_HKS_LEVEL(nx);
    GC_HKS_PREFETCH(true, nx, 0);
    for (uint32_t lv = 0; lv < nsteps; lv++) {
        const Step st = nx_st;
        const uint32_t e_hash = nx_eh, n_free = nx_nf, H = nx_H;
        if (!nx_wide)
            eval_hbm_keyed_pass<NR, HAS_OR>(st, hks_unpack(nx_pos0, nx_g0), nx_d0, ninputs, ti_log2, TI, Wt, Tt, lo);
        else if (wave < H)
            hks_hash_role<NR, true, HAS_OR>(st, e_hash, H, wave, nx_pos0, nx_g0, nx_d0, nx_d1, descs, ninputs, ti_log2, tim, TI, Wt,
                                            Tt, (const uint4 *)nullptr, lo);
        else
            hks_free_role<false>(st, n_free, H, wave, descs, ninputs, ti_log2, tim, Wt, nullptr);
        if (lv + 1 < nsteps) GC_HKS_PREFETCH(true, nx, lv + 1);
        __syncthreads();
    }
}

hipError_t launch_fused_hbm_keyed_split(bool eval, const FusedArgs &a, const uint32_t *rk_per_instance, bool has_or,
                                        const BatchGeom &g, uint32_t tune, hipStream_t s) {
    if (a.nsteps == 0) return hipSuccess;
    if (g.ti_log2 > 6 || !rk_per_instance || tune >= kHksWaves) return hipErrorInvalidValue;
    const size_t lds = fused_hbm_keyed_bytes(g.ti_log2, a.rounds);
    if (lds > kFlatLdsBytes) return hipErrorInvalidConfiguration;  // (the LDS of a CU: never with TI <= 64)
    const dim3 grid(g.ntiles), block(kHbmKeyedThreads);
    const size_t wt = g.lw.tile_stride, tt = g.lt.tile_stride;
    const uint4 *Tc = a.T;
    return with_rounds(a.rounds, [&](auto nr) {
        return with_flag(has_or, [&](auto has_or_t) {
            constexpr int NR = decltype(nr)::value;
            constexpr bool OR = decltype(has_or_t)::value;
            if (eval)
                return launch_with_lds(k_eval_hbm_keyed_split<NR, OR>, grid, block, lds, s, a.descs, a.steps, a.nsteps, a.ninputs,
                                       g.ti_log2, g.batch, wt, tt, a.W, Tc, rk_per_instance, a.te0, tune);
            return launch_with_lds(k_garble_hbm_keyed_split<NR, OR>, grid, block, lds, s, a.descs, a.steps, a.nsteps, a.ninputs,
                                   g.ti_log2, g.batch, wt, tt, a.W, a.R, a.T, rk_per_instance, a.te0, tune);
        });
    });
}

}  // namespace gc
