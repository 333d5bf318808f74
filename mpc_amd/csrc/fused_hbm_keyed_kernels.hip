// fused_hbm_keyed_kernels.hip — the level-walking batch kernels with the wires in HBM and ONE AES KEY PER INSTANCE: what
// gc_batch_garble_keyed / gc_batch_eval_keyed run on a batch that the flattened keyed kernels (fused_flat_keyed_kernels.hip)
// cannot serve, a circuit whose live set fits no LDS plan.
//
// The loop is k_garble_col / k_eval_col (fused_kernels.hip): a 1024-thread workgroup owns a tile of TI instances and walks
// Plan::levels behind one __syncthreads() per level, the Step and this lane's GateDesc of the next level fetched before the
// barrier; wires at Wt[(wire << ti_log2) + inst], table rows at Tt[(row << ti_log2) + inst].  What differs:
//   * the prologue copies the tile's TI schedules (k_expand_keys: [batch][4 (NR + 1)] words, the last round key folded with
//     round key 0) into an LDS key table; instances of the last tile past the batch get zero keys and are not read;
//   * every hashed lane runs column-sliced (hash_col_whitened) with keyaddr = key table + inst * 16 (NR + 1) + 4 c, in any
//     number of passes of 1024 column lanes per level.  A gate-instance is a row of 16 lanes or a divisor of it and a pass
//     holds whole rows, so the DPP partners of a lane are always in its pass;
//   * OR gates take the same form (the algebra of garble_hash_keyed / eval_hash_keyed); HAS_OR = false compiles them out.
// The plain loop only: no hash-wave / free-wave split, no prefetch pipeline, no profiling build, no cooperative form.
// LDS map: 64 KiB AES table | R[64] | keys [TI][NR + 1] uint4 (at most 15 360 B).
#include "aes_device.h"
#include "col_lanes.h"
#include "kernels.h"

namespace gc {

namespace {

constexpr int kHbmKeyedThreads = 1024;
constexpr uint32_t kHbmKeyedR16 = kTeDualBytes / 16;          // uint4 index of R[64]
constexpr uint32_t kHbmKeyedKeyTab = kTeDualBytes + 64 * 16;  // LDS byte address of the key table

// column c of K ^ rk_0 with K = 2x ^ 4y ^ tweak (makeK, garble.go:74-83), the tweak in column 3
__device__ __forceinline__ uint32_t col_whiten_k(uint32_t xc, uint32_t xc1, uint32_t yc, uint32_t yc1, uint32_t c, uint32_t tweak,
                                                 uint32_t k0) {
    const uint32_t kx = __builtin_amdgcn_alignbit(xc, c == 3 ? 0u : xc1, 31);
    const uint32_t ky = __builtin_amdgcn_alignbit(yc, c == 3 ? 0u : yc1, 30);
    return xor3(kx, ky, k0) ^ (c == 3 ? tweak : 0u);
}
// value of the lane 8 further on / back inside the row of 16: the q ^ 2 partner of a garbler lane
__device__ __forceinline__ uint32_t col_pair8(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, true); }

// the tile's schedules into LDS; instances past the batch (the last tile) get zero keys and are not read
template <int NR>
__device__ __forceinline__ void load_tile_keys(uint32_t *keys, const uint32_t *__restrict__ rk, uint32_t ti_log2, uint32_t batch) {
    constexpr uint32_t kWords = 4 * (NR + 1);
    const uint32_t inst0 = blockIdx.x << ti_log2;
    for (uint32_t i = threadIdx.x; i < (kWords << ti_log2); i += kHbmKeyedThreads)
        keys[i] = inst0 + i / kWords < batch ? rk[(size_t)inst0 * kWords + i] : 0u;
}

// one lane of the garbler: garble_col_pass (fused_kernels.hip) with the instance's own key, and the OR gates
template <int NR, bool HAS_OR>
__device__ __forceinline__ void garble_hbm_keyed_pass(const Step &st, const ColPos &p, const GateDesc &d, uint32_t ninputs,
                                                      uint32_t ti_log2, uint32_t TI, uint4 *Wt, uint4 *Tt, const uint4 *Rt,
                                                      uint32_t lo) {
    if (p.kind == K_NONE) return;
    const uint32_t inst = p.inst;
    uint4 *outl = Wt + ((size_t)(ninputs + st.first + p.g) << ti_log2) + inst;
    const uint4 *la = Wt + ((size_t)d.in0 << ti_log2) + inst;
    if (p.kind == K_FREE) {
        uint4 v = lxor(*la, Wt[((size_t)d.in1 << ti_log2) + inst]);
        if ((d.row_op >> kOpShift) == GC_XNOR) v = lxor(v, Rt[inst]);  // garble.go:342-351
        *outl = v;
        return;
    }
    const uint32_t c = p.c, q = p.q, wo = (c ^ 1u) << 2, wo1 = (((c + 1u) ^ 1u) << 2) & 12u;
    const bool is_or = HAS_OR && p.kind == K_OR;
    const uint4 *lb = p.kind != K_INV ? Wt + ((size_t)d.in1 << ti_log2) + inst : la;
    const uint32_t keyaddr = kHbmKeyedKeyTab + inst * (16u * (NR + 1)) + (c << 2);
    const uint32_t a0c = label_word(la, wo), a0y = label_word(la, 4), b0y = label_word(lb, 4);
    const uint32_t rc = label_word(Rt + inst, wo), rc1 = label_word(Rt + inst, wo1);
    const uint32_t k0 = *(lds_u32 *)(uintptr_t)keyaddr;
    uint32_t s0;
    if (is_or) {  // e[q] = H(2x ^ 4y ^ id), x = a0 ^ (q & 2 ? R : 0), y = b0 ^ (q & 1 ? R : 0)  (garble.go:421-424)
        const uint32_t mx = (q & 2u) ? ~0u : 0u, my = (q & 1u) ? ~0u : 0u;
        const uint32_t xc = __builtin_amdgcn_bitop3_b32(a0c, rc, mx, 0x78);
        const uint32_t xc1 = __builtin_amdgcn_bitop3_b32(label_word(la, wo1), rc1, mx, 0x78);
        const uint32_t yc = __builtin_amdgcn_bitop3_b32(label_word(lb, wo), rc, my, 0x78);
        const uint32_t yc1 = __builtin_amdgcn_bitop3_b32(label_word(lb, wo1), rc1, my, 0x78);
        s0 = col_whiten_k(xc, xc1, yc, yc1, c, d.tweak, k0);
    } else {  // AND q = 0..3 hash a0, a1, b0, b1 (lanes 2, 3: tweak + 1); INV q = 0, 1 hash a0, a1
        const uint4 *lown = (q & 2u) ? lb : la;  // INV lanes have q < 2
        const uint32_t modd = (q & 1u) ? ~0u : 0u;
        const uint32_t xc = __builtin_amdgcn_bitop3_b32(label_word(lown, wo), rc, modd, 0x78);
        const uint32_t xc1 = __builtin_amdgcn_bitop3_b32(label_word(lown, wo1), rc1, modd, 0x78);
        s0 = col_whiten(xc, xc1, c, d.tweak + (q >> 1), k0);
    }
    const uint32_t h = hash_col_whitened<NR>(s0, keyaddr, lo);
    char *row0 = (char *)(Tt + ((size_t)(d.row_op & kRowMask) << ti_log2) + inst) + wo;
    const uint32_t pa = (uint32_t)((int32_t)a0y >> 31), pb = (uint32_t)((int32_t)b0y >> 31);
    const uint32_t x1 = col_pair4(h);  // the hash of lane q ^ 1
    if (p.kind == K_AND) {  // garble.go:353-395, one column
        const uint32_t pp = h ^ x1;
        const uint32_t m2 = (q & 2u) ? ~0u : 0u;
        const uint32_t mk = m2 ? pb : pa, rm = pb & ~m2;
        const uint32_t w = __builtin_amdgcn_bitop3_b32(pp, rc, rm, 0x78);
        const uint32_t tab = __builtin_amdgcn_bitop3_b32(w, a0c, m2, 0x78);
        const uint32_t v = __builtin_amdgcn_bitop3_b32(h, w, mk, 0x78);
        if (!(q & 1u)) *(uint32_t *)(row0 + (((q & 2u) ? (size_t)TI : 0) << 4)) = tab;
        uint32_t o = v ^ col_pair8(v);
        asm volatile("" : "+v"(o));
        if (q == 0) *(uint32_t *)((char *)outl + wo) = o;
    } else if (!is_or) {  // INV, garble.go:446-474
        const uint32_t pp = h ^ x1;
        if (q == 0) {
            *(uint32_t *)row0 = pp ^ rc;
            *(uint32_t *)((char *)outl + wo) = h ^ (((int32_t)a0y < 0) ? pp : rc);
        }
    } else {  // OR, garble.go:412-444: table[q] = e[q ^ l0] ^ (q == l0 ? c0 : c1), l0 = 2 S(a0) + S(b0)
        const uint32_t x2 = col_pair8(h), x3 = col_pair4(x2);  // the hashes of lanes q ^ 2, q ^ 3
        const uint32_t l0 = (pa & 2u) | (pb & 1u);
        auto pick = [&](uint32_t dist) { return dist == 0 ? h : dist == 1 ? x1 : dist == 2 ? x2 : x3; };
        const uint32_t tk = pick(l0), t0v = pick(q ^ l0);  // e[q ^ l0], e[l0]
        const uint32_t c0 = t0v ^ (l0 ? rc : 0u), c1 = t0v ^ (l0 ? 0u : rc);
        if (q != 0) *(uint32_t *)(row0 + (((size_t)(q - 1) << ti_log2) << 4)) = tk ^ (q == l0 ? c0 : c1);
        else *(uint32_t *)((char *)outl + wo) = c0;
    }
}

// one lane of the evaluator: eval_col_pass with the instance's own key, and the OR gates (eval.go:53-109)
template <int NR, bool HAS_OR>
__device__ __forceinline__ void eval_hbm_keyed_pass(const Step &st, const ColPos &p, const GateDesc &d, uint32_t ninputs,
                                                    uint32_t ti_log2, uint32_t TI, uint4 *Wt, const uint4 *Tt, uint32_t lo) {
    if (p.kind == K_NONE) return;
    const uint32_t inst = p.inst;
    uint4 *outl = Wt + ((size_t)(ninputs + st.first + p.g) << ti_log2) + inst;
    const uint4 *la = Wt + ((size_t)d.in0 << ti_log2) + inst;
    if (p.kind == K_FREE) {  // eval.go:49-51
        *outl = lxor(*la, Wt[((size_t)d.in1 << ti_log2) + inst]);
        return;
    }
    const uint32_t c = p.c, q = p.q, wo = (c ^ 1u) << 2, wo1 = (((c + 1u) ^ 1u) << 2) & 12u;
    const bool is_or = HAS_OR && p.kind == K_OR;
    const uint4 *lb = p.kind != K_INV ? Wt + ((size_t)d.in1 << ti_log2) + inst : la;
    const uint4 *lown = q ? lb : la;  // AND lane 1 hashes operand b (INV, OR: q = 0)
    const uint32_t keyaddr = kHbmKeyedKeyTab + inst * (16u * (NR + 1)) + (c << 2);
    const uint4 *row = Tt + ((size_t)(d.row_op & kRowMask) << ti_log2) + inst;
    const uint32_t xc = label_word(lown, wo), xc1 = label_word(lown, wo1), xy = label_word(lown, 4);
    const uint32_t ac = label_word(la, wo), k0 = *(lds_u32 *)(uintptr_t)keyaddr;
    uint32_t s0, tab = 0;
    if (is_or) {  // eval.go:80-94: both operands, row index - 1 (index 0 has no row)
        const uint32_t index = (xy >> 31) * 2u + (label_word(lb, 4) >> 31);
        if (index > 0) tab = label_word(row + ((size_t)(index - 1) << ti_log2), wo);
        s0 = col_whiten_k(xc, xc1, label_word(lb, wo), label_word(lb, wo1), c, d.tweak, k0);
    } else {  // AND: lane q hashes operand q with tweak + q and needs table row q; INV: operand a, row 0
        tab = label_word(row + (q ? TI : 0u), wo);
        s0 = col_whiten(xc, xc1, c, d.tweak + q, k0);
    }
    const uint32_t h = hash_col_whitened<NR>(s0, keyaddr, lo);
    const uint32_t sm = (uint32_t)((int32_t)xy >> 31);
    if (p.kind == K_AND) {  // eval.go:53-78: lane 0 WG = H(a) ^ (sa ? TG : 0), lane 1 WE = H(b) ^ (sb ? TE ^ a : 0)
        const uint32_t v = __builtin_amdgcn_bitop3_b32(h, __builtin_amdgcn_bitop3_b32(tab, ac, q ? ~0u : 0u, 0x78), sm, 0x78);
        uint32_t o = v ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x104, 0xf, 0xf, true);  // + the lane 4 further on (q = 1)
        asm volatile("" : "+v"(o));
        if (q == 0) *(uint32_t *)((char *)outl + wo) = o;
    } else if (!is_or) {  // eval.go:96-109
        *(uint32_t *)((char *)outl + wo) = __builtin_amdgcn_bitop3_b32(h, tab, sm, 0x78);
    } else {  // (tab is zero for index 0)
        *(uint32_t *)((char *)outl + wo) = h ^ tab;
    }
}

}  // namespace

// rk: the expanded keys of the whole batch (k_expand_keys)
template <int NR, bool HAS_OR>
__global__ __launch_bounds__(kHbmKeyedThreads) void k_garble_hbm_keyed(const GateDesc *__restrict__ descs, const Step *__restrict__ steps,
                                                                       uint32_t nsteps, uint32_t ninputs, uint32_t ti_log2,
                                                                       uint32_t batch, size_t w_tile, size_t t_tile,
                                                                       uint4 *__restrict__ W, const uint4 *__restrict__ Rv,
                                                                       uint4 *__restrict__ T, const uint32_t *__restrict__ rk,
                                                                       const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    uint32_t *te = (uint32_t *)smem;
    uint4 *Rt = smem + kHbmKeyedR16;
    load_te_dual(te, g_te0);
    load_tile_keys<NR>(te + kHbmKeyedKeyTab / 4, rk, ti_log2, batch);
    const uint32_t TI = 1u << ti_log2, tim = TI - 1;
    if (threadIdx.x < TI) Rt[threadIdx.x] = Rv[(size_t)blockIdx.x * TI + threadIdx.x];
    __syncthreads();
    const uint32_t lo = te_lane_off();
    uint4 *Wt = W + (size_t)blockIdx.x * w_tile;
    uint4 *Tt = T + (size_t)blockIdx.x * t_tile;
    Step st_next = steps[0];
    ColPos cp_next = col_classify<2, 1, HAS_OR, 2>(st_next, threadIdx.x, ti_log2, tim);
    GateDesc d_next = descs[st_next.first + cp_next.g];
    for (uint32_t lv = 0; lv < nsteps; lv++) {
        const Step st = st_next;
        garble_hbm_keyed_pass<NR, HAS_OR>(st, cp_next, d_next, ninputs, ti_log2, TI, Wt, Tt, Rt, lo);
        const uint32_t lanes = col_lanes<2, 1, true, 2>(st, ti_log2);
        for (uint32_t J = kHbmKeyedThreads; J < lanes; J += kHbmKeyedThreads) {  // the further passes of a wide level
            const ColPos cp = col_classify<2, 1, HAS_OR, 2>(st, J + threadIdx.x, ti_log2, tim);
            garble_hbm_keyed_pass<NR, HAS_OR>(st, cp, descs[st.first + cp.g], ninputs, ti_log2, TI, Wt, Tt, Rt, lo);
        }
        if (lv + 1 < nsteps) {
            st_next = steps[lv + 1];
            cp_next = col_classify<2, 1, HAS_OR, 2>(st_next, threadIdx.x, ti_log2, tim);
            d_next = descs[st_next.first + cp_next.g];
        }
        __syncthreads();
    }
}

template <int NR, bool HAS_OR>
__global__ __launch_bounds__(kHbmKeyedThreads) void k_eval_hbm_keyed(const GateDesc *__restrict__ descs, const Step *__restrict__ steps,
                                                                     uint32_t nsteps, uint32_t ninputs, uint32_t ti_log2,
                                                                     uint32_t batch, size_t w_tile, size_t t_tile,
                                                                     uint4 *__restrict__ W, const uint4 *__restrict__ T,
                                                                     const uint32_t *__restrict__ rk,
                                                                     const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    uint32_t *te = (uint32_t *)smem;
    load_te_dual(te, g_te0);
    load_tile_keys<NR>(te + kHbmKeyedKeyTab / 4, rk, ti_log2, batch);
    __syncthreads();
    const uint32_t TI = 1u << ti_log2, tim = TI - 1;
    const uint32_t lo = te_lane_off();
    uint4 *Wt = W + (size_t)blockIdx.x * w_tile;
    const uint4 *Tt = T + (size_t)blockIdx.x * t_tile;
    Step st_next = steps[0];
    ColPos cp_next = col_classify<1, 0, HAS_OR, 0>(st_next, threadIdx.x, ti_log2, tim);
    GateDesc d_next = descs[st_next.first + cp_next.g];
    for (uint32_t lv = 0; lv < nsteps; lv++) {
        const Step st = st_next;
        eval_hbm_keyed_pass<NR, HAS_OR>(st, cp_next, d_next, ninputs, ti_log2, TI, Wt, Tt, lo);
        const uint32_t lanes = col_lanes<1, 0, true, 0>(st, ti_log2);
        for (uint32_t J = kHbmKeyedThreads; J < lanes; J += kHbmKeyedThreads) {
            const ColPos cp = col_classify<1, 0, HAS_OR, 0>(st, J + threadIdx.x, ti_log2, tim);
            eval_hbm_keyed_pass<NR, HAS_OR>(st, cp, descs[st.first + cp.g], ninputs, ti_log2, TI, Wt, Tt, lo);
        }
        if (lv + 1 < nsteps) {
            st_next = steps[lv + 1];
            cp_next = col_classify<1, 0, HAS_OR, 0>(st_next, threadIdx.x, ti_log2, tim);
            d_next = descs[st_next.first + cp_next.g];
        }
        __syncthreads();
    }
}

size_t fused_hbm_keyed_bytes(uint32_t ti_log2, int rounds) { return kHbmKeyedKeyTab + ((size_t)16 * (rounds + 1) << ti_log2); }

hipError_t launch_fused_hbm_keyed(bool eval, const FusedArgs &a, const uint32_t *rk_per_instance, bool has_or, const BatchGeom &g,
                                  hipStream_t s) {
    if (a.nsteps == 0) return hipSuccess;
    if (g.ti_log2 > 6 || !rk_per_instance) return hipErrorInvalidValue;
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
                return launch_with_lds(k_eval_hbm_keyed<NR, OR>, grid, block, lds, s, a.descs, a.steps, a.nsteps, a.ninputs,
                                       g.ti_log2, g.batch, wt, tt, a.W, Tc, rk_per_instance, a.te0);
            return launch_with_lds(k_garble_hbm_keyed<NR, OR>, grid, block, lds, s, a.descs, a.steps, a.nsteps, a.ninputs, g.ti_log2,
                                   g.batch, wt, tt, a.W, a.R, a.T, rk_per_instance, a.te0);
        });
    });
}

}  // namespace gc
