// hbm_keyed_pass.h — one column lane of the split form of the keyed HBM-wire kernels (fused_hbm_keyed_split_kernels.hip: one AES
// key per instance, round keys in an LDS key table): the per-lane algebra of fused_hbm_keyed_kernels.hip cut in two.  *_issue
// loads the words of a hashed lane's operand labels (and the evaluator's table word), *_finish whitens, hashes and stores.  A
// narrow level runs them back to back (garble_hbm_keyed_pass / eval_hbm_keyed_pass: the plain form's single pass); the hash
// waves of a wide level issue pass p + 1 under the AES of pass p.  The plain form keeps its own uncut copy: compiled from this
// header its kernels come out with other register counts than the pinned ones (profiles/hbm_keyed_kernels_resources.txt).
// Device code only; every function is inlined.
// LDS map of both forms: 64 KiB AES table | R[64] | keys [TI][NR + 1] uint4 (at most 15 360 B).
#pragma once

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

// the words a hashed garbler lane loads: x = the operand it hashes (AND lanes 2, 3: b; OR: a), u = operand a (AND, INV) or
// b (OR) at the same columns, and the word of both operands that holds the select bit
struct GarbleColWords {
    uint32_t xw, xw1, uw, uw1, ay, by;  // uw1: OR lanes only
};
// p.kind K_NONE (an idle lane of the split form) loads as an AND lane 0 does
template <bool HAS_OR>
__device__ __forceinline__ void garble_hbm_keyed_issue(GarbleColWords &o, const ColPos &p, uint32_t in0, uint32_t in1,
                                                       uint32_t ti_log2, const uint4 *Wt) {
    const uint32_t inst = p.inst, c = p.c, wo = (c ^ 1u) << 2, wo1 = (((c + 1u) ^ 1u) << 2) & 12u;
    const bool is_or = HAS_OR && p.kind == K_OR;
    const uint4 *la = Wt + ((size_t)in0 << ti_log2) + inst;
    const uint4 *lb = p.kind != K_INV ? Wt + ((size_t)in1 << ti_log2) + inst : la;
    const uint4 *lx = (!is_or && (p.q & 2u)) ? lb : la;  // INV lanes have q < 2
    const uint4 *lu = is_or ? lb : la;
    o.uw = label_word(lu, wo), o.ay = label_word(la, 4), o.by = label_word(lb, 4);
    o.xw = label_word(lx, wo), o.xw1 = label_word(lx, wo1);
    if (is_or) o.uw1 = label_word(lb, wo1);
}

// the hash, the table words and the output column of a hashed garbler lane.  WAIT: the split form's one wait for vector
// memory, behind the hash (what it waits for is one AES old) and in front of the stores
template <int NR, bool HAS_OR, bool WAIT>
__device__ __forceinline__ void garble_hbm_keyed_finish(const Step &st, const ColPos &p, const GarbleColWords &w, uint32_t tweak,
                                                        uint32_t row_op, uint32_t ninputs, uint32_t ti_log2, uint32_t TI, uint4 *Wt,
                                                        uint4 *Tt, const uint4 *Rt, uint32_t lo) {
    const uint32_t inst = p.inst;
    uint4 *outl = Wt + ((size_t)(ninputs + st.first + p.g) << ti_log2) + inst;
    const uint32_t c = p.c, q = p.q, wo = (c ^ 1u) << 2, wo1 = (((c + 1u) ^ 1u) << 2) & 12u;
    const bool is_or = HAS_OR && p.kind == K_OR;
    const uint32_t keyaddr = kHbmKeyedKeyTab + inst * (16u * (NR + 1)) + (c << 2);
    const uint32_t a0c = w.uw, a0y = w.ay, b0y = w.by;  // (a0c: AND and INV lanes)
    const uint32_t rc = label_word(Rt + inst, wo), rc1 = label_word(Rt + inst, wo1);
    const uint32_t k0 = *(lds_u32 *)(uintptr_t)keyaddr;
    uint32_t s0;
    if (is_or) {  // e[q] = H(2x ^ 4y ^ id), x = a0 ^ (q & 2 ? R : 0), y = b0 ^ (q & 1 ? R : 0)  (garble.go:421-424)
        const uint32_t mx = (q & 2u) ? ~0u : 0u, my = (q & 1u) ? ~0u : 0u;
        const uint32_t xc = __builtin_amdgcn_bitop3_b32(w.xw, rc, mx, 0x78);
        const uint32_t xc1 = __builtin_amdgcn_bitop3_b32(w.xw1, rc1, mx, 0x78);
        const uint32_t yc = __builtin_amdgcn_bitop3_b32(w.uw, rc, my, 0x78);
        const uint32_t yc1 = __builtin_amdgcn_bitop3_b32(w.uw1, rc1, my, 0x78);
        s0 = col_whiten_k(xc, xc1, yc, yc1, c, tweak, k0);
    } else {  // AND q = 0..3 hash a0, a1, b0, b1 (lanes 2, 3: tweak + 1); INV q = 0, 1 hash a0, a1
        const uint32_t modd = (q & 1u) ? ~0u : 0u;
        const uint32_t xc = __builtin_amdgcn_bitop3_b32(w.xw, rc, modd, 0x78);
        const uint32_t xc1 = __builtin_amdgcn_bitop3_b32(w.xw1, rc1, modd, 0x78);
        s0 = col_whiten(xc, xc1, c, tweak + (q >> 1), k0);
    }
    const uint32_t h = hash_col_whitened<NR>(s0, keyaddr, lo);
    if constexpr (WAIT) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    char *row0 = (char *)(Tt + ((size_t)(row_op & kRowMask) << ti_log2) + inst) + wo;
    const uint32_t pa = (uint32_t)((int32_t)a0y >> 31), pb = (uint32_t)((int32_t)b0y >> 31);
    const uint32_t x1 = col_pair4(h);  // the hash of lane q ^ 1
    if (p.kind == K_AND) {  // garble.go:353-395, one column
        const uint32_t pp = h ^ x1;
        const uint32_t m2 = (q & 2u) ? ~0u : 0u;
        const uint32_t mk = m2 ? pb : pa, rm = pb & ~m2;
        const uint32_t wv = __builtin_amdgcn_bitop3_b32(pp, rc, rm, 0x78);
        const uint32_t tab = __builtin_amdgcn_bitop3_b32(wv, a0c, m2, 0x78);
        const uint32_t v = __builtin_amdgcn_bitop3_b32(h, wv, mk, 0x78);
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

// a free lane of either side: the garbler adds R for XNOR (garble.go:342-351, eval.go:49-51)
template <bool GARBLE>
__device__ __forceinline__ void free_hbm_keyed_lane(const Step &st, const ColPos &p, const GateDesc &d, uint32_t ninputs,
                                                    uint32_t ti_log2, uint4 *Wt, const uint4 *Rt) {
    const uint32_t inst = p.inst;
    uint4 v = lxor(Wt[((size_t)d.in0 << ti_log2) + inst], Wt[((size_t)d.in1 << ti_log2) + inst]);
    if (GARBLE && (d.row_op >> kOpShift) == GC_XNOR) v = lxor(v, Rt[inst]);
    Wt[((size_t)(ninputs + st.first + p.g) << ti_log2) + inst] = v;
}

// one lane of the garbler: garble_col_pass (fused_kernels.hip) with the instance's own key, and the OR gates
template <int NR, bool HAS_OR>
__device__ __forceinline__ void garble_hbm_keyed_pass(const Step &st, const ColPos &p, const GateDesc &d, uint32_t ninputs,
                                                      uint32_t ti_log2, uint32_t TI, uint4 *Wt, uint4 *Tt, const uint4 *Rt,
                                                      uint32_t lo) {
    if (p.kind == K_NONE) return;
    if (p.kind == K_FREE) {
        free_hbm_keyed_lane<true>(st, p, d, ninputs, ti_log2, Wt, Rt);
        return;
    }
    GarbleColWords w;
    garble_hbm_keyed_issue<HAS_OR>(w, p, d.in0, d.in1, ti_log2, Wt);
    garble_hbm_keyed_finish<NR, HAS_OR, false>(st, p, w, d.tweak, d.row_op, ninputs, ti_log2, TI, Wt, Tt, Rt, lo);
}

// the words a hashed evaluator lane loads: x = the operand it hashes (AND lane 1: b); u = the same column of operand a (AND,
// INV) or b (OR); t = the table word of an AND or INV lane, the next column of operand b of an OR lane (whose table row depends
// on both select bits: loaded in eval_hbm_keyed_finish); by = the select word of operand b (builds with OR gates).  Every
// field is loaded by every lane: a field that only some kinds define sends the set to scratch.
struct EvalColWords {
    uint32_t xc, xc1, xy, u, t, by;
};
// p.kind K_NONE (an idle lane of the split form) loads as an AND lane 0 does
template <bool HAS_OR>
__device__ __forceinline__ void eval_hbm_keyed_issue(EvalColWords &o, const ColPos &p, uint32_t in0, uint32_t in1, uint32_t row_op,
                                                     uint32_t ti_log2, uint32_t TI, const uint4 *Wt, const uint4 *Tt) {
    const uint32_t inst = p.inst, c = p.c, q = p.q, wo = (c ^ 1u) << 2, wo1 = (((c + 1u) ^ 1u) << 2) & 12u;
    const bool is_or = HAS_OR && p.kind == K_OR;
    const uint4 *la = Wt + ((size_t)in0 << ti_log2) + inst;
    const uint4 *lb = p.kind != K_INV ? Wt + ((size_t)in1 << ti_log2) + inst : la;
    const uint4 *lown = q ? lb : la;  // AND lane 1 hashes operand b (INV, OR: q = 0)
    const uint4 *row = Tt + ((size_t)(row_op & kRowMask) << ti_log2) + inst + (q ? TI : 0u);  // AND: lane q needs row q; INV: row 0
    o.xc = label_word(lown, wo), o.xc1 = label_word(lown, wo1), o.xy = label_word(lown, 4);
    o.u = label_word(is_or ? lb : la, wo);
    o.t = is_or ? label_word(lb, wo1) : label_word(row, wo);
    if constexpr (HAS_OR) o.by = label_word(lb, 4);
}

template <int NR, bool HAS_OR, bool WAIT>
__device__ __forceinline__ void eval_hbm_keyed_finish(const Step &st, const ColPos &p, const EvalColWords &w, uint32_t tweak,
                                                      uint32_t row_op, uint32_t ninputs, uint32_t ti_log2, uint4 *Wt,
                                                      const uint4 *Tt, uint32_t lo) {
    const uint32_t inst = p.inst;
    uint4 *outl = Wt + ((size_t)(ninputs + st.first + p.g) << ti_log2) + inst;
    const uint32_t c = p.c, q = p.q, wo = (c ^ 1u) << 2;
    const bool is_or = HAS_OR && p.kind == K_OR;
    const uint32_t keyaddr = kHbmKeyedKeyTab + inst * (16u * (NR + 1)) + (c << 2);
    const uint32_t xy = w.xy, ac = w.u, k0 = *(lds_u32 *)(uintptr_t)keyaddr;
    uint32_t s0, tab = 0;
    if (is_or) {  // eval.go:80-94: both operands, row index - 1 (index 0 has no row)
        const uint4 *row = Tt + ((size_t)(row_op & kRowMask) << ti_log2) + inst;
        const uint32_t index = (xy >> 31) * 2u + (w.by >> 31);
        if (index > 0) tab = label_word(row + ((size_t)(index - 1) << ti_log2), wo);
        s0 = col_whiten_k(w.xc, w.xc1, w.u, w.t, c, tweak, k0);
    } else {  // AND: lane q hashes operand q with tweak + q; INV: operand a
        tab = w.t;
        s0 = col_whiten(w.xc, w.xc1, c, tweak + q, k0);
    }
    const uint32_t h = hash_col_whitened<NR>(s0, keyaddr, lo);
    if constexpr (WAIT) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
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

// one lane of the evaluator: eval_col_pass with the instance's own key, and the OR gates (eval.go:53-109)
template <int NR, bool HAS_OR>
__device__ __forceinline__ void eval_hbm_keyed_pass(const Step &st, const ColPos &p, const GateDesc &d, uint32_t ninputs,
                                                    uint32_t ti_log2, uint32_t TI, uint4 *Wt, const uint4 *Tt, uint32_t lo) {
    if (p.kind == K_NONE) return;
    if (p.kind == K_FREE) {
        free_hbm_keyed_lane<false>(st, p, d, ninputs, ti_log2, Wt, nullptr);
        return;
    }
    EvalColWords w;
    eval_hbm_keyed_issue<HAS_OR>(w, p, d.in0, d.in1, d.row_op, ti_log2, TI, Wt, Tt);
    eval_hbm_keyed_finish<NR, HAS_OR, false>(st, p, w, d.tweak, d.row_op, ninputs, ti_log2, Wt, Tt, lo);
}

}  // namespace

}  // namespace gc
