// flat_lanes.h — lane-level pieces of the flattened fused kernels that fused_flat_kernels.hip (one key per batch, round
// keys in SGPRs) and fused_flat_keyed_kernels.hip (one key per instance, round keys in LDS) share: DPP and LDS label
// helpers, the unit header, the hash-lane map and the XOR part, every device function inlined; and the host's fill of their
// kernel argument.
#pragma once

#include "aes_device.h"
#include "kernels.h"

namespace gc {

namespace {

constexpr int TF = 1024;

constexpr int DPP_XOR1 = 0xB1;   // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;   // [2,3,0,1]
constexpr int DPP_XOR3 = 0x1B;   // [3,2,1,0]
constexpr int DPP_BC0 = 0x00;    // [0,0,0,0]
constexpr int DPP_BC2 = 0xAA;    // [2,2,2,2]
constexpr int DPP_PAIR0 = 0xA0;  // [0,0,2,2]

template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
    // quad permutes have no invalid source lanes inside a full quad: no "old" value, so no register initialisation
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ uint4 dpp128(uint4 v) {
    return make_uint4(dpp32<CTRL>(v.x), dpp32<CTRL>(v.y), dpp32<CTRL>(v.z), dpp32<CTRL>(v.w));
}

// v ^ (v of the quad partner): computed by every lane of the quad so that it is four v_xor_b32_dpp; the opaque asm
// keeps the compiler from sinking the XOR into the q == 0 branch that uses it (DPP cannot read from lanes that are
// switched off, so there it becomes 4 DPP moves + 4 XORs)
template <int CTRL>
__device__ __forceinline__ uint4 quad_xor(uint4 v) {
    uint4 o = make_uint4(v.x ^ dpp32<CTRL>(v.x), v.y ^ dpp32<CTRL>(v.y), v.z ^ dpp32<CTRL>(v.z), v.w ^ dpp32<CTRL>(v.w));
    asm volatile("" : "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(o.w));
    return o;
}

typedef uint32_t lds_v4 __attribute__((ext_vector_type(4)));
using lds_v4p = __attribute__((address_space(3))) const lds_v4 *;
using lds_v4w = __attribute__((address_space(3))) lds_v4 *;

// Wire labels in LDS by byte address: label of slot s, instance inst = ib + (s << sh) with ib = wl + 16 inst and
// sh = ti_log2 + 4: one v_lshl_add_u32 per access (the indexed form costs two shifts and a three-input add)
__device__ __forceinline__ uint4 lds_label(uint32_t ib, uint32_t slot, uint32_t sh) {
    const lds_v4 v = *(lds_v4p)(uintptr_t)((slot << sh) + ib);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void lds_label_put(uint32_t ib, uint32_t slot, uint32_t sh, uint4 v) {
    lds_v4 o;
    o.x = v.x, o.y = v.y, o.z = v.z, o.w = v.w;
    *(lds_v4w)(uintptr_t)((slot << sh) + ib) = o;
}
// low (hi = false) or high half-word of a packed slot pair, chosen per lane: one v_perm_b32
__device__ __forceinline__ uint32_t half_of(uint32_t packed, bool hi) {
    return __builtin_amdgcn_perm(packed, packed, hi ? 0x0c0c0302u : 0x0c0c0100u);
}

// h ^ (w & m) per bit: one v_bitop3_b32 per word
__device__ __forceinline__ uint4 xand4(uint4 h, uint4 w, uint32_t m) {
    return make_uint4(__builtin_amdgcn_bitop3_b32(h.x, w.x, m, 0x78), __builtin_amdgcn_bitop3_b32(h.y, w.y, m, 0x78),
                      __builtin_amdgcn_bitop3_b32(h.z, w.z, m, 0x78), __builtin_amdgcn_bitop3_b32(h.w, w.w, m, 0x78));
}

__device__ __forceinline__ uint4 lxor3(uint4 a, uint4 b, uint4 c) {
    return make_uint4(xor3(a.x, b.x, c.x), xor3(a.y, b.y, c.y), xor3(a.z, b.z, c.z), xor3(a.w, b.w, c.w));
}

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

using FlArgs = FlatJob;  // kernels.h

// host: the kernel argument of a batch launch, every workgroup one tile of the same circuit
inline FlArgs flat_job(bool eval, const FusedFlatArgs &f, const BatchGeom &g) {
    FlArgs a{};
    a.prog = (const uint4 *)f.prog;
    a.units = f.units;
    a.hgslot = f.hgslot;
    a.ogslot = f.ogslot;
    a.in_lds = f.in_lds;
    a.nunits = f.nunits;
    a.ninputs = f.ninputs;
    a.ti_log2 = g.ti_log2;
    a.zslot = f.nls - 1;
    a.ustride = f.ustride;
    a.w_tile = g.lw.tile_stride;
    a.t_tile = g.lt.tile_stride;
    a.W = f.W;
    a.R = f.R;
    a.T = f.T;
    a.rk = f.rk;
    a.te0 = f.te0;
    a.prof = f.prof;
    a.rnd = eval ? nullptr : f.rnd;
    a.Rout = const_cast<uint4 *>(f.R);
    a.batch = g.batch;
    return a;
}

// Unit header i.  Loaded with VECTOR loads on purpose (vz is a zero the compiler cannot see through): scalar loads
// share the lgkm counter with LDS and return out of order, so with a header in flight the first LDS read of the
// next unit would have to wait for it (s_waitcnt lgkmcnt(0)); vector loads are tracked by vmcnt and cost nothing
// until their values are used one unit later.
// The unit array ends with two all-zero records and the program with one stage buffer of padding (engine.cpp), so
// headers and images two units past the end can be fetched without bounds checks (they describe empty units).
__device__ __forceinline__ FUnit load_unit(const FUnit *units, uint32_t i, uint32_t vz) {
    FUnit u;
    const uint4 *p = (const uint4 *)(units + i) + vz;
    const uint4 a = p[0], b = p[1], c = p[2];
    u.off16 = a.x, u.n16 = a.y, u.n_and = a.z, u.n_or = a.w;
    u.n_inv = b.x, u.nout = b.y, u.outs_off16 = b.z, u.xparts = b.w;
    u.hfirst = c.x, u.ofirst = c.y;
    u.pad_[0] = u.pad_[1] = 0;
    return u;
}
// wave-uniform copy in SGPRs (readfirstlane) of a header whose loads have landed
__device__ __forceinline__ FUnit uniform_unit(const FUnit &v) {
    FUnit u{};
    u.off16 = __builtin_amdgcn_readfirstlane(v.off16);
    u.n16 = __builtin_amdgcn_readfirstlane(v.n16);
    u.n_and = __builtin_amdgcn_readfirstlane(v.n_and);
    u.n_or = __builtin_amdgcn_readfirstlane(v.n_or);
    u.n_inv = __builtin_amdgcn_readfirstlane(v.n_inv);
    u.nout = __builtin_amdgcn_readfirstlane(v.nout);
    u.outs_off16 = __builtin_amdgcn_readfirstlane(v.outs_off16);
    u.hfirst = __builtin_amdgcn_readfirstlane(v.hfirst);
    u.ofirst = __builtin_amdgcn_readfirstlane(v.ofirst);
    u.xparts = __builtin_amdgcn_readfirstlane(v.xparts);
    return u;
}

// hash-part lane -> (kind, gate, instance, sub-lane); kinds: 0 none, 1 AND, 2 OR, 3 INV
struct HP {
    uint32_t kind, g, inst, q;
};
template <int LQA, int LQO, int LQI, bool HAS_OR = true>
__device__ __forceinline__ HP hpos(uint32_t t, const FUnit &c, uint32_t ti_log2, uint32_t tim) {
    HP p{0, 0, 0, 0};
    if constexpr (!HAS_OR) {  // AND lanes, then INV lanes: branch-free (selects instead of exec-mask regions)
        const uint32_t e_and = (c.n_and << ti_log2) << LQA;
        const uint32_t e_all = e_and + ((c.n_inv << ti_log2) << LQI);
        const bool is_and = t < e_and;
        const uint32_t u = is_and ? t : t - e_and;
        const uint32_t lq = is_and ? (uint32_t)LQA : (uint32_t)LQI;
        p.kind = is_and ? 1u : t < e_all ? 3u : 0u;
        p.g = (u >> (ti_log2 + lq)) + (is_and ? 0u : c.n_and);
        p.inst = (u >> lq) & tim;
        p.q = u & ((1u << lq) - 1);
        return p;
    }
    const uint32_t e_and = (c.n_and << ti_log2) << LQA;
    const uint32_t e_or = HAS_OR ? e_and + ((c.n_or << ti_log2) << LQO) : e_and;
    const uint32_t e_all = e_or + ((c.n_inv << ti_log2) << LQI);
    if (t < e_and) {
        p.kind = 1;
        p.g = t >> (ti_log2 + LQA);
        p.inst = (t >> LQA) & tim;
        p.q = t & ((1u << LQA) - 1);
    } else if (HAS_OR && t < e_or) {
        const uint32_t u = t - e_and;
        p.kind = 2;
        p.g = c.n_and + (u >> (ti_log2 + LQO));
        p.inst = (u >> LQO) & tim;
        p.q = u & ((1u << LQO) - 1);
    } else if (t < e_all) {
        const uint32_t u = t - e_or;
        p.kind = 3;
        p.g = c.n_and + c.n_or + (u >> (ti_log2 + LQI));
        p.inst = (u >> LQI) & tim;
        p.q = u & ((1u << LQI) - 1);
    }
    return p;
}
template <int LQA, int LQO, int LQI>
__device__ __forceinline__ uint32_t hlanes(const FUnit &c, uint32_t ti_log2) {
    return ((c.n_and << ti_log2) << LQA) + ((c.n_or << ti_log2) << LQO) + ((c.n_inv << ti_log2) << LQI);
}

// value of the lane SH further on inside its row of 16 lanes (DPP row_shl: register to register, no LDS)
template <int SH>
__device__ __forceinline__ uint4 row_down(uint4 v) {
    return make_uint4((uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.x, 0x100 + SH, 0xf, 0xf, true),
                      (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.y, 0x100 + SH, 0xf, 0xf, true),
                      (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.z, 0x100 + SH, 0xf, 0xf, true),
                      (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.w, 0x100 + SH, 0xf, 0xf, true));
}
__device__ __forceinline__ uint4 sel4(bool c, uint4 a, uint4 b) {
    return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}
// leader of a list spread over 2 / 4 lanes TI apart (all inside one row: parts * TI <= 16, plan.h / geom_for): its own
// partial sum plus those of the following parts; every other lane keeps its value
template <int TIV>
__device__ __forceinline__ uint4 join_parts(uint4 acc, uint32_t flags, bool four) {
    const uint4 a1 = lxor(acc, row_down<TIV>(acc));
    uint4 r = sel4((flags & (kXoJoin2 | kXoJoin4)) != 0, a1, acc);
    if constexpr (2 * TIV < 16) {
        if (four) {
            const uint4 a2 = lxor(a1, row_down<2 * TIV>(a1));
            r = sel4((flags & kXoJoin4) != 0, a2, r);
        }
    }
    return r;
}

// XOR part: one lane per (XOut, instance): the label is the XOR of up to 8 terms whose LDS slots sit in the XOut
// itself (one LDS round trip for the item, one for its labels); lists of more than 8 terms come as 2 / 4 parts.
// garble.go:331-351 / eval.go:49-51 restated over the expanded terms.
template <bool GARBLE>
__device__ __forceinline__ void xor_part(const uint4 *buf, const FUnit &u, const uint32_t *ogslot, uint4 *wl,
                                         const uint4 *rl, uint4 *Wt, uint32_t ti_log2, uint32_t tim) {
    const uint2 *outs = (const uint2 *)(buf + u.outs_off16);  // 3 x 8 bytes per XOut
    const uint32_t nitems = u.nout << ti_log2;
    for (uint32_t t = threadIdx.x; t < nitems; t += TF) {
        const uint32_t o = t >> ti_log2, inst = t & tim;
        const uint2 d0 = outs[3 * o], d2 = outs[3 * o + 2];
        uint2 d1 = outs[3 * o + 1];
        // keep the read of the second half of the item with the other two (one LDS round trip for the whole item);
        // the compiler would otherwise sink it into the n > 4 branch: a third dependent round trip for long lists
        asm volatile("" : "+v"(d1.x), "+v"(d1.y));
        const uint32_t flags = d2.x >> 16, n = d2.y & 0xffffu;
        // byte addressing by hand: label of slot s, instance inst = wl + (s << (ti_log2 + 4)) + 16 inst — one shift of
        // the extracted half-word and one add per term
        const uint32_t sh = ti_log2 + 4, ib = (uint32_t)(uintptr_t)wl + (inst << 4);
        auto lab = [&](uint32_t packed, bool high) {
            const uint32_t s16 = high ? packed >> 16 : packed & 0xffffu;
            const lds_v4 v = *(lds_v4p)(uintptr_t)((s16 << sh) + ib);
            return make_uint4(v.x, v.y, v.z, v.w);
        };
        // Items are sorted by length and padded with the zero slot: a wave that holds a list of more than four terms
        // reads all eight labels in ONE batch (a wave-uniform branch; the short lists of that wave read zeros), the
        // other waves read four.  Three-input XORs (v_bitop3): 2 / 4 per word.
        uint4 acc;
        if (__ballot(n > 4) != 0) {
            const uint4 v0 = lab(d0.x, false), v1 = lab(d0.x, true), v2 = lab(d0.y, false), v3 = lab(d0.y, true);
            const uint4 v4 = lab(d1.x, false), v5 = lab(d1.x, true), v6 = lab(d1.y, false), v7 = lab(d1.y, true);
            acc = lxor(lxor3(lxor3(v0, v1, v2), v3, v4), lxor3(v5, v6, v7));
        } else {
            const uint4 v0 = lab(d0.x, false), v1 = lab(d0.x, true), v2 = lab(d0.y, false), v3 = lab(d0.y, true);
            acc = lxor(lxor3(v0, v1, v2), v3);
        }
        // collect the partial sums of lists that were spread over 2 / 4 lanes: only in units that have such lists, and
        // there only in the waves that hold them (they come first in the length order) - a wave-uniform test
        if (u.xparts > 1 && __ballot((flags & (kXoJoin2 | kXoJoin4 | kXoPart)) != 0) != 0) {
            const bool four = u.xparts > 2;
            if (ti_log2 == 0) acc = join_parts<1>(acc, flags, four);
            else if (ti_log2 == 1) acc = join_parts<2>(acc, flags, four);
            else if (ti_log2 == 2) acc = join_parts<4>(acc, flags, four);
            else acc = join_parts<8>(acc, flags, false);
        }
        if (flags & kXoPart) continue;
        if (GARBLE && (flags & kXoRpar)) acc = lxor(acc, rl[inst]);
        lds_label_put(ib, d2.x & 0xffffu, sh, acc);
        if (flags & kXoStore) Wt[((size_t)ogslot[u.ofirst + o] << ti_log2) + inst] = acc;
    }
}

// Every hash lane of the wide form becomes a quad (lane = 4 * wide lane + column): a lone wave's 14 AES rounds take
// ~3.3 k cycles, the four quarter-waves of the column form ~2.2 k, and in such units that latency is the phase.  Same
// arithmetic as the wide form, one 32-bit column per lane: label word W_c (big-endian column c) sits at dword c ^ 1.
// Partner lanes of a gate are 4 (q ^ 1) and 8 (q ^ 2) lanes away: DPP row shifts / rotations inside the row of 16.
__device__ __forceinline__ uint32_t lds_word(uint32_t addr) { return *(lds_u32 *)(uintptr_t)addr; }
__device__ __forceinline__ void lds_word_put(uint32_t addr, uint32_t v) {
    *(__attribute__((address_space(3))) uint32_t *)(uintptr_t)addr = v;
}
// value of the lane 4 further on (q even) / 4 back (q odd): the q ^ 1 partner
__device__ __forceinline__ uint32_t pair4(uint32_t v) {
    uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0x5, false);   // row_shl:4 -> banks 0, 2
    return (uint32_t)__builtin_amdgcn_update_dpp((int)r, (int)v, 0x114, 0xf, 0xa, false);     // row_shr:4 -> banks 1, 3
}
// column c of K ^ rk_0 with K = 2x ^ tweak: (x_c << 1) | (x_c+1 >> 31), the tweak in column 3
__device__ __forceinline__ uint32_t whiten_col(uint32_t xc, uint32_t xc1, uint32_t c, uint32_t tweak, uint32_t k0) {
    const uint32_t kcol = __builtin_amdgcn_alignbit(xc, c == 3 ? 0u : xc1, 31);
    return xor3(kcol, c == 3 ? tweak : 0u, k0);
}

}  // namespace

}  // namespace gc
