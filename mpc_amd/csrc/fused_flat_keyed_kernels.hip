// fused_flat_keyed_kernels.hip — the flattened batch kernels with ONE AES KEY PER INSTANCE (gc_batch_garble_keyed /
// gc_batch_eval_keyed): circuit.Garbler draws a fresh key for every session (garbler.go:47-53), so a batch that gathers S
// sessions holds S keys.
//
// Same plan, unit images, wire slots and table layout as k_garble_flat / k_eval_flat (fused_flat_kernels.hip); what differs:
//   * k_expand_keys turns u8 [batch][keylen] into round-key words [batch][4 (NR + 1)] (the word order of FlatJob::rk, the
//     last round key folded with round key 0: the hashes run on whitened blocks);
//   * the prologue copies the tile's TI schedules into an LDS key table BEHIND the wire slots (the planner's geometry is
//     untouched; the engine launches only when the table fits) — no round key sits in an SGPR: a wave's lanes span the
//     tile's instances;
//   * every hashed item runs column-sliced (hash_col_whitened: four lanes per block, round keys from LDS) with
//     keyaddr = key table + inst * 16 (NR + 1) + 4 c, in passes of 1024 column lanes; OR gates take the same form.
// LDS map: 64 KiB AES table | 256 B unused (the one-key kernels' column keys) | 2 x ustride stage | R[TI] | wires
// [slot][TI] | keys [TI][NR + 1] uint4.
#include "aes_device.h"
#include "aes_schedule.h"
#include "flat_lanes.h"

namespace gc {

namespace {

constexpr int kExpandThreads = 256;  // k_expand_keys: one lane = one instance

// AES key schedule (FIPS-197 5.2) of one instance per lane; S-box = byte 1 of Te0, kept in LDS
template <int NR>
__global__ __launch_bounds__(kExpandThreads) void k_expand_keys(const uint8_t *__restrict__ keys, uint32_t batch,
                                                                const uint32_t *__restrict__ g_te0,
                                                                uint32_t *__restrict__ out) {
    constexpr int NK = NR - 6, NW = 4 * (NR + 1);
    __shared__ uint8_t sbox[256];
    load_sbox(sbox, g_te0);
    __syncthreads();
    const uint32_t gi = blockIdx.x * kExpandThreads + threadIdx.x;
    if (gi >= batch) return;
    uint32_t w[NW];
    aes_key_schedule<NR>(keys + (size_t)gi * (4 * NK), sbox, w);
    uint32_t *o = out + (size_t)gi * NW;
#pragma unroll
    for (int i = 0; i < NW; i++) o[i] = i >= 4 * NR ? w[i] ^ w[i - 4 * NR] : w[i];
}

// column c of K ^ rk_0 with K = 2x ^ 4y ^ tweak (makeK, garble.go:74-83), the tweak in column 3
__device__ __forceinline__ uint32_t whiten_col_k(uint32_t xc, uint32_t xc1, uint32_t yc, uint32_t yc1, uint32_t c,
                                                 uint32_t tweak, uint32_t k0) {
    const uint32_t kx = __builtin_amdgcn_alignbit(xc, c == 3 ? 0u : xc1, 31);
    const uint32_t ky = __builtin_amdgcn_alignbit(yc, c == 3 ? 0u : yc1, 30);
    return xor3(kx, ky, k0) ^ (c == 3 ? tweak : 0u);
}
// value of the lane 8 further on / back inside the row of 16: the q ^ 2 partner of a garbler lane
__device__ __forceinline__ uint32_t pair8(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, true); }

// Hash part of the garbler, column-sliced for the whole unit: column lane j = 4 * (hash lane of the wide form) + column,
// in passes of TF lanes.  A gate-instance is a whole row of 16 lanes (AND, OR: q = 0..3) or half a row (INV: q = 0, 1)
// and a pass holds whole rows, so the DPP partners of a lane are always in its pass.  keytab: byte address of the tile's
// key table.  garble.go:353-474, one column per lane.
template <int NR, bool HAS_OR>
__device__ __forceinline__ void garble_hash_keyed(const uint4 *buf, const FUnit &u, const FlArgs &a, uint32_t ti_log2,
                                                  uint32_t tim, uint4 *wl, const uint4 *rl, uint4 *Tt, uint4 *Wt,
                                                  uint32_t keytab, uint32_t lo, uint32_t wave_base) {
    const uint32_t TI = 1u << ti_log2;
    const uint32_t ncol = hlanes<2, 2, 1>(u, ti_log2) << 2;
    for (uint32_t j0 = 0; j0 + wave_base < ncol; j0 += TF) {  // scalar test: a wave without lanes leaves at once
        const uint32_t j = j0 + threadIdx.x;
        const HP hp = hpos<2, 2, 1, HAS_OR>(j >> 2, u, ti_log2, tim);
        if (hp.kind == 0) continue;
        const uint32_t c = j & 3u, q = hp.q, inst = hp.inst, wo = (c ^ 1u) << 2, wo1 = (((c + 1u) ^ 1u) << 2) & 12u;
        const uint4 dv = buf[hp.g];
        const FDesc d{dv.x, dv.y, dv.z, dv.w};
        const uint32_t sh = ti_log2 + 4, ib = (uint32_t)(uintptr_t)wl + (inst << 4);
        const uint32_t ra = (uint32_t)(uintptr_t)rl + (inst << 4);
        const bool is_or = HAS_OR && hp.kind == 2;
        // the two operands' labels (an INV has one: its second slot field is not a slot)
        const uint32_t sa = ((d.lin & 0xffffu) << sh) + ib, sb = hp.kind != 3 ? ((d.lin >> 16) << sh) + ib : sa;
        const uint32_t keyaddr = keytab + inst * (16u * (NR + 1)) + (c << 2);
        const uint32_t rc = lds_word(ra + wo), rc1 = lds_word(ra + wo1);
        const uint32_t a0c = lds_word(sa + wo), a0y = lds_word(sa + 4), b0y = lds_word(sb + 4);
        const uint32_t k0 = lds_word(keyaddr);
        uint32_t s0;
        if (is_or) {  // e[q] = H(2x ^ 4y ^ id), x = a0 ^ (q & 2 ? R : 0), y = b0 ^ (q & 1 ? R : 0)  (garble.go:421-424)
            const uint32_t mx = (q & 2u) ? ~0u : 0u, my = (q & 1u) ? ~0u : 0u;
            const uint32_t xc = __builtin_amdgcn_bitop3_b32(a0c, rc, mx, 0x78);
            const uint32_t xc1 = __builtin_amdgcn_bitop3_b32(lds_word(sa + wo1), rc1, mx, 0x78);
            const uint32_t yc = __builtin_amdgcn_bitop3_b32(lds_word(sb + wo), rc, my, 0x78);
            const uint32_t yc1 = __builtin_amdgcn_bitop3_b32(lds_word(sb + wo1), rc1, my, 0x78);
            s0 = whiten_col_k(xc, xc1, yc, yc1, c, d.tweak, k0);
        } else {  // AND q = 0..3 hash a0, a1, b0, b1 (lanes 2, 3: tweak + 1); INV q = 0, 1 hash a0, a1
            const uint32_t so = (q & 2u) ? sb : sa;  // INV lanes have q < 2
            const uint32_t modd = (q & 1u) ? ~0u : 0u;
            const uint32_t xc = __builtin_amdgcn_bitop3_b32(lds_word(so + wo), rc, modd, 0x78);
            const uint32_t xc1 = __builtin_amdgcn_bitop3_b32(lds_word(so + wo1), rc1, modd, 0x78);
            s0 = whiten_col(xc, xc1, c, d.tweak + (q >> 1), k0);
        }
        const uint32_t h = hash_col_whitened<NR>(s0, keyaddr, lo);
        const uint32_t rowb = ((((d.row_op & kRowMask) << ti_log2) + inst) << 4) + wo;
        auto row = [&](uint32_t r) -> uint32_t & { return *(uint32_t *)((char *)Tt + (rowb + (r << 4))); };
        auto put = [&](uint32_t v) {
            if (q == 0) {
                lds_word_put(((d.lout & 0xffffu) << sh) + ib + wo, v);
                if (d.lout & kFStoreGlobal)
                    *(uint32_t *)((char *)(Wt + ((size_t)a.hgslot[u.hfirst + hp.g] << ti_log2) + inst) + wo) = v;
            }
        };
        const uint32_t pa = (uint32_t)((int32_t)a0y >> 31), pb = (uint32_t)((int32_t)b0y >> 31);
        const uint32_t x1 = pair4(h);  // the hash of lane q ^ 1
        if (hp.kind == 1) {  // garble.go:353-395
            const uint32_t p = h ^ x1;
            const uint32_t m2 = (q & 2u) ? ~0u : 0u;
            const uint32_t mk = m2 ? pb : pa, rm = pb & ~m2;
            const uint32_t w = __builtin_amdgcn_bitop3_b32(p, rc, rm, 0x78);
            const uint32_t tab = __builtin_amdgcn_bitop3_b32(w, a0c, m2, 0x78);
            const uint32_t v = __builtin_amdgcn_bitop3_b32(h, w, mk, 0x78);
            if (!(q & 1u)) row((q & 2u) ? TI : 0) = tab;
            uint32_t o = v ^ pair8(v);
            asm volatile("" : "+v"(o));
            put(o);
        } else if (!is_or) {  // INV, garble.go:446-474
            const uint32_t p = h ^ x1;
            if (q == 0) row(0) = p ^ rc;
            put(h ^ (((int32_t)a0y < 0) ? p : rc));
        } else {  // OR, garble.go:412-444: table[q] = e[q ^ l0] ^ (q == l0 ? c0 : c1), l0 = 2 S(a0) + S(b0)
            const uint32_t x2 = pair8(h), x3 = pair4(x2);  // the hashes of lanes q ^ 2, q ^ 3
            const uint32_t l0 = (pa & 2u) | (pb & 1u);
            auto pick = [&](uint32_t dist) { return dist == 0 ? h : dist == 1 ? x1 : dist == 2 ? x2 : x3; };
            const uint32_t tk = pick(l0), t0v = pick(q ^ l0);  // e[q ^ l0], e[l0]
            const uint32_t c0 = t0v ^ (l0 ? rc : 0u), c1 = t0v ^ (l0 ? 0u : rc);
            if (q != 0) row((q - 1) << ti_log2) = tk ^ (q == l0 ? c0 : c1);
            put(c0);
        }
    }
}

// Hash part of the evaluator in the same form: AND = two blocks (operand a / b, 8 lanes), INV and OR one (4 lanes).
// eval.go:53-109, one column per lane.
template <int NR, bool HAS_OR>
__device__ __forceinline__ void eval_hash_keyed(const uint4 *buf, const FUnit &u, const FlArgs &a, uint32_t ti_log2,
                                                uint32_t tim, uint4 *wl, const uint4 *Tt, uint4 *Wt, uint32_t keytab,
                                                uint32_t lo, uint32_t wave_base) {
    const uint32_t TI = 1u << ti_log2;
    const uint32_t ncol = hlanes<1, 0, 0>(u, ti_log2) << 2;
    for (uint32_t j0 = 0; j0 + wave_base < ncol; j0 += TF) {
        const uint32_t j = j0 + threadIdx.x;
        const HP hp = hpos<1, 0, 0, HAS_OR>(j >> 2, u, ti_log2, tim);
        if (hp.kind == 0) continue;
        const uint32_t c = j & 3u, q = hp.q, inst = hp.inst, wo = (c ^ 1u) << 2, wo1 = (((c + 1u) ^ 1u) << 2) & 12u;
        const uint4 dv = buf[hp.g];
        const FDesc d{dv.x, dv.y, dv.z, dv.w};
        const uint32_t sh = ti_log2 + 4, ib = (uint32_t)(uintptr_t)wl + (inst << 4);
        const bool is_or = HAS_OR && hp.kind == 2;
        const uint32_t sa = ((d.lin & 0xffffu) << sh) + ib, sb = hp.kind != 3 ? ((d.lin >> 16) << sh) + ib : sa;
        const uint32_t so = q ? sb : sa;  // AND lane 1 hashes operand b (INV, OR: q = 0)
        const uint32_t keyaddr = keytab + inst * (16u * (NR + 1)) + (c << 2);
        const uint32_t rowb = ((((d.row_op & kRowMask) << ti_log2) + inst) << 4) + wo;
        const uint32_t xc = lds_word(so + wo), xc1 = lds_word(so + wo1), xy = lds_word(so + 4);
        const uint32_t ac = lds_word(sa + wo), k0 = lds_word(keyaddr);
        auto put = [&](uint32_t v) {
            if (q == 0) {
                lds_word_put(((d.lout & 0xffffu) << sh) + ib + wo, v);
                if (d.lout & kFStoreGlobal)
                    *(uint32_t *)((char *)(Wt + ((size_t)a.hgslot[u.hfirst + hp.g] << ti_log2) + inst) + wo) = v;
            }
        };
        uint32_t s0, tab = 0;
        if (is_or) {  // eval.go:80-94: both operands, row index - 1 (index 0 has no row)
            const uint32_t index = (xy >> 31) * 2u + (lds_word(sb + 4) >> 31);
            if (index > 0) tab = *(const uint32_t *)((const char *)Tt + (rowb + (((index - 1) << ti_log2) << 4)));
            s0 = whiten_col_k(xc, xc1, lds_word(sb + wo), lds_word(sb + wo1), c, d.tweak, k0);
        } else {  // AND: lane q hashes operand q with tweak + q and needs table row q; INV: operand a, row 0
            tab = *(const uint32_t *)((const char *)Tt + (rowb + ((q ? TI : 0u) << 4)));  // lands during the AES
            s0 = whiten_col(xc, xc1, c, d.tweak + q, k0);
        }
        const uint32_t h = hash_col_whitened<NR>(s0, keyaddr, lo);
        const uint32_t sm = (uint32_t)((int32_t)xy >> 31);
        if (hp.kind == 1) {  // eval.go:53-78: lane 0 WG = H(a) ^ (sa ? TG : 0), lane 1 WE = H(b) ^ (sb ? TE ^ a : 0)
            const uint32_t v = __builtin_amdgcn_bitop3_b32(h, __builtin_amdgcn_bitop3_b32(tab, ac, q ? ~0u : 0u, 0x78), sm, 0x78);
            uint32_t o = v ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x104, 0xf, 0xf, true);  // + the lane 4 further on (q = 1)
            asm volatile("" : "+v"(o));
            put(o);
        } else if (!is_or) {  // eval.go:96-109
            put(__builtin_amdgcn_bitop3_b32(h, tab, sm, 0x78));
        } else {  // (tab is zero for index 0)
            put(h ^ tab);
        }
    }
}

// One pass over the unit program for a tile; a.rk = the expanded keys of the whole batch (k_expand_keys)
template <int NR, bool HAS_OR, bool GARBLE>
__device__ __forceinline__ void flat_keyed_body(const FlArgs &a) {
    constexpr uint32_t kWords = 4 * (NR + 1);
    const uint32_t tile = blockIdx.x;
    extern __shared__ uint4 smem[];
    uint32_t *te = (uint32_t *)smem;
    const uint32_t ti_log2 = a.ti_log2, TI = 1u << ti_log2, tim = TI - 1;
    uint4 *stage = smem + kFlatStageOff16;
    const uint32_t ustride = a.ustride;
    uint4 *rl = stage + 2 * ustride;
    uint4 *wl = rl + TI;
    uint32_t *keys = (uint32_t *)(wl + ((a.zslot + 1) << ti_log2));  // behind the wire slots
    load_te_dual(te, a.te0);
    uint32_t vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    // the tile's schedules; instances past the batch (the last tile) get zero keys and are not read
    for (uint32_t i = threadIdx.x; i < (kWords << ti_log2); i += TF)
        keys[i] = tile * TI + i / kWords < a.batch ? a.rk[(size_t)tile * TI * kWords + i] : 0u;
    uint4 *Wt = a.W + (size_t)tile * a.w_tile;
    uint4 *Tt = a.T + (size_t)tile * a.t_tile;
    if (threadIdx.x < TI) wl[(a.zslot << ti_log2) + threadIdx.x] = make_uint4(0, 0, 0, 0);
    if (GARBLE) {
        // R and the input zero-labels of the tile straight from the caller's random stream ([instance][1 + ninputs]
        // big-endian labels; garble.go:253-258, 271-278)
        for (uint32_t i = threadIdx.x; i < ((a.ninputs + 1) << ti_log2); i += TF) {
            const uint32_t j = i >> ti_log2, inst = i & tim, gi = tile * TI + inst;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (gi < a.batch) {
                const uint4 raw = a.rnd[(size_t)gi * (a.ninputs + 1) + j];
                v = make_uint4(__builtin_bswap32(raw.y), __builtin_bswap32(raw.x), __builtin_bswap32(raw.w),
                               __builtin_bswap32(raw.z));
            }
            if (j == 0) {
                v.y |= 0x80000000u;  // R.SetS(true)
                rl[inst] = v;
                a.Rout[(size_t)tile * TI + inst] = v;
            } else {
                const uint32_t ls = a.in_lds[j - 1];
                Wt[((j - 1) << ti_log2) + inst] = v;
                if (ls != 0xffffu) wl[(ls << ti_log2) + inst] = v;
            }
        }
    } else {
        for (uint32_t i = threadIdx.x; i < (a.ninputs << ti_log2); i += TF) {
            const uint32_t ls = a.in_lds[i >> ti_log2];
            if (ls != 0xffffu) wl[(ls << ti_log2) + (i & tim)] = Wt[i];
        }
    }
    // unit headers and images run ahead exactly as in the one-key kernels (fused_flat_kernels.hip)
    FUnit u = uniform_unit(load_unit(a.units, 0, vz));
    FUnit un = load_unit(a.units, 1, vz);
    if (threadIdx.x < u.n16) stage[threadIdx.x] = a.prog[u.off16 + threadIdx.x];
    uint4 pre_cur = a.prog[un.off16 + threadIdx.x];
    __syncthreads();
    const uint32_t lo = te_lane_off();
    const uint32_t wave_base = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    const uint32_t keytab = (uint32_t)(uintptr_t)keys;
    for (uint32_t ui = 0; ui < a.nunits; ui++) {
        const uint4 *buf = stage + (ui & 1u) * ustride;
        const uint32_t nh = u.n_and + u.n_or + u.n_inv;
        if (nh) {
            if constexpr (GARBLE) garble_hash_keyed<NR, HAS_OR>(buf, u, a, ti_log2, tim, wl, rl, Tt, Wt, keytab, lo, wave_base);
            else eval_hash_keyed<NR, HAS_OR>(buf, u, a, ti_log2, tim, wl, Tt, Wt, keytab, lo, wave_base);
        }
        const FUnit unn_v = load_unit(a.units, ui + 2, vz);
        const uint4 pre_next = a.prog[un.off16 + un.n16 + threadIdx.x];
        if (nh && u.nout) lds_barrier();
        if (u.nout) xor_part<GARBLE>(buf, u, a.ogslot, wl, rl, Wt, ti_log2, tim);
        if (threadIdx.x < un.n16) stage[((ui + 1) & 1u) * ustride + threadIdx.x] = pre_cur;
        lds_barrier();
        u = uniform_unit(un);
        un = unn_v;
        pre_cur = pre_next;
    }
}

}  // namespace

template <int NR, bool HAS_OR>
__global__ __launch_bounds__(TF) void k_garble_flat_keyed(FlArgs a) {
    flat_keyed_body<NR, HAS_OR, true>(a);
}
template <int NR, bool HAS_OR>
__global__ __launch_bounds__(TF) void k_eval_flat_keyed(FlArgs a) {
    flat_keyed_body<NR, HAS_OR, false>(a);
}

size_t fused_flat_keyed_bytes(uint32_t nls, uint32_t ti_log2, uint32_t ustride, int rounds) {
    return fused_flat_bytes(nls, ti_log2, ustride) + ((size_t)16 * (rounds + 1) << ti_log2);
}

hipError_t launch_expand_keys(const uint8_t *d_keys, int rounds, uint32_t batch, const uint32_t *te0, uint32_t *d_out,
                              hipStream_t s) {
    const dim3 grid((batch + kExpandThreads - 1) / kExpandThreads), block(kExpandThreads);
    return with_rounds(rounds, [&](auto nr) {
        return launch_kernel(k_expand_keys<decltype(nr)::value>, grid, block, s, d_keys, batch, te0, d_out);
    });
}

// (a.prof is carried along and ignored)
hipError_t launch_fused_flat_keyed(bool eval, const FusedFlatArgs &f, const BatchGeom &g, hipStream_t s) {
    const FlArgs a = flat_job(eval, f, g);
    if (a.nunits == 0) return hipSuccess;
    if (!eval && !f.rnd) return hipErrorInvalidValue;
    const size_t lds = fused_flat_keyed_bytes(f.nls, g.ti_log2, f.ustride, f.rounds);
    if (lds > kFlatLdsBytes) return hipErrorInvalidConfiguration;
    const dim3 grid(g.ntiles), block(TF);
    return with_rounds(f.rounds, [&](auto nr) {
        return with_flag(f.has_or, [&](auto has_or) {
            constexpr int NR = decltype(nr)::value;
            constexpr bool OR = decltype(has_or)::value;
            if (eval) return launch_with_lds(k_eval_flat_keyed<NR, OR>, grid, block, lds, s, a);
            return launch_with_lds(k_garble_flat_keyed<NR, OR>, grid, block, lds, s, a);
        });
    });
}

}  // namespace gc
