// aes_otf_dual.h — AES-128 with a per-lane key on the perm-addressed dual table (aes_device.h): the key schedule runs
// in the lane, one round ahead of the state.  Shared by the COT / ROT kernels (ot_kernels.hip) and the VOLE sender
// (vole_kernels.hip).
#pragma once

#include "aes_device.h"

namespace gc {

// SubWord(RotWord(w)) from four dual-table words: A = Te2[b2(w)], B = Te0[b1(w)], C = Te0[b0(w)], D = Te2[b3(w)]
// (S[x] is byte 3 and byte 0 of Te2[x], byte 2 and byte 1 of Te0[x]: the final-round selects of aes_encrypt_dual)
__device__ __forceinline__ uint32_t subrot_select(uint32_t A, uint32_t B, uint32_t C, uint32_t D) {
    const uint32_t hi = __builtin_amdgcn_bitop3_b32(0xff000000u, A, B, 0xCA);
    const uint32_t lo = __builtin_amdgcn_bitop3_b32(0x0000ff00u, C, D, 0xCA);
    return __builtin_amdgcn_bitop3_b32(0xffff0000u, hi, lo, 0xCA);
}

// N blocks under ONE per-lane AES-128 key k (big-endian words), key schedule on the fly; s in: plaintext columns,
// out: ciphertext columns
template <int N>
__device__ __forceinline__ void aes128_otf_dual(uint32_t (&s)[N][4], uint32_t (&k)[4], uint32_t lo0) {
    const uint32_t lo2 = lo0 + 128u;
    const uint32_t sel0 = GC_PERM_SEL(0), sel1 = GC_PERM_SEL(1), sel2 = GC_PERM_SEL(2), sel3 = GC_PERM_SEL(3);
#pragma unroll
    for (int b = 0; b < N; b++)
#pragma unroll
        for (int c = 0; c < 4; c++) s[b][c] ^= k[c];
    uint32_t rcon = 0x01000000u;
#pragma unroll
    for (int r = 1; r <= 10; r++) {
        uint32_t ad[N][16], t[N][16], ka[4], kt[4];
        // key schedule addresses: RotWord moves byte 2 to byte 3, 1 -> 2, 0 -> 1, 3 -> 0
        ka[0] = __builtin_amdgcn_perm(k[3], lo2, sel2);
        ka[1] = __builtin_amdgcn_perm(k[3], lo0, sel1);
        ka[2] = __builtin_amdgcn_perm(k[3], lo0, sel0);
        ka[3] = __builtin_amdgcn_perm(k[3], lo2, sel3);
        if (r < 10) {
#pragma unroll
            for (int b = 0; b < N; b++) te_round_addrs(s[b], lo0, lo2, ad[b]);
        } else {
#pragma unroll
            for (int b = 0; b < N; b++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    ad[b][4 * c + 0] = __builtin_amdgcn_perm(s[b][c], lo2, sel3);
                    ad[b][4 * c + 1] = __builtin_amdgcn_perm(s[b][(c + 1) & 3], lo0, sel2);
                    ad[b][4 * c + 2] = __builtin_amdgcn_perm(s[b][(c + 2) & 3], lo0, sel1);
                    ad[b][4 * c + 3] = __builtin_amdgcn_perm(s[b][(c + 3) & 3], lo2, sel0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; i++) kt[i] = *(lds_u32 *)(uintptr_t)ka[i];
#pragma unroll
        for (int b = 0; b < N; b++)
#pragma unroll
            for (int i = 0; i < 16; i++) t[b][i] = *(lds_u32 *)(uintptr_t)ad[b][i];
        __builtin_amdgcn_sched_barrier(0);
        k[0] ^= subrot_select(kt[0], kt[1], kt[2], kt[3]) ^ rcon;
        k[1] ^= k[0];
        k[2] ^= k[1];
        k[3] ^= k[2];
        rcon = r == 8 ? 0x1b000000u : rcon << 1;
#pragma unroll
        for (int b = 0; b < N; b++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (r < 10) {
                    s[b][c] = xor3(t[b][4 * c], t[b][4 * c + 1], k[c]) ^ rotr32(t[b][4 * c + 2] ^ t[b][4 * c + 3], 8);
                } else {
                    s[b][c] = subrot_select(t[b][4 * c], t[b][4 * c + 1], t[b][4 * c + 2], t[b][4 * c + 3]) ^ k[c];
                }
            }
    }
}

}  // namespace gc
