// aes_schedule.h — the AES key schedule (FIPS-197 5.2) of one key per lane, for the kernels that expand many keys at once
// (k_expand_keys of the keyed batch passes, k_rand_expand of the random streams).  The S-box is byte 1 of Te0, kept in LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gc {

// sbox: 256 bytes of LDS, filled by the whole workgroup; the caller synchronises
__device__ __forceinline__ void load_sbox(uint8_t *sbox, const uint32_t *__restrict__ g_te0) {
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) sbox[i] = (uint8_t)(g_te0[i] >> 8);
}

// key: 4 (NR - 6) bytes -> w: the NR + 1 round keys as big-endian words, plain (nothing folded)
template <int NR>
__device__ __forceinline__ void aes_key_schedule(const uint8_t *__restrict__ key, const uint8_t *sbox, uint32_t (&w)[4 * (NR + 1)]) {
    constexpr int NK = NR - 6, NW = 4 * (NR + 1);
    auto subword = [&](uint32_t v) {
        return ((uint32_t)sbox[v >> 24] << 24) | ((uint32_t)sbox[(v >> 16) & 0xff] << 16) |
               ((uint32_t)sbox[(v >> 8) & 0xff] << 8) | (uint32_t)sbox[v & 0xff];
    };
#pragma unroll
    for (int i = 0; i < NK; i++)
        w[i] = ((uint32_t)key[4 * i] << 24) | ((uint32_t)key[4 * i + 1] << 16) | ((uint32_t)key[4 * i + 2] << 8) |
               (uint32_t)key[4 * i + 3];
    uint32_t rcon = 0x01u;
#pragma unroll
    for (int i = NK; i < NW; i++) {
        uint32_t t = w[i - 1];
        if (i % NK == 0) {
            t = subword((t << 8) | (t >> 24)) ^ (rcon << 24);
            rcon = ((rcon << 1) ^ ((rcon & 0x80u) ? 0x11bu : 0u)) & 0xffu;
        } else if (NK > 6 && i % NK == 4) {
            t = subword(t);
        }
        w[i] = w[i - NK] ^ t;
    }
}

}  // namespace gc
