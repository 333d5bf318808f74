// iknp_multi_stream.h — what a lane of the multi-session IKNP kernels (iknp_multi_kernels.hip, iknp_multi_bits_kernels.hip)
// does with its column: the AES-128-CTR keystream of a base label from a byte position on, the key schedule in the lane.
// What these kernels share with k_iknp_fused (LDS accesses, chunk buffer, transposing wave, the loads and stores of a column
// of the u message) is in iknp_chunk.h, included here.  Device code only.
#pragma once

#include "aes_device.h"
#include "aes_otf_dual.h"
#include "iknp_chunk.h"

namespace gc {

// Keystream block j of the lane's column as four little-endian dwords.  The key schedule runs again for every block
// (aes128_otf_dual consumes its key), and the blocks go one at a time: the case this kernel is for needs one, and two in
// lock-step next to the finished stream words do not fit the 128 VGPRs of a 1024-lane workgroup.  HI0: every counter of the
// launch is below 2^32 (launch-uniform), word 2 of the block is the literal zero.
template <bool HI0>
__device__ __forceinline__ void stream_block(const uint32_t (&key)[4], uint64_t j, uint32_t lo0, uint32_t (&out)[4]) {
    uint32_t k[4] = {key[0], key[1], key[2], key[3]};
    uint32_t s[1][4] = {{0u, 0u, HI0 ? 0u : (uint32_t)(j >> 32), (uint32_t)j}};
    aes128_otf_dual<1>(s, k, lo0);
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = __builtin_bswap32(s[0][c]);
}

// The keystream bytes of one column from stream byte position p on (p mod 16 == sh, launch-uniform), as far as nb blocks
// (1 .. 5, 5 only when MISALIGNED) give them: t[0..15] little-endian dwords, zero behind.  prg() of iknp.go:632-637 restated
// for a lane.  Off a block boundary quarter q of the column is bytes [sh, sh + 16) of blocks q and q + 1: it is cut out as
// soon as block q + 1 is there (zeros when it is not needed), so only one block waits next to the finished quarters.
template <bool MISALIGNED, bool HI0>
__device__ __forceinline__ void column_stream(uint64_t p, uint32_t sh, uint32_t nb, const uint32_t (&key)[4], uint32_t lo0,
                                              uint32_t (&t)[16]) {
    const uint64_t j0 = p >> 4;
    if constexpr (!MISALIGNED) {
#pragma unroll
        for (int b = 0; b < 4; b++) {
            uint32_t cur[4] = {0u, 0u, 0u, 0u};
            if ((uint32_t)b < nb) stream_block<HI0>(key, j0 + b, lo0, cur);
#pragma unroll
            for (int i = 0; i < 4; i++) t[4 * b + i] = cur[i];
        }
    } else {
        const uint32_t ws = sh >> 2, bs = sh & 3u;  // dwords and bytes of the shift
        uint32_t c[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the block before | the block
#pragma unroll
        for (int b = 0; b < 5; b++) {
#pragma unroll
            for (int i = 0; i < 4; i++) c[i] = c[4 + i], c[4 + i] = 0u;
            if ((uint32_t)b < nb) {
                uint32_t cur[4];
                stream_block<HI0>(key, j0 + b, lo0, cur);
#pragma unroll
                for (int i = 0; i < 4; i++) c[4 + i] = cur[i];
            }
            if (b > 0) {
                uint32_t d[5];  // dwords ws .. ws + 4 of the pair
#pragma unroll
                for (int i = 0; i < 5; i++) d[i] = ws == 0 ? c[i] : ws == 1 ? c[i + 1] : ws == 2 ? c[i + 2] : c[i + 3];
#pragma unroll
                for (int i = 0; i < 4; i++) t[4 * (b - 1) + i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], bs);
            }
        }
    }
}

}  // namespace gc
