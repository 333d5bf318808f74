// iknp_multi_stream.h — what a lane of the multi-session IKNP kernels (iknp_multi_kernels.hip, iknp_multi_bits_kernels.hip)
// does with its column: the AES-128-CTR keystream of a base label from a byte position on, the byte-granular loads and
// stores of a column of the u message, and the 16-byte LDS accesses of the chunk buffers.  Device code only.
#pragma once

#include "aes_device.h"
#include "aes_otf_dual.h"

namespace gc {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
using lds_u4 = __attribute__((address_space(3))) u32x4;
using lds_w32 = __attribute__((address_space(3))) uint32_t;

__device__ __forceinline__ uint4 lds_ld4(uint32_t addr) {
    const u32x4 v = *(lds_u4 *)(uintptr_t)addr;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void lds_st4(uint32_t addr, uint4 v) {
    u32x4 w;
    w.x = v.x, w.y = v.y, w.z = v.z, w.w = v.w;
    *(lds_u4 *)(uintptr_t)addr = w;
}
__device__ __forceinline__ uint32_t lds_ld1(uint32_t addr) { return *(lds_w32 *)(uintptr_t)addr; }
__device__ __forceinline__ void lds_st1(uint32_t addr, uint32_t v) { *(lds_w32 *)(uintptr_t)addr = v; }

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

__device__ __forceinline__ uint32_t load_u8s(const uint8_t *src, uint32_t nbytes) {  // up to 4 bytes, little-endian
    uint32_t v = 0;
    for (uint32_t b = 0; b < nbytes; b++) v |= (uint32_t)src[b] << (8 * b);
    return v;
}

// bytes [16q, 16q + 16) of a column of byte_rows (<= 64) bytes, 16q < byte_rows; bytes past byte_rows read as zero and are
// not written.  A column whose length is a multiple of 16 starts 16-byte aligned (col * byte_rows behind an offset that is a
// multiple of 128) and goes as whole quarters; any other goes byte by byte.
__device__ __forceinline__ uint4 load_quarter(const uint8_t *src, uint32_t byte_rows, uint32_t q) {
    if ((byte_rows & 15u) == 0) return ((const uint4 *)src)[q];
    uint32_t v[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t o = 16u * q + 4u * i;
        v[i] = o < byte_rows ? load_u8s(src + o, byte_rows - o < 4 ? byte_rows - o : 4) : 0;
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_quarter(uint8_t *dst, uint32_t byte_rows, uint32_t q, uint4 x) {
    if ((byte_rows & 15u) == 0) {
        ((uint4 *)dst)[q] = x;
        return;
    }
    const uint32_t v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (uint32_t i = 0; i < 4; i++)
        for (uint32_t b = 0; b < 4; b++)
            if (16u * q + 4u * i + b < byte_rows) dst[16 * q + 4 * i + b] = (uint8_t)(v[i] >> (8 * b));
}

}  // namespace gc
