// iknp_chunk.h — what the IKNP extension kernels (k_iknp_fused, k_iknp_multi, k_iknp_multi_recv_bits) share around a chunk
// of 128 columns x 64 bytes: the LDS accesses by byte address, the swizzled chunk buffer, the wave that transposes it into
// 512 labels (createLabels, iknp.go:647-683) and the byte-granular loads and stores of a column of the u message.
// Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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

// Position (in dwords) of dword rd of column col inside a chunk buffer (kChunkBuf bytes).  Chosen so that
//   * the lane = column ds_write_b128 of a keystream quarter hits 8 distinct 16-byte bank slots per 8 lanes,
//   * the transposing wave (lane = rd * 4 + column group) reads dword rd of column (cg * 32 + k) from 32 distinct
//     banks per 32 lanes for every k, and
//   * for a fixed lane the 32 read addresses are one of FOUR bases plus the immediate 64 k (4 address registers
//     instead of 32).
constexpr uint32_t kCgStride = 520;              // dwords per column group: 32 columns x 16 + 8 (bank skew)
constexpr uint32_t kChunkBuf = 512 * 16 + 16 * 16;  // 8 448 bytes: >= 4 * kCgStride * 4 for the columns, and room for the
                                                   // 512 labels with one 16-byte pad per 32 labels on the way out
__device__ __forceinline__ uint32_t chunk_pos(uint32_t col, uint32_t rd) {
    const uint32_t cg = col >> 5, k = col & 31u;
    return cg * kCgStride + k * 16u + (((rd >> 2) ^ ((k >> 1) & 3u)) << 2) + (rd & 3u);
}

// The lane's keystream quarters q < nq of column col (t[0..15], little-endian dwords) into the chunk buffer at byte address
// bufaddr.  A literal nq = 4 leaves four unguarded stores.
__device__ __forceinline__ void chunk_put_quarters(uint32_t bufaddr, uint32_t col, const uint32_t (&t)[16], uint32_t nq) {
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
        if (q < nq)
            lds_st4(bufaddr + 4 * chunk_pos(col, 4 * q), make_uint4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]));
}

// createLabels for the chunk buffer at byte address wbuf, by one wave of k_iknp_multi: dst[r] = label r for r < wrows (<= 512).
// lane = (rd, cg): dword rd (OTs 32rd .. 32rd+31) of the 32 columns of group cg.  A dword row without an OT was not written
// by chunk_put_quarters (nq short of 4) and is not read, transposed or written back here.
// k_iknp_fused keeps its own unguarded copy of this wave (iknp_fused_kernels.hip): called from there, this function made the
// one-session receiver 1 - 2 % slower in every form tried, at the same register counts, waits and LDS accesses.
// Keep the two in step.
__device__ __forceinline__ void chunk_create_labels(uint32_t wbuf, uint32_t lane, uint32_t wrows, uint4 *__restrict__ dst) {
    const uint32_t rd = lane >> 2, cg = lane & 3u;
    if (32u * rd < wrows) {
        uint32_t base[4];
#pragma unroll
        for (uint32_t h = 0; h < 4; h++)
            base[h] = wbuf + 4 * (cg * kCgStride + (((rd >> 2) ^ h) << 2) + (rd & 3u));  // chunk_pos without 16 k
        uint32_t x[32];
#pragma unroll
        for (uint32_t k = 0; k < 32; k++) x[k] = lds_ld1(base[(k >> 1) & 3u] + 64u * k);
        // 32 x 32 bit transpose (masked swaps): afterwards x[i] bit k = column (cg*32+k), OT 32rd+i
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {  // stage 16 swaps half-words: two byte permutes where the masked swap takes four
            const uint32_t a = x[k], b = x[k + 16];
            x[k] = __builtin_amdgcn_perm(b, a, 0x05040100u);
            x[k + 16] = __builtin_amdgcn_perm(b, a, 0x07060302u);
        }
        uint32_t msk = 0x00ff00ffu;
#pragma unroll
        for (uint32_t j = 8; j != 0; j >>= 1, msk ^= msk << j) {
#pragma unroll
            for (uint32_t k = 0; k < 32; k = ((k | j) + 1) & ~j) {
                const uint32_t tt = ((x[k] >> j) ^ x[k | j]) & msk;
                x[k] ^= tt << j;
                x[k | j] ^= tt;
            }
        }
        // labels back through the same buffer (all reads of this wave are done: a wave's DS operations execute
        // in order and every write depends on the lane's 32 reads); label r sits at 16 * (r + r / 32): the pad
        // per 32 labels keeps the dword stores conflict-free and every address a base plus an immediate
        const uint32_t wbase = wbuf + 16 * (33 * rd) + 4 * cg;
#pragma unroll
        for (uint32_t i = 0; i < 32; i++) lds_st1(wbase + 16 * i, x[i]);
    }
    const uint32_t rbase = wbuf + 16 * (lane + (lane >> 5));
#pragma unroll
    for (uint32_t mth = 0; mth < 8; mth++) {
        const uint32_t r = lane + 64 * mth;  // label r was written by the lanes of dword row r / 32 < ceil(wrows / 32)
        // read before the test on purpose: for r >= wrows these are words of the buffer (in bounds: at most byte 8 432 of
        // 8 448) that nobody wrote in this step, and the value is dropped
        const uint4 v = lds_ld4(rbase + 16 * 66 * mth);
        if (r < wrows) dst[r] = v;  // uint4 = {D0 lo, D0 hi, D1 lo, D1 hi}: columns 0-31, 32-63, ...
    }
}

__device__ __forceinline__ uint32_t load_u8s(const uint8_t *src, uint32_t nbytes) {  // up to 4 bytes, little-endian
    uint32_t v = 0;
    for (uint32_t b = 0; b < nbytes; b++) v |= (uint32_t)src[b] << (8 * b);
    return v;
}

// bytes [16q, 16q + 16) of a column of byte_rows (<= 64) bytes, 16q < byte_rows; bytes past byte_rows read as zero and are
// not written.  whole: the caller knows that the column starts 16-byte aligned and that its length is a multiple of 16, and
// it goes as whole quarters; any other goes byte by byte.  k_iknp_fused says so of full chunks only (col * 64 behind the
// caller's pointer: a shorter last chunk asks nothing of that pointer), the multi kernels of every length that is a multiple
// of 16 (col * byte_rows behind an offset that is a multiple of 128).
__device__ __forceinline__ uint4 load_quarter(const uint8_t *src, uint32_t byte_rows, uint32_t q, bool whole) {
    if (whole) return ((const uint4 *)src)[q];
    uint32_t v[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t o = 16u * q + 4u * i;
        v[i] = o < byte_rows ? load_u8s(src + o, byte_rows - o < 4 ? byte_rows - o : 4) : 0;
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_quarter(uint8_t *dst, uint32_t byte_rows, uint32_t q, uint4 x, bool whole) {
    if (whole) {
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
