// kos_clmul.h — the 128 x 128 carry-less multiply of the KOS sums (ot/mul128_generic.go), accumulated unreduced: one loop for
// k_kos_accumulate (ot_kernels.hip) and k_kos_multi (kos_multi_kernels.hip).  128-bit values are little-endian word vectors
// (D0 low, D0 high, D1 low, D1 high: the uint4 component order).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gc {

// p[0..7] ^= chi * b: four 128 x 32-bit partial products of 5 words each, added at word offset w.  Per bit one mask, five
// (q ^= cur & m) as v_bitop3 and five shifts.
__device__ __forceinline__ void kos_clmul_acc(uint32_t (&p)[8], const uint32_t (&chi)[4], const uint32_t (&bw)[4]) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint32_t cur[5] = {chi[0], chi[1], chi[2], chi[3], 0u}, q[5] = {0u, 0u, 0u, 0u, 0u};
        uint32_t word = bw[w];
#pragma unroll 8
        for (int k = 0; k < 32; k++) {
            const uint32_t m = 0u - (word & 1u);
            word >>= 1;
#pragma unroll
            for (int t = 0; t < 5; t++) q[t] = __builtin_amdgcn_bitop3_b32(q[t], cur[t], m, 0x78);  // q ^ (cur & m)
#pragma unroll
            for (int t = 4; t > 0; t--) cur[t] = __builtin_amdgcn_alignbit(cur[t], cur[t - 1], 31);
            cur[0] <<= 1;
        }
#pragma unroll
        for (int t = 0; t < 5; t++) p[w + t] ^= q[t];
    }
}

}  // namespace gc
