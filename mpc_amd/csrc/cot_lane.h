// cot_lane.h — what a lane of the MITCCRH / COT pad kernels (k_mitccrh, k_cot_send, k_cot_recv, k_cot_dual in
// ot_kernels.hip; k_cot_multi in iknp_multi_kernels.hip) does for its OT: the per-OT AES key, and for the kernels around the
// perm-addressed dual table the hash of the lane's labels under it.  Device code only.
#pragma once

#include "aes_device.h"
#include "aes_otf_dual.h"

namespace gc {

// MITCCRH key of OT index gid: BE(Label{D0:gid, D1:0} ^ seed)   (mitccrh.go:70-82)
__device__ __forceinline__ void mitccrh_key(uint4 seed, uint64_t gid, uint32_t (&k)[4]) {
    const uint64_t d0 = (((uint64_t)seed.y << 32) | seed.x) ^ gid;
    k[0] = (uint32_t)(d0 >> 32);
    k[1] = (uint32_t)d0;
    k[2] = seed.w;
    k[3] = seed.z;
}

// NB labels hashed under one key: h[b] = x[b] ^ AES_k(x[b])  (mitccrh.go:107-127), the key schedule in the lane.
// k is DESTROYED: aes128_otf_dual runs the key schedule in place, so afterwards k is no longer the key; a caller that needs
// the key again makes it again (mitccrh_key).  lo0 = te_lane_off() with the dual table at LDS offset 0.
template <int NB>
__device__ __forceinline__ void mitccrh_pads(const uint4 (&x)[NB], uint32_t (&k)[4], uint32_t lo0, uint4 (&h)[NB]) {
    uint32_t s[NB][4];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        s[b][0] = x[b].y;
        s[b][1] = x[b].x;
        s[b][2] = x[b].w;
        s[b][3] = x[b].z;
    }
    aes128_otf_dual<NB>(s, k, lo0);
#pragma unroll
    for (int b = 0; b < NB; b++) h[b] = lxor(x[b], cols_to_label(s[b]));
}

}  // namespace gc
