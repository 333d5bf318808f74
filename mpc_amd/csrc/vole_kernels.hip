// vole_kernels.hip — CDNA4 kernels of the packed-IKNP VOLE (vole/vole.go, vole/prg.go).
//
//   k_vole_sender    (*Sender).Mul's per-label work (vole.go:58-97): r = BE256(AES-CTR_label(0^32)) mod p,
//                    u = (r + x * y mod p) mod p
//   k_vole_receiver  (*Receiver).Mul's reduction (vole.go:182-187): us = BE256(u_msg) mod p
//
// Every value is 32 bytes big-endian, element i at [32i, 32i + 32): the reference's messages as they are (bytes32,
// vole.go:219-227).  One lane = one element.  The sender is the ROT kernel's shape (k_cot_dual<1, 2>, ot_kernels.hip):
// persistent 1024-thread workgroups around the 64 KiB dual AES table, one per-lane AES-128 key schedule and two blocks,
// then the arithmetic mod p (vole_mod.h) instead of the feed-forward XOR: two Montgomery products for x * y, two more for
// the reduction of the pad when p < 2^255 (above, one conditional subtraction).  The receiver needs no table.
#include <algorithm>

#include "aes_otf_dual.h"
#include "kernels.h"
#include "vole_mod.h"

namespace gc {

namespace {

constexpr int kVoleThreads = 1024;   // sender: as k_cot_dual
constexpr int kVoleGrid = 512;       // persistent workgroups, two per CU (64 KiB of LDS each; grid-stride)
constexpr int kVoleRecvThreads = 256;
constexpr int kVoleRecvGrid = 2048;

__device__ __forceinline__ void load_be256(const uint4 *p, uint32_t (&v)[kVoleLimbs]) {
    const uint4 a = p[0], b = p[1];
    const uint32_t w[kVoleLimbs] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    vole_from_be_words(w, v);
}

__device__ __forceinline__ void store_be256(uint4 *p, const uint32_t (&v)[kVoleLimbs]) {
    uint32_t w[kVoleLimbs];
    vole_to_be_words(v, w);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// labels: gc_label [m] (the layout gc_iknp_send_dev writes); x, y_msg, r_out, u_out: 32 bytes per element
__global__ __launch_bounds__(kVoleThreads) void k_vole_sender(VoleMod mod, const uint4 *__restrict__ labels, const uint4 *x,
                                                              const uint4 *y_msg, size_t m, uint4 *r_out, uint4 *u_out,
                                                              const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off();
    for (size_t i = (size_t)blockIdx.x * kVoleThreads + threadIdx.x; i < m; i += (size_t)gridDim.x * kVoleThreads) {
        // key = GetData(label) = BE64(D0) || BE64(D1) (label.go:105-108): big-endian words {y, x, w, z}
        const uint4 l = labels[i];
        uint32_t k[4] = {l.y, l.x, l.w, l.z};
        // AES-CTR, zero IV, over 32 zero bytes (prg.go:16-27): counter blocks 0 and 1
        uint32_t s[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 1u}};
        aes128_otf_dual<2>(s, k, lo0);
        // pad = the 32 key-stream bytes as one big-endian integer: limb 7 = first column of block 0
        uint32_t pad[kVoleLimbs];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            pad[7 - c] = s[0][c];
            pad[3 - c] = s[1][c];
        }
        uint32_t r[kVoleLimbs], xv[kVoleLimbs], yv[kVoleLimbs], t[kVoleLimbs];
        vole_reduce(pad, mod, r);                  // r = pad mod p (vole.go:71-73)
        load_be256(y_msg + 2 * i, yv);
        load_be256(x + 2 * i, xv);
        vole_mul_mod(xv, yv, mod, t);              // x * (y mod p) mod p = x * y mod p (vole.go:86-95)
        vole_add_mod(r, t, mod, t);                // u = (r + t) mod p
        store_be256(r_out + 2 * i, r);
        store_be256(u_out + 2 * i, t);
    }
}

// u_out may be u_msg (in place): a lane reads its element before it writes it
__global__ __launch_bounds__(kVoleRecvThreads) void k_vole_receiver(VoleMod mod, const uint4 *u_msg, size_t m, uint4 *u_out) {
    for (size_t i = (size_t)blockIdx.x * kVoleRecvThreads + threadIdx.x; i < m; i += (size_t)gridDim.x * kVoleRecvThreads) {
        uint32_t v[kVoleLimbs], r[kVoleLimbs];
        load_be256(u_msg + 2 * i, v);
        vole_reduce(v, mod, r);
        store_be256(u_out + 2 * i, r);
    }
}

}  // namespace

// grids are computed in 64 bits and capped; the kernels' grid-stride loops cover any m
hipError_t launch_vole_sender(const VoleMod &mod, const uint4 *labels, const uint4 *x, const uint4 *y_msg, size_t m, uint4 *r_out,
                              uint4 *u_out, const uint32_t *te0, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>(kVoleGrid, (m + kVoleThreads - 1) / kVoleThreads);
    return launch_with_lds(k_vole_sender, grid, kVoleThreads, kTeDualBytes, s, mod, labels, x, y_msg, m, r_out, u_out, te0);
}

hipError_t launch_vole_receiver(const VoleMod &mod, const uint4 *u_msg, size_t m, uint4 *u_out, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>(kVoleRecvGrid, (m + kVoleRecvThreads - 1) / kVoleRecvThreads);
    return launch_kernel(k_vole_receiver, grid, kVoleRecvThreads, s, mod, u_msg, m, u_out);
}

}  // namespace gc
