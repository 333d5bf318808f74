// rand_kernels.hip — CDNA4 kernels of the device random streams (gc_rand_*; rand_ctr.h defines the streams).
//
//   k_rand_expand  the plain AES key schedule of S seeds, one lane per seed (the shape of k_expand_keys, which folds the
//                  last round key for the hash and so cannot serve here), and the S IVs as two native words each
//   k_rand_fill    bytes [pos, pos + n) of every stream: MODE 0 into the caller's slots, MODE 1 as tripleBatch's shares
//                  a[i] = BE64(bytes 0..7), b[i] = BE64(bytes 8..15) of draw i (gmw/triples.go:301-310)
//
// k_rand_fill has the launch shape of the other AES-CTR kernels (k_vole_sender, k_cot_dual): persistent 1024-thread
// workgroups around the 64 KiB dual table, one per CU (66 VGPRs: four waves per SIMD).  A unit of work is one wave's run of
// 64 consecutive blocks of ONE stream (rand_ctr.h), so the round keys are wave-uniform and sit in SGPRs (the last four
// rounds' in VGPRs); wave w of the grid takes units w, w + waves, ... (64-bit), and reloads the keys only when the stream
// changes: never in one long stream, per unit in many short ones.
// A lane's block is stored as one 16-byte word, 1 KiB in a row per wave; the ragged first and last block of a slot, and
// every block of a slot whose blocks do not fall on multiples of 16 (a position in mid-block, an odd stride), go out
// bytewise.  Every address comes from S, n, stride and pos through rand_cover / rand_piece.
#include <algorithm>

#include "aes_device.h"
#include "aes_schedule.h"
#include "kernels.h"
#include "rand_ctr.h"

namespace gc {

namespace {

constexpr int kRandWaves = kRandThreads / 64;  // waves of a workgroup

template <int NR>
__global__ __launch_bounds__(kRandExpandThreads) void k_rand_expand(const uint8_t *__restrict__ seeds,
                                                                    const uint8_t *__restrict__ ivs, uint64_t S,
                                                                    const uint32_t *__restrict__ g_te0,
                                                                    uint32_t *__restrict__ rk_out, RandCtr *__restrict__ iv_out) {
    constexpr int NK = NR - 6, NW = 4 * (NR + 1);
    __shared__ uint8_t sbox[256];
    load_sbox(sbox, g_te0);
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * kRandExpandThreads + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kRandExpandThreads) {
        uint32_t w[NW];
        aes_key_schedule<NR>(seeds + s * (4 * NK), sbox, w);
        uint32_t *o = rk_out + s * NW;
#pragma unroll
        for (int i = 0; i < NW; i++) o[i] = w[i];
        iv_out[s] = ivs ? rand_ctr_from_bytes(ivs + s * 16) : RandCtr{0, 0};
    }
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    // (the builtin returns int: without the casts the low word would be sign-extended over the high one)
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    return ((uint64_t)hi << 32) | lo;
}

// rk: [S][4 (NR + 1)] (k_rand_expand), ivs: [S].  MODE 0: out = slots of `stride` bytes.  MODE 1: out = a, out_b = b, u64
// [S][n / 16], pos a multiple of 16.
template <int NR, int MODE>
__global__ __launch_bounds__(kRandThreads) void k_rand_fill(const uint32_t *__restrict__ rk_all, const RandCtr *__restrict__ ivs,
                                                            uint64_t S, uint64_t pos, uint64_t n, uint8_t *out, uint64_t stride,
                                                            uint64_t *out_b, const uint32_t *__restrict__ g_te0) {
    constexpr int NW = 4 * (NR + 1);
    extern __shared__ uint4 smem[];
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off(), lane = threadIdx.x & 63u;
    const RandCover cov = rand_cover(pos, n);
    const uint64_t ups = rand_units(cov.nblocks), units = S * ups;
    const uint64_t nwaves = (uint64_t)gridDim.x * kRandWaves;
    // unit u = (stream s, run r of it); a step adds nwaves = qn * ups + rn units: one division per kernel, none per unit
    uint64_t u = (uint64_t)blockIdx.x * kRandWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= units) return;
    const uint64_t qn = nwaves / ups, rn = nwaves - qn * ups;
    uint64_t s = uniform64(u / ups), r = uniform64(u - (u / ups) * ups);
    // the last four round keys live in VGPRs: with all 60 words of AES-256 in SGPRs the loop's own scalars spill
    uint32_t vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    while (s < S) {  // the units of this wave in stream s: one with short streams, all of them in one long stream
        uint32_t rk[NW];
        load_round_keys<NR>(rk, rk_all + s * NW);
#pragma unroll
        for (int i = NW - 16; i < NW; i++) rk[i] ^= vz;
        const RandCtr iv{uniform64(ivs[s].hi), uniform64(ivs[s].lo)};
        const uint64_t cur = s;
        do {
            const uint64_t k = r * kRandRun + lane;
            if (k < cov.nblocks) {
                const RandCtr c = rand_ctr_add(iv, cov.first + k);
                uint32_t st[1][4] = {{(uint32_t)(c.hi >> 32), (uint32_t)c.hi, (uint32_t)(c.lo >> 32), (uint32_t)c.lo}};
                aes_encrypt_dual<NR, 1>(st, rk, (const uint32_t *)smem, lo0);
                __builtin_amdgcn_sched_barrier(0);  // the addresses are worked out behind the rounds, not kept alive across them
                if constexpr (MODE == 1) {
                    const uint64_t at = s * (n >> 4) + k;
                    ((uint64_t *)out)[at] = ((uint64_t)st[0][0] << 32) | st[0][1];
                    out_b[at] = ((uint64_t)st[0][2] << 32) | st[0][3];
                } else {
                    const RandPiece p = rand_piece(cov, n, k);
                    uint8_t *slot = out + s * stride;
                    const bool aligned = (((uintptr_t)slot - cov.head) & 15u) == 0;  // every whole block of the slot, or none
                    // the block as it lies in memory: w0 holds bytes 0..3, byte 0 lowest
                    uint32_t w0 = __builtin_bswap32(st[0][0]), w1 = __builtin_bswap32(st[0][1]);
                    uint32_t w2 = __builtin_bswap32(st[0][2]), w3 = __builtin_bswap32(st[0][3]);
                    if (aligned && p.from == 0 && p.to == 16) {
                        *(uint4 *)(slot + p.at) = make_uint4(w0, w1, w2, w3);
                    } else {
                        uint8_t *dst = slot + p.at - p.from;  // where byte 0 of the block would go
#pragma unroll 1
                        for (uint32_t b = 0; b < p.to; b++) {
                            if (b >= p.from) dst[b] = (uint8_t)w0;
                            w0 = __builtin_amdgcn_alignbit(w1, w0, 8);
                            w1 = __builtin_amdgcn_alignbit(w2, w1, 8);
                            w2 = __builtin_amdgcn_alignbit(w3, w2, 8);
                            w3 >>= 8;
                        }
                    }
                }
            }
            s += qn;
            r += rn;
            if (r >= ups) {
                r -= ups;
                s++;
            }
        } while (s == cur);
    }
}

template <int MODE>
hipError_t launch_fill(int rounds, const uint32_t *rk, const RandCtr *ivs, size_t S, uint64_t pos, uint64_t n, void *out,
                       size_t stride, uint64_t *out_b, const uint32_t *te0, hipStream_t s) {
    const uint64_t units = (uint64_t)S * rand_units(rand_cover(pos, n).nblocks);
    const unsigned grid = (unsigned)std::min<uint64_t>(kRandGrid, (units + kRandWaves - 1) / kRandWaves);
    return with_rounds(rounds, [&](auto nr) {
        return launch_with_lds(k_rand_fill<decltype(nr)::value, MODE>, grid, kRandThreads, kTeDualBytes, s, rk, ivs, (uint64_t)S, pos,
                               n, (uint8_t *)out, (uint64_t)stride, out_b, te0);
    });
}

}  // namespace

hipError_t launch_rand_expand(const uint8_t *d_seeds, int rounds, const uint8_t *d_ivs, size_t S, const uint32_t *te0,
                              uint32_t *d_rk, RandCtr *d_iv, hipStream_t s) {
    const unsigned grid = (unsigned)std::min<uint64_t>(kRandExpandGrid, ((uint64_t)S + kRandExpandThreads - 1) / kRandExpandThreads);
    return with_rounds(rounds, [&](auto nr) {
        return launch_kernel(k_rand_expand<decltype(nr)::value>, grid, kRandExpandThreads, s, d_seeds, d_ivs, (uint64_t)S, te0, d_rk,
                             d_iv);
    });
}

hipError_t launch_rand_fill(int rounds, const uint32_t *d_rk, const RandCtr *d_iv, size_t S, uint64_t pos, uint64_t n,
                            uint8_t *d_out, size_t stride, const uint32_t *te0, hipStream_t s) {
    return launch_fill<0>(rounds, d_rk, d_iv, S, pos, n, d_out, stride, nullptr, te0, s);
}

hipError_t launch_rand_gmw_shares(int rounds, const uint32_t *d_rk, const RandCtr *d_iv, size_t S, uint64_t pos, uint64_t words,
                                  uint64_t *d_a, uint64_t *d_b, const uint32_t *te0, hipStream_t s) {
    return launch_fill<1>(rounds, d_rk, d_iv, S, pos, 16 * words, d_a, 0, d_b, te0, s);
}

}  // namespace gc
