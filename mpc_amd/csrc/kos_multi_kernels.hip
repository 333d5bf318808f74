// kos_multi_kernels.hip — the KOS consistency check of the malicious IKNP variant for S sessions of equal length in one launch
// (gc_kos_multi_*): byte for byte what gc_kos_receiver_tags / gc_kos_sender_check give on each session alone
// (ot/iknp.go:138-194, 405-465; ot/gf128.go:14-27; ot/mul128_generic.go).
//
// k_kos_multi has the outer shape of k_cot_multi / k_kos_accumulate: persistent workgroups of kKosMultiThreads lanes, at most
// kKosMultiGrid of them, around the perm-addressed dual AES table.  Where k_kos_accumulate spreads ONE session's labels over
// the whole grid and meets in six 64-bit atomics on a zeroed accumulator, here a TEAM of lanes owns a session from its first
// label to its tags (kos_multi.h: which team, which label, which choice bit):
//   * a lane walks labels tl, tl + team, ... of the session's per + 256, encrypts the counter under the session's chi key and
//     XORs the 256-bit product and (receiver) the selected chi into ITS registers: the sums are linear;
//   * the chi key is seed2[s]: 16 bytes, uniform over the team.  Every lane expands it ONCE per session into 44 round-key
//     registers of its own (expand_key_dual: the schedule of aes_otf_dual.h) and encrypts its blocks with the 24-VALU round of
//     aes_encrypt_dual, as k_kos_accumulate does from its SGPRs: 106 - 115 VGPRs, under the 128 of a 1024-lane workgroup.
//     (Moved into SGPRs with readfirstlane the keys cost two SGPR spills in one instantiation; expanded next to every block,
//     as in k_cot_multi, the kernel needs 71 VGPRs and 8 % more time at (1 024, 128): EXPERIMENTS.md.)
//   * sender: the last lane of the team also adds x_s * delta_s, so the folded sum is q ^ x * Delta;
//   * the team is folded with wave shuffles and, when it is the whole workgroup, through 768 bytes of LDS behind the table;
//   * lane 0 writes the three tags (receiver) or compares with (t0, t1) and writes the verdict byte (sender) with plain vector
//     stores.  A failing session costs one atomic add and one atomic min on the status block; an honest run issues none.
// WG = false: a team is one wave (n = per + 256 <= kKosMultiWaveMax), 16 sessions per workgroup and trip; WG = true: the
// whole workgroup.  Sessions go round the workgroups first (kos_multi_session), so 1 024 short sessions run as 4 waves on each
// of 256 compute units, not as 16 on each of 64.
#include <algorithm>

#include "aes_device.h"
#include "aes_otf_dual.h"
#include "kernels.h"
#include "kos_clmul.h"
#include "kos_multi.h"

namespace gc {

namespace {

constexpr uint32_t KT = kKosMultiThreads;
constexpr uint32_t kFoldWords = 12;                              // 8 of the product sum, 4 of x
constexpr uint32_t kFoldBytes = (KT / 64) * kFoldWords * 4;      // one row per wave, behind the table

// the 44 round-key words of AES-128 under key k (big-endian words): the schedule of aes128_otf_dual, run once
__device__ __forceinline__ void expand_key_dual(const uint32_t (&key)[4], uint32_t lo0, uint32_t (&rk)[44]) {
    const uint32_t lo2 = lo0 + 128u;
    const uint32_t sel0 = GC_PERM_SEL(0), sel1 = GC_PERM_SEL(1), sel2 = GC_PERM_SEL(2), sel3 = GC_PERM_SEL(3);
#pragma unroll
    for (int c = 0; c < 4; c++) rk[c] = key[c];
    uint32_t rcon = 0x01000000u;
#pragma unroll
    for (int r = 1; r <= 10; r++) {
        const uint32_t w = rk[4 * r - 1];
        const uint32_t a = *(lds_u32 *)(uintptr_t)__builtin_amdgcn_perm(w, lo2, sel2);
        const uint32_t b = *(lds_u32 *)(uintptr_t)__builtin_amdgcn_perm(w, lo0, sel1);
        const uint32_t c = *(lds_u32 *)(uintptr_t)__builtin_amdgcn_perm(w, lo0, sel0);
        const uint32_t d = *(lds_u32 *)(uintptr_t)__builtin_amdgcn_perm(w, lo2, sel3);
        rk[4 * r] = rk[4 * r - 4] ^ subrot_select(a, b, c, d) ^ rcon;
        rk[4 * r + 1] = rk[4 * r - 3] ^ rk[4 * r];
        rk[4 * r + 2] = rk[4 * r - 2] ^ rk[4 * r + 1];
        rk[4 * r + 3] = rk[4 * r - 1] ^ rk[4 * r + 2];
        rcon = r == 8 ? 0x1b000000u : rcon << 1;
    }
}

template <bool SEND, bool WG>
__global__ __launch_bounds__(KT) void k_kos_multi(const uint4 *__restrict__ seed2, const uint4 *__restrict__ result,
                                                  const uint8_t *__restrict__ choice, const uint4 *__restrict__ cv,
                                                  const uint8_t *__restrict__ bcv, const uint4 *__restrict__ delta,
                                                  const uint4 *__restrict__ tags_in, uint64_t S, uint64_t per,
                                                  uint4 *__restrict__ tags_out, uint8_t *__restrict__ ok,
                                                  unsigned long long *__restrict__ status,
                                                  const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    constexpr uint32_t TEAM = WG ? KT : 64u, TPW = KT / TEAM;
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t team = WG ? 0u : wave, tl = WG ? threadIdx.x : lane;
    const uint64_t n = kos_multi_labels(per);
    uint32_t *red = (uint32_t *)smem + kTeDualBytes / 4;  // WG only

    for (uint64_t trip = 0;; trip++) {
        const uint64_t s = kos_multi_session(blockIdx.x, team, trip, gridDim.x, TPW);  // uniform over the team
        if (s >= S) break;
        const uint4 sd = seed2[s];
        const uint32_t key[4] = {sd.y, sd.x, sd.w, sd.z};  // BE(seed2) (newPrg, iknp.go:622-630)
        uint32_t rk[44];
        expand_key_dual(key, lo0, rk);
        uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, xs[4] = {0, 0, 0, 0};
        for (uint64_t i = tl; i < n; i += TEAM) {
            const KosMultiLabel m = kos_multi_label(s, i, per);
            // chi_i = AES(BE128(i)); the ciphertext columns are the label's big-endian words (k_kos_accumulate)
            uint32_t st[1][4] = {{0u, 0u, (uint32_t)(m.ctr >> 32), (uint32_t)m.ctr}};
            aes_encrypt_dual<10, 1, 0>(st, rk, (const uint32_t *)smem, lo0);
            const uint32_t chi[4] = {st[0][1], st[0][0], st[0][3], st[0][2]};
            const uint4 b = (m.in_cv ? cv : result)[m.off];
            const uint32_t bw[4] = {b.x, b.y, b.z, b.w};
            kos_clmul_acc(p, chi, bw);
            if (!SEND) {
                const uint32_t byte = (m.in_cv ? bcv : choice)[m.bit_byte];
                const uint32_t msk = 0u - ((byte >> m.bit) & 1u);
#pragma unroll
                for (int t = 0; t < 4; t++) xs[t] ^= chi[t] & msk;
            }
        }
        if (SEND && tl == TEAM - 1) {  // mul128(x, s.Delta) (iknp.go:186)
            const uint4 x = tags_in[3 * s], d = delta[s];
            const uint32_t xw[4] = {x.x, x.y, x.z, x.w}, dw[4] = {d.x, d.y, d.z, d.w};
            kos_clmul_acc(p, xw, dw);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int q = 0; q < 8; q++) p[q] ^= __shfl_xor(p[q], off, 64);
            if (!SEND) {
#pragma unroll
                for (int q = 0; q < 4; q++) xs[q] ^= __shfl_xor(xs[q], off, 64);
            }
        }
        if (WG) {
            // the 16 waves through LDS: wave w leaves its 12 words in row w, lane q < 12 of wave 0 folds column q.  The rows are
            // free again once every lane is past the second barrier, which is before any lane writes them on the next trip.
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 8; q++) red[wave * kFoldWords + q] = p[q];
#pragma unroll
                for (int q = 0; q < 4; q++) red[wave * kFoldWords + 8 + q] = xs[q];
            }
            __syncthreads();
            if (wave == 0) {
                uint32_t r = 0;
                if (lane < kFoldWords)
                    for (uint32_t w = 0; w < KT / 64; w++) r ^= red[w * kFoldWords + lane];
                // back into every lane of wave 0, in the order the wave form has them
#pragma unroll
                for (int q = 0; q < 8; q++) p[q] = __shfl(r, q, 64);
#pragma unroll
                for (int q = 0; q < 4; q++) xs[q] = __shfl(r, 8 + q, 64);
            }
            __syncthreads();
        }
        if (tl == 0) {
            if (SEND) {
                const uint4 t0 = tags_in[3 * s + 1], t1 = tags_in[3 * s + 2];
                const uint32_t diff = (p[0] ^ t0.x) | (p[1] ^ t0.y) | (p[2] ^ t0.z) | (p[3] ^ t0.w) | (p[4] ^ t1.x) |
                                      (p[5] ^ t1.y) | (p[6] ^ t1.z) | (p[7] ^ t1.w);
                ok[s] = diff == 0u ? 1 : 0;
                if (diff != 0u) {  // "OT extension check failed" (iknp.go:190-192)
                    atomicAdd(&status[0], 1ull);
                    atomicMin(&status[1], (unsigned long long)s);
                }
            } else {
                tags_out[3 * s] = make_uint4(xs[0], xs[1], xs[2], xs[3]);
                tags_out[3 * s + 1] = make_uint4(p[0], p[1], p[2], p[3]);
                tags_out[3 * s + 2] = make_uint4(p[4], p[5], p[6], p[7]);
            }
        }
    }
}

template <typename K>
hipError_t launch(K kern, bool wg, const uint4 *seed2, const uint4 *result, const uint8_t *choice, const uint4 *cv,
                  const uint8_t *bcv, const uint4 *delta, const uint4 *tags_in, size_t S, size_t per, uint4 *tags_out,
                  uint8_t *ok, unsigned long long *status, const uint32_t *te0, hipStream_t s) {
    const size_t lds = kTeDualBytes + (wg ? kFoldBytes : 0);
    return launch_with_lds(kern, kos_multi_grid(S, kKosMultiGrid), KT, lds, s, seed2, result, choice, cv, bcv, delta, tags_in,
                           (uint64_t)S, (uint64_t)per, tags_out, ok, status, te0);
}

}  // namespace

hipError_t launch_kos_multi_tags(const uint4 *seed2, const uint4 *result, const uint8_t *choice, const uint4 *cv,
                                 const uint8_t *bcv, size_t S, size_t per, uint4 *tags_out, const uint32_t *te0,
                                 hipStream_t s) {
    if (S == 0) return hipSuccess;
    if (kos_multi_wave_team(per, kKosMultiWaveMax))
        return launch(k_kos_multi<false, false>, false, seed2, result, choice, cv, bcv, nullptr, nullptr, S, per, tags_out,
                      nullptr, nullptr, te0, s);
    return launch(k_kos_multi<false, true>, true, seed2, result, choice, cv, bcv, nullptr, nullptr, S, per, tags_out, nullptr,
                  nullptr, te0, s);
}

hipError_t launch_kos_multi_check(const uint4 *seed2, const uint4 *result, const uint4 *cv, const uint4 *delta,
                                  const uint4 *tags, size_t S, size_t per, uint8_t *ok, unsigned long long *status,
                                  const uint32_t *te0, hipStream_t s) {
    if (S == 0) return hipSuccess;
    if (kos_multi_wave_team(per, kKosMultiWaveMax))
        return launch(k_kos_multi<true, false>, false, seed2, result, nullptr, cv, nullptr, delta, tags, S, per, nullptr, ok,
                      status, te0, s);
    return launch(k_kos_multi<true, true>, true, seed2, result, nullptr, cv, nullptr, delta, tags, S, per, nullptr, ok, status,
                  te0, s);
}

}  // namespace gc
