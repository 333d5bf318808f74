// iknp_multi_bits_kernels.hip — bit-COT for S sessions of equal length in one launch per role (gc_iknp_multi_*_bits*) and the
// local folds of a GMW triple batch over S peers (gc_gmw_triples_multi_*): byte for byte what gc_iknp_receive_bits /
// gc_iknp_send_bits give on each session alone.  Indices: iknp_multi_bits.h.
//
// The result of bit-COT is bit 0 of every label, and that is column 0 of the g0 stream untransposed (iknp.go:287-304,
// :601-611), so neither kernel transposes or writes a label.
//
// k_iknp_multi_recv_bits is the receiver of k_iknp_multi (iknp_multi_kernels.hip) — the same items, lanes and keystream,
// since u needs all 128 columns of both streams — less the transposing wave, the label store and two of the three barriers
// of a step.  The g1 lanes hand their quarters to the g0 lanes through LDS; with one barrier a step the g1 lanes may run
// one step ahead, so the hand-over buffers alternate between two sets.  The choice bytes are read from the caller's u64
// words (whole words only), and the column-0 lane of the g0 stream stores its bytes into `result` as masked u64 words.
// LDS: 64 KiB table | 2 sets x 4 items x 8 KiB.
//
// k_iknp_multi_send_bits computes column 0 only.  The other 127 column streams just advance, which is the handle's `pos`.
// A lane makes 16 result bytes: one AES block on a block boundary, two with the byte shift off it.
#include <algorithm>

#include "iknp_multi_bits.h"
#include "iknp_multi_stream.h"
#include "kernels.h"

namespace gc {

namespace {

constexpr int IKT = kIknpThreads;
constexpr uint32_t kHandBuf = 4 * 128 * 16;  // one item's g1 bytes: [quarter][column] x 16 bytes, conflict-free both ways

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// keys: the handle's label pairs [S][128][2]; choices / u_out / result: the arrays of the call (iknp_multi_bits.h)
template <bool MISALIGNED, bool HI0>
__global__ __launch_bounds__(IKT) void k_iknp_multi_recv_bits(const uint4 *__restrict__ keys, uint64_t pos0, uint64_t S,
                                                              uint64_t per, const uint64_t *__restrict__ choices,
                                                              uint64_t stride, uint8_t *__restrict__ u_out,
                                                              uint64_t *__restrict__ result,
                                                              const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    constexpr uint32_t NCH = kIknpRecvChunks;  // items per workgroup step
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off();
    const uint32_t slice = threadIdx.x >> 7, col = threadIdx.x & 127u;
    const uint32_t cig = slice & 3u;      // item inside the step
    const uint32_t stream = slice >> 2;   // 0 = g0 (t), 1 = g1
    const uint32_t sh = (uint32_t)(pos0 & 15u);
    const uint64_t items = iknp_multi_items(S, per);
    const uint64_t steps = iknp_multi_steps(items, NCH);
    uint32_t set = 0;

    for (uint64_t step = blockIdx.x; step < steps; step += gridDim.x, set ^= 1u) {
        const uint64_t it = step * NCH + cig;
        const bool valid = it < items;  // uniform over the two waves of a slice
        const IknpMultiItem m = iknp_multi_item(valid ? it : 0, per, pos0);
        const uint32_t byte_rows = valid ? m.byte_rows : 0;
        const uint32_t nq = (byte_rows + 15u) / 16u;  // quarters of the column that hold bytes
        // a column whose length is a multiple of 16 starts 16-byte aligned (col * byte_rows behind an offset that is a
        // multiple of 128) and goes as whole quarters
        const bool whole = (byte_rows & 15u) == 0;
        uint32_t t[16];
        if (valid) {
            const uint4 kl = keys[(m.session * 128 + col) * 2 + stream];
            const uint32_t key[4] = {kl.y, kl.x, kl.w, kl.z};  // BE(label) (newPrg, iknp.go:622-630)
            column_stream<MISALIGNED, HI0>(m.stream_pos, sh, m.blocks, key, lo0, t);
        }
        const uint32_t hand = kTeDualBytes + (set * NCH + cig) * kHandBuf + col * 16u;
        if (valid && stream == 1) {
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)
                if (q < nq) lds_st4(hand + q * 2048u, make_uint4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]));
        }
        // the only barrier of a step.  The g1 lanes write set `set` again two steps on, behind the next barrier, which the
        // g0 lanes reach with this step's reads done
        __syncthreads();
        if (valid && stream == 0) {
            const IknpBitsItem bi = iknp_bits_item(m, per, stride);
            const uint64_t at = m.u_off + (uint64_t)col * byte_rows;  // column-major message layout (iknp.go:490-499)
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)
                if (q < nq) {
                    // words 2q and 2q + 1 of the item's choices, the same for every column; a word enters only whole
                    const uint64_t b0 = 2 * q < bi.choice_words ? choices[bi.choice_word + 2 * q] : 0;
                    const uint64_t b1 = 2 * q + 1 < bi.choice_words ? choices[bi.choice_word + 2 * q + 1] : 0;
                    const uint4 t1 = lds_ld4(hand + q * 2048u);
                    store_quarter(u_out + at, byte_rows, q,
                                  make_uint4(t[4 * q] ^ t1.x ^ (uint32_t)b0, t[4 * q + 1] ^ t1.y ^ (uint32_t)(b0 >> 32),
                                             t[4 * q + 2] ^ t1.z ^ (uint32_t)b1, t[4 * q + 3] ^ t1.w ^ (uint32_t)(b1 >> 32)),
                                  whole);
                }
            if (col == 0) {  // labelsBuf[row].Bit(0) is bit `row` of column 0 (iknp.go:601-611)
#pragma unroll
                for (uint32_t w = 0; w < 8; w++)
                    if (w < bi.result_words)
                        result[bi.result_word + w] = u64_of(t[2 * w], t[2 * w + 1]) & iknp_bits_word_mask(per, 8 * m.chunk + w);
            }
        }
    }
}

// keys: the handle's k0 [S][128]; delta: [S] uint4; u_in with u_session / u_chunk bytes between sessions / chunks
template <bool HI0>
__global__ __launch_bounds__(kIknpBitsSendThreads) void k_iknp_multi_send_bits(
    const uint4 *__restrict__ keys, const uint32_t *__restrict__ delta, uint64_t pos0, uint64_t S, uint64_t per,
    const uint8_t *__restrict__ u_in, uint64_t u_session, uint64_t u_chunk, uint64_t *__restrict__ result,
    const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off();
    const uint32_t sh = (uint32_t)(pos0 & 15u), ws = sh >> 2, bs = sh & 3u;  // the shift: dwords and bytes
    const uint64_t lanes = iknp_bits_send_lanes(S, per), W = iknp_bits_words(per);
    for (uint64_t g = (uint64_t)blockIdx.x * kIknpBitsSendThreads + threadIdx.x; g < lanes;
         g += (uint64_t)gridDim.x * kIknpBitsSendThreads) {
        const IknpBitsLane n = iknp_bits_send_lane(g, per, pos0, u_session, u_chunk);
        const uint4 kl = keys[n.session * 128];  // column 0
        const uint32_t key[4] = {kl.y, kl.x, kl.w, kl.z};
        const uint64_t j0 = n.stream_pos >> 4;
        uint32_t c0[4], c1[4] = {0u, 0u, 0u, 0u};
        stream_block<HI0>(key, j0, lo0, c0);
        if (n.blocks > 1) stream_block<HI0>(key, j0 + 1, lo0, c1);
        // bytes [sh, sh + 16) of the pair
        const uint32_t c[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
        uint32_t d[5], o[4];
#pragma unroll
        for (int i = 0; i < 5; i++) d[i] = ws == 0 ? c[i] : ws == 1 ? c[i + 1] : ws == 2 ? c[i + 2] : c[i + 3];
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], bs);
        if (delta[n.session * 4] & 1u) {  // Delta.Bit(0): bit 0 of D0
            const uint8_t *src = u_in + n.u_off;
            if (n.nbytes == 16) {
                const uint4 u = *(const uint4 *)src;
                o[0] ^= u.x, o[1] ^= u.y, o[2] ^= u.z, o[3] ^= u.w;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 4; i++)
                    if (4 * i < n.nbytes) o[i] ^= load_u8s(src + 4 * i, n.nbytes - 4 * i < 4 ? n.nbytes - 4 * i : 4);
            }
        }
        uint64_t *dst = result + n.session * W + n.word;
        dst[0] = u64_of(o[0], o[1]) & iknp_bits_word_mask(per, n.word);
        if (n.words > 1) dst[1] = u64_of(o[2], o[3]) & iknp_bits_word_mask(per, n.word + 1);
    }
}

// ---- the local words of tripleBatch for S peers at once (triples.go:340-349, 362-364, 387-389) ----

// u[s][i] = a[i] ^ (Delta_s.Bit(0) ? ~0 : 0)
__global__ __launch_bounds__(kGmwMultiFoldThreads) void k_gmw_multi_sender_u(const uint32_t *__restrict__ delta,
                                                                             const uint64_t *__restrict__ a,
                                                                             uint64_t *__restrict__ u, uint64_t S, uint64_t words) {
    const uint64_t n = S * words, stride = (uint64_t)gridDim.x * kGmwMultiFoldThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kGmwMultiFoldThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t s = i / words;
        u[i] = a[i - s * words] ^ ((delta[4 * s] & 1u) ? ~0ull : 0ull);
    }
}

// SENDER: c[i] ^= XOR_s (x[s][i] ^ (y[s][i] & z[s][i]))   (x = s, y = u, z = v);  else c[i] ^= XOR_s x[s][i]   (x = r)
template <bool SENDER>
__global__ __launch_bounds__(kGmwMultiFoldThreads) void k_gmw_multi_fold(const uint64_t *__restrict__ x,
                                                                         const uint64_t *__restrict__ y,
                                                                         const uint64_t *__restrict__ z, uint64_t *__restrict__ c,
                                                                         uint64_t S, uint64_t words) {
    const uint64_t stride = (uint64_t)gridDim.x * kGmwMultiFoldThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kGmwMultiFoldThreads + threadIdx.x; i < words; i += stride) {
        uint64_t acc = c[i];
        for (uint64_t s = 0; s < S; s++) {
            const uint64_t at = s * words + i;
            acc ^= SENDER ? x[at] ^ (y[at] & z[at]) : x[at];
        }
        c[i] = acc;
    }
}

unsigned fold_grid(uint64_t n) {
    return (unsigned)std::min<uint64_t>((n + kGmwMultiFoldThreads - 1) / kGmwMultiFoldThreads, kGmwMultiFoldGrid);
}

}  // namespace

hipError_t launch_iknp_multi_recv_bits(const uint4 *keys, uint64_t pos0, size_t S, size_t per, const uint64_t *choices,
                                       size_t stride, uint8_t *u_out, uint64_t *result, const uint32_t *te0, hipStream_t s) {
    if (S == 0 || per == 0) return hipSuccess;
    const uint64_t steps = iknp_multi_steps(iknp_multi_items(S, per), kIknpRecvChunks);
    const unsigned grid = (unsigned)std::min<uint64_t>(steps, kIknpMultiGrid);
    const size_t lds = kTeDualBytes + 2 * (size_t)kIknpRecvChunks * kHandBuf;
    const bool mis = (pos0 & 15u) != 0, hi0 = iknp_counters_fit_32(pos0, iknp_multi_chunks(per));
    auto go = [&](auto kern) {
        return launch_with_lds(kern, grid, IKT, lds, s, keys, pos0, (uint64_t)S, (uint64_t)per, choices, (uint64_t)stride, u_out,
                               result, te0);
    };
    if (mis) return hi0 ? go(k_iknp_multi_recv_bits<true, true>) : go(k_iknp_multi_recv_bits<true, false>);
    return hi0 ? go(k_iknp_multi_recv_bits<false, true>) : go(k_iknp_multi_recv_bits<false, false>);
}

hipError_t launch_iknp_multi_send_bits(const uint4 *keys, const uint4 *delta, uint64_t pos0, size_t S, size_t per,
                                       const uint8_t *u_in, size_t u_session, size_t u_chunk, uint64_t *result,
                                       const uint32_t *te0, hipStream_t s) {
    if (S == 0 || per == 0) return hipSuccess;
    const uint64_t lanes = iknp_bits_send_lanes(S, per);
    const unsigned grid = (unsigned)std::min<uint64_t>((lanes + kIknpBitsSendThreads - 1) / kIknpBitsSendThreads, kIknpBitsSendGrid);
    auto go = [&](auto kern) {
        return launch_with_lds(kern, grid, kIknpBitsSendThreads, kTeDualBytes, s, keys, (const uint32_t *)delta, pos0, (uint64_t)S,
                               (uint64_t)per, u_in, (uint64_t)u_session, (uint64_t)u_chunk, result, te0);
    };
    return iknp_counters_fit_32(pos0, iknp_multi_chunks(per)) ? go(k_iknp_multi_send_bits<true>) : go(k_iknp_multi_send_bits<false>);
}

hipError_t launch_gmw_multi_sender_u(const uint4 *delta, const uint64_t *a, uint64_t *u, size_t S, size_t words, hipStream_t s) {
    if (S == 0 || words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gmw_multi_sender_u, dim3(fold_grid((uint64_t)S * words)), dim3(kGmwMultiFoldThreads), 0, s,
                       (const uint32_t *)delta, a, u, (uint64_t)S, (uint64_t)words);
    return hipGetLastError();
}

hipError_t launch_gmw_multi_sender_fold(const uint64_t *sv, const uint64_t *u, const uint64_t *v, uint64_t *c, size_t S,
                                        size_t words, hipStream_t s) {
    if (S == 0 || words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gmw_multi_fold<true>, dim3(fold_grid(words)), dim3(kGmwMultiFoldThreads), 0, s, sv, u, v, c,
                       (uint64_t)S, (uint64_t)words);
    return hipGetLastError();
}

hipError_t launch_gmw_multi_receiver_fold(const uint64_t *r, uint64_t *c, size_t S, size_t words, hipStream_t s) {
    if (S == 0 || words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gmw_multi_fold<false>, dim3(fold_grid(words)), dim3(kGmwMultiFoldThreads), 0, s, r,
                       (const uint64_t *)nullptr, (const uint64_t *)nullptr, c, (uint64_t)S, (uint64_t)words);
    return hipGetLastError();
}

}  // namespace gc
