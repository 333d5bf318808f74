// iknp_multi_kernels.hip — the IKNP OT extension and the COT pad loops for S sessions of equal length in one launch each
// (gc_iknp_multi_*, gc_cot_multi_*): byte for byte what k_iknp_fused / k_cot_dual give on each session alone.
//
// k_iknp_multi has the shape of k_iknp_fused (iknp_fused_kernels.hip): persistent workgroups of kIknpThreads lanes around
// the perm-addressed dual table, lane = (slice, column), a slice of 128 lanes produces the column bytes of one chunk, the
// chunk goes through a swizzled buffer in LDS, one wave transposes it (createLabels, iknp.go:647-683) and stores the labels
// coalesced.  Where that kernel walks the chunks of one session, this one walks (session, chunk) ITEMS (iknp_multi.h), so:
//   * the column key is per item: 16 bytes per lane from the handle's copy of the base labels, expanded in the lane by the
//     on-the-fly schedule of aes_otf_dual.h (key = BE(label), words {y, x, w, z}).  No round keys in LDS: a session of 128
//     OTs would load 22 KiB of them to encrypt 2 KiB;
//   * a lane encrypts the blocks its item needs, ceil((pos % 16 + byte_rows) / 16): ONE for a session of 128 OTs at
//     position 0, where a full chunk takes four (five off a block boundary).  The count is the same for every item but the
//     last chunk of a session, and uniform over the two waves of a slice;
//   * quarters of the chunk buffer and dword rows of the transpose that hold no OT are skipped.
// LDS: 64 KiB table | 8 (sender) or 4 (receiver: 4 items x 2 streams) chunk buffers of 8 448 bytes.
//
// k_cot_multi is k_cot_dual's body (ot_kernels.hip) with the seed and delta of the lane's session read from arrays and the
// MITCCRH key index restarting at 0 in every session; a wave may span sessions.
#include <algorithm>

#include "cot_lane.h"
#include "iknp_multi.h"
#include "iknp_multi_stream.h"
#include "kernels.h"

namespace gc {

namespace {

constexpr int IKT = kIknpThreads;

// keys: the handle's base labels, [S][128] uint4 (sender: k0) or [S][128][2] (receiver: l0, l1 of every pair);
// delta: [S] uint4 (sender).  choice / u_in / u_out / labels: the arrays of the call, laid out as iknp_multi.h says.
template <bool RECV, bool MISALIGNED, bool HI0>
__global__ __launch_bounds__(IKT) void k_iknp_multi(const uint4 *__restrict__ keys, const uint32_t *__restrict__ delta,
                                                    uint64_t pos0, uint64_t S, uint64_t per,
                                                    const uint8_t *__restrict__ choice, const uint8_t *__restrict__ u_in,
                                                    uint8_t *__restrict__ u_out, uint4 *__restrict__ labels,
                                                    const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    constexpr uint32_t NCH = RECV ? kIknpRecvChunks : kIknpSendChunks;  // items per workgroup step
    constexpr uint32_t kBuf = kTeDualBytes;                             // byte address of chunk buffer 0
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t slice = wave >> 1, col = threadIdx.x & 127u;
    const uint32_t cig = RECV ? (slice & 3u) : slice;  // item inside the step
    const uint32_t stream = RECV ? (slice >> 2) : 0u;  // receiver: 0 = g0 (t), 1 = g1
    const uint32_t bufaddr = kBuf + cig * kChunkBuf;
    const uint32_t sh = (uint32_t)(pos0 & 15u);
    const uint64_t items = iknp_multi_items(S, per);
    const uint64_t steps = iknp_multi_steps(items, NCH);

    for (uint64_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const uint64_t it = step * NCH + cig;
        const bool valid = it < items;
        const IknpMultiItem m = iknp_multi_item(valid ? it : 0, per, pos0);
        const uint32_t byte_rows = valid ? m.byte_rows : 0;
        const uint32_t nq = (byte_rows + 15u) / 16u;  // quarters of the column that hold bytes
        // a column whose length is a multiple of 16 starts 16-byte aligned (col * byte_rows behind an offset that is a
        // multiple of 128) and goes as whole quarters
        const bool whole = (byte_rows & 15u) == 0;
        uint32_t t[16];
        if (valid) {
            const uint4 kl = keys[(m.session * 128 + col) * (RECV ? 2 : 1) + stream];
            const uint32_t key[4] = {kl.y, kl.x, kl.w, kl.z};  // BE(label) (newPrg, iknp.go:622-630)
            column_stream<MISALIGNED, HI0>(m.stream_pos, sh, m.blocks, key, lo0, t);
        }
        const uint64_t at = m.u_off + (uint64_t)col * byte_rows;  // column-major message layout (iknp.go:490-499)
        if (RECV) {
            if (valid && stream == 1) chunk_put_quarters(bufaddr, col, t, nq);
            __syncthreads();
            if (valid && stream == 0) {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (q < nq) {
                        // the choice bytes, the same for every column.  Whole quarters: the contract of the call (gcengine.h)
                        // is that an item's 64 bytes exist whatever its length is; padding bytes fall behind byte_rows and
                        // are not stored
                        const uint4 b = ((const uint4 *)(choice + m.choice_off))[q];
                        const uint4 t1 = lds_ld4(bufaddr + 4 * chunk_pos(col, 4 * q));
                        store_quarter(u_out + at, byte_rows, q,
                                      make_uint4(t[4 * q] ^ t1.x ^ b.x, t[4 * q + 1] ^ t1.y ^ b.y, t[4 * q + 2] ^ t1.z ^ b.z,
                                                 t[4 * q + 3] ^ t1.w ^ b.w),
                                      whole);
                    }
            }
        } else if (valid) {
            // Delta.Bit(i): bit i of D0 for i < 64 (label.go:129-141) — D0 is the low limb
            const uint32_t word = delta[m.session * 4 + (col >> 5)];
            if ((word >> (col & 31u)) & 1u) {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (q < nq) {
                        const uint4 u = load_quarter(u_in + at, byte_rows, q, whole);
                        t[4 * q] ^= u.x, t[4 * q + 1] ^= u.y, t[4 * q + 2] ^= u.z, t[4 * q + 3] ^= u.w;
                    }
            }
        }
        if (valid && stream == 0) chunk_put_quarters(bufaddr, col, t, nq);
        __syncthreads();
        // createLabels: wave w transposes item w of the step.  A dword row without an OT was not written above and is not
        // read there.
        if (wave < NCH && step * NCH + wave < items) {
            const IknpMultiItem wm = iknp_multi_item(step * NCH + wave, per, pos0);
            chunk_create_labels(kBuf + wave * kChunkBuf, lane, wm.rows, labels + wm.label_off);
        }
        __syncthreads();
    }
}

// SEND: COT.Send pads   (cot.go:160-181): out[2i] = H_j(x_i) ^ L0_i, out[2i+1] = H_j(x_i ^ delta_s) ^ L1_i
// else: COT.Receive     (cot.go:203-232): out[i] = data[2i + flag_i] ^ H_j(out[i])         (data = the 2n labels received)
// for OT i = s * per + j of n = S * per, H_j under key BE(Label{j, 0} ^ seed_s)
template <bool SEND>
__global__ __launch_bounds__(kCotThreads) void k_cot_multi(const uint4 *__restrict__ seeds, const uint4 *__restrict__ deltas,
                                                           const uint4 *__restrict__ data, const uint4 *__restrict__ wires,
                                                           const uint8_t *__restrict__ flags, uint4 *__restrict__ out,
                                                           uint64_t n, uint64_t per, const uint32_t *__restrict__ g_te0) {
    extern __shared__ uint4 smem[];
    constexpr int NB = SEND ? 2 : 1;
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off();
    const bool small = n <= 0xffffffffull;  // launch-uniform: the session of an OT by a 32-bit division
    for (uint64_t i = (uint64_t)blockIdx.x * kCotThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kCotThreads) {
        const uint64_t s = small ? (uint64_t)((uint32_t)i / (uint32_t)per) : i / per;
        uint32_t k[4];
        mitccrh_key(seeds[s], i - s * per, k);
        uint4 x[NB], pad[NB];
        if (SEND) {
            x[0] = data[i];
            x[NB - 1] = lxor(x[0], deltas[s]);
            pad[0] = wires[2 * i];
            pad[NB - 1] = wires[2 * i + 1];
        } else {
            x[0] = out[i];
            pad[0] = data[2 * i + (flags[i] ? 1 : 0)];
        }
        uint4 h[NB];
        mitccrh_pads<NB>(x, k, lo0, h);
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (SEND) out[2 * i + b] = lxor(h[b], pad[b]);
            else out[i] = lxor(h[b], pad[b]);
        }
    }
}

}  // namespace

hipError_t launch_iknp_multi(bool recv, const uint4 *keys, const uint4 *delta, uint64_t pos0, size_t S, size_t per,
                             const uint8_t *choice, const uint8_t *u_in, uint8_t *u_out, uint4 *labels, const uint32_t *te0,
                             hipStream_t s) {
    if (S == 0 || per == 0) return hipSuccess;
    const uint32_t nch = recv ? kIknpRecvChunks : kIknpSendChunks;
    const uint64_t steps = iknp_multi_steps(iknp_multi_items(S, per), nch);
    const unsigned grid = (unsigned)std::min<uint64_t>(steps, kIknpMultiGrid);
    const size_t lds = kTeDualBytes + (size_t)nch * kChunkBuf;
    const bool mis = (pos0 & 15u) != 0;
    const bool hi0 = iknp_counters_fit_32(pos0, iknp_multi_chunks(per));
    auto go = [&](auto kern) {
        return launch_with_lds(kern, grid, IKT, lds, s, keys, (const uint32_t *)delta, pos0, (uint64_t)S, (uint64_t)per, choice,
                               u_in, u_out, labels, te0);
    };
    if (recv) {
        if (mis) return hi0 ? go(k_iknp_multi<true, true, true>) : go(k_iknp_multi<true, true, false>);
        return hi0 ? go(k_iknp_multi<true, false, true>) : go(k_iknp_multi<true, false, false>);
    }
    if (mis) return hi0 ? go(k_iknp_multi<false, true, true>) : go(k_iknp_multi<false, true, false>);
    return hi0 ? go(k_iknp_multi<false, false, true>) : go(k_iknp_multi<false, false, false>);
}

template <typename K>
static hipError_t launch_cot_multi(K kern, const uint4 *seeds, const uint4 *deltas, const uint4 *data, const uint4 *wires,
                                   const uint8_t *flags, uint4 *out, size_t n, size_t per, const uint32_t *te0, hipStream_t s) {
    const unsigned grid = (unsigned)std::min<size_t>(kCotGrid, (n + kCotThreads - 1) / kCotThreads);
    return launch_with_lds(kern, grid, kCotThreads, kTeDualBytes, s, seeds, deltas, data, wires, flags, out, (uint64_t)n,
                           (uint64_t)per, te0);
}

hipError_t launch_cot_multi_send(const uint4 *seeds, const uint4 *deltas, const uint4 *data, const uint4 *wires, size_t S,
                                 size_t per, uint4 *out, const uint32_t *te0, hipStream_t s) {
    if (S == 0 || per == 0) return hipSuccess;
    return launch_cot_multi(k_cot_multi<true>, seeds, deltas, data, wires, nullptr, out, S * per, per, te0, s);
}

hipError_t launch_cot_multi_recv(const uint4 *seeds, const uint8_t *flags, const uint4 *sent, uint4 *result, size_t S,
                                 size_t per, const uint32_t *te0, hipStream_t s) {
    if (S == 0 || per == 0) return hipSuccess;
    return launch_cot_multi(k_cot_multi<false>, seeds, nullptr, sent, nullptr, flags, result, S * per, per, te0, s);
}

}  // namespace gc
