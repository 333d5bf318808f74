// yao_kernels.hip — the kernels of the gc_yao_* calls (yao.h): circuit.Garbler's and circuit.Evaluator's
// messages for S sessions, built and read on the device.
//
// M1 out and M1 in are the hot path: per session 4 + keylen + gc_tables_wire_bytes() + 16 ng bytes next to a keyed pass that
// takes under a millisecond.  A workgroup owns piece p of the message (yao_skel.h) for a TILE of consecutive sessions and
// holds the tile's pieces in LDS, one stage per session.  Everything in M1 lies on a multiple of 4 bytes and a slot on a
// multiple of 16, so a stage is filled and read in 32-bit words and moves to and from the slot in whole 16-byte lines; only
// the message's last 4, 8 or 12 bytes move as words.  A slot's padding is never written.
//   out: the skeleton's lines to every stage (one global read, `tile` LDS writes), then the words that differ per session on
//        top — key, table rows, own labels — then the stages to the slots, a wave writing 1 KiB runs of one session.
//   in:  the slots' lines to the stages, then rows, key and labels from the stages to their arrays, and every word the
//        skeleton fixes compared with it: the lowest failing check per session by atomicMin in LDS, and one global atomicMin
//        per BAD session and piece (an honest call has none).
// The table rows of a tile are read and written as contiguous runs: Layout::at is [tile][row][instance], so with q =
// min(instances per layout tile, sessions per workgroup) the rows r0 .. r1 of q sessions are (r1 - r0) q labels in a row.  At
// fewer than 512 sessions the layout's tile is one instance and a session's rows are simply consecutive.
#include "launch_dispatch.h"
#include "yao.h"

namespace gc {

namespace {

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
// ot.Label <-> its 16 big-endian bytes loaded as a uint4 of little-endian words (its own inverse)
__device__ __forceinline__ uint4 label_be(uint4 v) { return make_uint4(bswap32(v.y), bswap32(v.x), bswap32(v.w), bswap32(v.z)); }
__device__ __forceinline__ uint4 lxor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ bool leq4(uint4 a, uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// the geometry of piece p in a workgroup
struct Piece {
    uint32_t lo, hi;   // bytes of the message
    uint32_t nw;       // words
    uint32_t r0, r1;   // rows with a byte in it lie in [r0, r1), r1 one too many where row r1 - 1 begins at hi
};
__device__ __forceinline__ Piece piece_of(const YaoDev &d, uint32_t p) {
    Piece c;
    c.lo = p * d.piece_bytes;
    c.hi = min(c.lo + d.piece_bytes, d.len1);
    c.nw = (c.hi - c.lo) >> 2;
    c.r0 = d.piece_row[p];
    c.r1 = min(d.piece_row[p + 1] + 1u, d.nrows);
    return c;
}

// the four words of a 16-byte field at byte `off` of the message into / out of a stage that holds [lo, lo + 4 nw): the words
// of the field that lie in the piece, w0 = (off - lo) / 4 may be negative
__device__ __forceinline__ void field_put(uint32_t *stage, int w0, uint32_t nw, uint4 v) {
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (w0 + c >= 0 && (uint32_t)(w0 + c) < nw) stage[w0 + c] = w4[c];
}

// labels [i_lo, i_hi) of the own-label section have a byte in [lo, hi) (out), or begin there (in)
__device__ __forceinline__ void label_range(const YaoDev &d, uint32_t lo, uint32_t hi, bool begins, uint32_t *i_lo, uint32_t *i_hi) {
    const uint32_t a = d.at_labels;
    *i_lo = lo > a ? (lo - a + (begins ? 15u : 0u)) >> 4 : 0u;
    *i_hi = hi > a ? min(d.ng, (hi - a + 15u) >> 4) : 0u;
}

template <uint32_t KLOG>
__global__ __launch_bounds__(kYaoThreads) void k_yao_m1_out(YaoDev d, const uint4 *__restrict__ T, Layout lt,
                                                            const uint4 *__restrict__ W, Layout lw, const uint4 *__restrict__ R,
                                                            const uint32_t *__restrict__ keys, const uint8_t *__restrict__ bits,
                                                            uint8_t *__restrict__ m1, size_t stride1, uint32_t S) {
    constexpr uint32_t K = 1u << KLOG;
    extern __shared__ __attribute__((aligned(16))) uint4 stage16[];
    uint32_t *stage32 = (uint32_t *)stage16;
    const uint32_t tid = threadIdx.x, s0 = blockIdx.x << KLOG;
    const uint32_t L16 = d.piece_bytes / 16 + 1, L32 = 4 * L16;  // a stage in lines and in words
    const uint32_t live = min(K, S - s0);                        // sessions of the tile
    const uint32_t ql = min(lt.ti_log2, KLOG), qw = min(lw.ti_log2, KLOG);
    for (uint32_t p = blockIdx.y; p < d.npieces; p += gridDim.y) {
        const Piece c = piece_of(d, p);
        // the skeleton of the piece, the same for every session
        for (uint32_t l = tid; 4 * l < c.nw; l += kYaoThreads) {
            const uint4 v = d.skel[c.lo / 16 + l];
#pragma unroll
            for (uint32_t j = 0; j < K; j++) stage16[j * L16 + l] = v;
        }
        __syncthreads();
        // the key: bytes 4 .. 4 + keylen, all in piece 0 (a piece is at least 64 bytes)
        if (p == 0) {
            const uint32_t kw = d.keylen / 4;
            for (uint32_t e = tid; e < live * kw; e += kYaoThreads) {
                const uint32_t j = e / kw, w = e % kw;
                stage32[j * L32 + 1 + w] = keys[(size_t)(s0 + j) * kw + w];
            }
        }
        // the table rows: runs of q sessions
        for (uint32_t j0 = 0; j0 < live; j0 += 1u << ql)
            for (uint32_t e = tid; e < (c.r1 - c.r0) << ql; e += kYaoThreads) {
                const uint32_t r = c.r0 + (e >> ql), j = j0 + (e & ((1u << ql) - 1u));
                const uint32_t off = d.row_off[r];
                if (off >= c.hi || j >= live) continue;
                field_put(stage32 + j * L32, ((int)off - (int)c.lo) >> 2, c.nw, label_be(T[lt.at(r, s0 + j)]));
            }
        // the garbler's own labels: LabelForBit of input wire i (garbler.go:86-91)
        uint32_t i_lo, i_hi;
        label_range(d, c.lo, c.hi, false, &i_lo, &i_hi);
        if (i_hi > i_lo)
            for (uint32_t j0 = 0; j0 < live; j0 += 1u << qw)
                for (uint32_t e = tid; e < (i_hi - i_lo) << qw; e += kYaoThreads) {
                    const uint32_t i = i_lo + (e >> qw), j = j0 + (e & ((1u << qw) - 1u));
                    if (j >= live) continue;
                    const uint32_t s = s0 + j;
                    uint4 v = W[lw.at(i, s)];
                    if (bits[(size_t)s * d.ng + i]) v = lxor4(v, R[s]);
                    field_put(stage32 + j * L32, ((int)(d.at_labels + 16 * i) - (int)c.lo) >> 2, c.nw, label_be(v));
                }
        __syncthreads();
        // the stages to the slots
        const uint32_t lines = c.nw >> 2, tail = c.nw & 3u;
        for (uint32_t j = 0; j < live; j++) {
            uint4 *dst = (uint4 *)(m1 + (size_t)(s0 + j) * stride1 + c.lo);
            for (uint32_t l = tid; l < lines; l += kYaoThreads) dst[l] = stage16[j * L16 + l];
            if (tid < tail) ((uint32_t *)(dst + lines))[tid] = stage32[j * L32 + 4 * lines + tid];
        }
        __syncthreads();
    }
}

template <uint32_t KLOG>
__global__ __launch_bounds__(kYaoThreads) void k_yao_m1_in(YaoDev d, uint4 *__restrict__ T, Layout lt, uint4 *__restrict__ W,
                                                           Layout lw, uint32_t *__restrict__ keys_out,
                                                           const uint8_t *__restrict__ m1, size_t stride1, uint32_t S,
                                                           uint32_t *__restrict__ badidx) {
    constexpr uint32_t K = 1u << KLOG;
    extern __shared__ __attribute__((aligned(16))) uint4 stage16[];
    uint32_t *stage32 = (uint32_t *)stage16;
    const uint32_t tid = threadIdx.x, s0 = blockIdx.x << KLOG;
    const uint32_t L16 = d.piece_bytes / 16 + 1, L32 = 4 * L16;
    uint32_t *bad = stage32 + K * L32;  // [K]
    const uint32_t live = min(K, S - s0);
    const uint32_t ql = min(lt.ti_log2, KLOG), qw = min(lw.ti_log2, KLOG);
    const uint32_t *skel32 = (const uint32_t *)d.skel;
    for (uint32_t p = blockIdx.y; p < d.npieces; p += gridDim.y) {
        const Piece c = piece_of(d, p);
        // the piece and the up to 12 bytes by which a field that begins in it reaches beyond: whole lines of the slot (the
        // last line of a message may end in the slot's padding, which is read and not used)
        const uint32_t ext = min(c.hi + 12u, d.len1) - c.lo, lines = (ext + 15u) >> 4;
        if (tid < K) bad[tid] = 0xffffffffu;
        for (uint32_t j = 0; j < live; j++) {
            const uint4 *src = (const uint4 *)(m1 + (size_t)(s0 + j) * stride1 + c.lo);
            for (uint32_t l = tid; l < lines; l += kYaoThreads) stage16[j * L16 + l] = src[l];
        }
        __syncthreads();
        if (p == 0) {
            const uint32_t kw = d.keylen / 4;
            for (uint32_t e = tid; e < live * kw; e += kYaoThreads) {
                const uint32_t j = e / kw, w = e % kw;
                keys_out[(size_t)(s0 + j) * kw + w] = stage32[j * L32 + 1 + w];
            }
            // SendData(key)'s length word, then the gate count (evaluator.go:31, :41-48): both in piece 0
            if (tid < live) {
                const uint32_t *st = stage32 + tid * L32;
                if (st[0] != skel32[0]) atomicMin(&bad[tid], kYaoBadKey);
                else if (st[d.at_tables / 4] != skel32[d.at_tables / 4]) atomicMin(&bad[tid], kYaoBadGates);
            }
        }
        // rows that BEGIN in the piece to the table array
        for (uint32_t j0 = 0; j0 < live; j0 += 1u << ql)
            for (uint32_t e = tid; e < (c.r1 - c.r0) << ql; e += kYaoThreads) {
                const uint32_t r = c.r0 + (e >> ql), j = j0 + (e & ((1u << ql) - 1u));
                const uint32_t off = d.row_off[r];
                if (off < c.lo || off >= c.hi || j >= live) continue;
                const uint32_t *q = stage32 + j * L32 + ((off - c.lo) >> 2);
                T[lt.at(r, s0 + j)] = label_be(make_uint4(q[0], q[1], q[2], q[3]));
            }
        // the peer's labels that begin in the piece to input wires 0 .. ng (evaluator.go:71-77)
        uint32_t i_lo, i_hi;
        label_range(d, c.lo, c.hi, true, &i_lo, &i_hi);
        if (i_hi > i_lo)
            for (uint32_t j0 = 0; j0 < live; j0 += 1u << qw)
                for (uint32_t e = tid; e < (i_hi - i_lo) << qw; e += kYaoThreads) {
                    const uint32_t i = i_lo + (e >> qw), j = j0 + (e & ((1u << qw) - 1u));
                    const uint32_t off = d.at_labels + 16 * i;
                    if (off >= c.hi || j >= live) continue;
                    const uint32_t *q = stage32 + j * L32 + ((off - c.lo) >> 2);
                    W[lw.at(i, s0 + j)] = label_be(make_uint4(q[0], q[1], q[2], q[3]));
                }
        // the row words of the piece's gates against the skeleton's: gc_batch_ingest_tables' rule, the lowest gate wins
        const uint32_t g0 = d.piece_gate[p], g1 = d.piece_gate[p + 1];
        for (uint32_t e = tid; e < (g1 - g0) << KLOG; e += kYaoThreads) {
            const uint32_t g = g0 + (e >> KLOG), j = e & (K - 1u);
            if (j >= live) continue;
            const uint32_t off = d.gate_off[g];
            if (stage32[j * L32 + ((off - c.lo) >> 2)] != skel32[off >> 2]) atomicMin(&bad[j], kYaoBadGate0 + g);
        }
        __syncthreads();
        if (tid < live && bad[tid] != 0xffffffffu) atomicMin(&badidx[s0 + tid], bad[tid]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kYaoThreads) void k_yao_m1_verdict(uint32_t S, const uint32_t *__restrict__ badidx,
                                                                uint32_t *__restrict__ verdict, uint32_t *__restrict__ kept) {
    const uint32_t s = blockIdx.x * kYaoThreads + threadIdx.x;
    if (s >= S) return;
    const uint32_t b = badidx[s];
    uint32_t v = 0;
    if (b == kYaoBadKey) v = kYaoKey;
    else if (b == kYaoBadGates) v = kYaoGates;
    else if (b != 0xffffffffu) v = kYaoRows | (b - kYaoBadGate0) << 8;
    verdict[s] = v;
    kept[s] = v;
}

// ---- M2 out: a tile of 16 outputs x 16 sessions, read with the lanes along the sessions and written with them along the
// outputs (the turn of k_sb_select / k_sb_decode): 256 contiguous bytes of a slot per 16 lanes
constexpr uint32_t kM2Tile = 16;
__global__ __launch_bounds__(kYaoThreads) void k_yao_m2_out(uint32_t nout, uint32_t S, const uint4 *__restrict__ W, Layout lw,
                                                            const uint32_t *__restrict__ out_slots,
                                                            const uint32_t *__restrict__ kept, uint8_t *__restrict__ m2,
                                                            size_t stride2, uint32_t *__restrict__ verdict) {
    __shared__ uint4 tile[kM2Tile][kM2Tile + 1];
    const uint32_t a = threadIdx.x / kM2Tile, b = threadIdx.x % kM2Tile;
    const uint32_t s0 = blockIdx.x * kM2Tile;
    for (uint32_t i0 = blockIdx.y * kM2Tile; i0 < nout; i0 += gridDim.y * kM2Tile) {
        if (i0 + a < nout && s0 + b < S) tile[a][b] = W[lw.at(out_slots[i0 + a], s0 + b)];
        __syncthreads();
        if (i0 + b < nout && s0 + a < S) {
            const uint4 v = kept[s0 + a] ? make_uint4(0, 0, 0, 0) : label_be(tile[b][a]);
            ((uint4 *)(m2 + (size_t)(s0 + a) * stride2))[i0 + b] = v;
        }
        __syncthreads();
    }
    if (blockIdx.y == 0 && threadIdx.x < kM2Tile && s0 + threadIdx.x < S) verdict[s0 + threadIdx.x] = kept[s0 + threadIdx.x];
}

// ---- M2 in, M3 out: a wave per session, a lane per output.  The bits of 64 outputs are one ballot, the lowest label that is
// neither L0 nor L1 (BitFromLabel, helpers.go:18-27) the first set bit of another; the message is yao_m3.h's, a lane per byte.
__global__ __launch_bounds__(kYaoThreads) void k_yao_m2_decode(uint32_t nout, uint32_t S, const uint4 *__restrict__ W, Layout lw,
                                                               const uint32_t *__restrict__ out_slots, const uint4 *__restrict__ R,
                                                               const uint8_t *__restrict__ m2, size_t stride2,
                                                               uint8_t *__restrict__ m3, size_t stride3,
                                                               uint32_t *__restrict__ len3, uint8_t *__restrict__ bits_out,
                                                               uint32_t *__restrict__ verdict) {
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * (kYaoThreads / 64) + (threadIdx.x >> 6);
    const bool live = s < S;
    const uint32_t nb8 = yao_m3_bits_bytes(nout);
    uint8_t *bits = bits_out + (size_t)(live ? s : 0) * nb8;
    uint32_t n = 0, first_bad = 0xffffffffu;
    const uint4 r = live ? R[s] : make_uint4(0, 0, 0, 0);
    for (uint32_t i0 = 0; i0 < nout; i0 += 64) {  // (uniform over the workgroup)
        const uint32_t i = i0 + lane;
        bool one = false, neither = false;
        if (live && i < nout) {
            const uint4 lab = label_be(((const uint4 *)(m2 + (size_t)s * stride2))[i]);
            const uint4 l0 = W[lw.at(out_slots[i], s)];
            one = leq4(lab, lxor4(l0, r));
            neither = !one && !leq4(lab, l0);
        }
        const unsigned long long ones = __ballot(one), bads = __ballot(neither);
        if (bads && first_bad == 0xffffffffu) first_bad = i0 + (uint32_t)__builtin_ctzll(bads);
        if (ones) n = i0 / 8 + (71u - (uint32_t)__builtin_clzll(ones)) / 8;  // bytes up to the highest set bit
        if (live && lane < 8 && i0 / 8 + lane < nb8) bits[i0 / 8 + lane] = (uint8_t)(ones >> (8 * lane));
    }
    __syncthreads();  // the bits bytes are read back by other lanes of their wave
    if (!live) return;
    uint8_t *msg = m3 + (size_t)s * stride3;
    if (first_bad != 0xffffffffu) {  // a bad session: zero bits, a zero message over its slot bytes, length 0
        for (uint32_t k = lane; k < nb8; k += 64) bits[k] = 0;
        for (uint32_t k = lane; k < 4 + nb8; k += 64) msg[k] = 0;
        if (lane == 0) len3[s] = 0, verdict[s] = kYaoLabel | first_bad << 8;
        return;
    }
    for (uint32_t k = lane; k < 4 + n; k += 64) msg[k] = yao_m3_byte(bits, n, k);
    if (lane == 0) len3[s] = 4 + n, verdict[s] = 0;
}

// ---- M3 in: a lane per bits byte
__global__ __launch_bounds__(kYaoThreads) void k_yao_m3_parse(uint32_t nout, uint32_t S, const uint8_t *__restrict__ m3,
                                                              size_t stride3, uint8_t *__restrict__ bits_out,
                                                              uint32_t *__restrict__ verdict) {
    const uint32_t nb8 = yao_m3_bits_bytes(nout);
    const size_t e = (size_t)blockIdx.x * kYaoThreads + threadIdx.x;
    if (e >= (size_t)S * nb8) return;
    const uint32_t s = (uint32_t)(e / nb8), j = (uint32_t)(e % nb8);
    const uint8_t *msg = m3 + (size_t)s * stride3;
    const uint32_t n = yao_m3_read_len(msg);
    const bool fits = 4 + (uint64_t)n <= stride3;
    bits_out[e] = fits ? yao_m3_bits_byte(msg + 4, n, nout, j) : (uint8_t)0;
    if (j == 0) verdict[s] = fits ? 0u : kYaoLength;
}

template <typename F>
hipError_t with_tile(uint32_t tile, F &&f) {
    switch (tile) {
    case 4: return f(std::integral_constant<uint32_t, 2>{});
    case 8: return f(std::integral_constant<uint32_t, 3>{});
    case 16: return f(std::integral_constant<uint32_t, 4>{});
    case 32: return f(std::integral_constant<uint32_t, 5>{});
    case 64: return f(std::integral_constant<uint32_t, 6>{});
    }
    return hipErrorInvalidValue;
}

dim3 m1_grid(const YaoDev &d, uint32_t S) { return dim3((S + d.tile - 1) / d.tile, d.npieces < 65535u ? d.npieces : 65535u); }

}  // namespace

hipError_t launch_yao_m1_out(const YaoDev &d, const uint4 *T, const Layout &lt, const uint4 *W, const Layout &lw, const uint4 *R,
                             const uint32_t *keys, const uint8_t *bits, uint8_t *m1, size_t stride1, uint32_t S, hipStream_t s) {
    return with_tile(d.tile, [&](auto klog) {
        return launch_with_lds(k_yao_m1_out<klog()>, m1_grid(d, S), dim3(kYaoThreads), yao_m1_lds_bytes(d.tile, d.piece_bytes), s, d,
                               T, lt, W, lw, R, keys, bits, m1, stride1, S);
    });
}

hipError_t launch_yao_m1_in(const YaoDev &d, uint4 *T, const Layout &lt, uint4 *W, const Layout &lw, uint32_t *keys_out,
                            const uint8_t *m1, size_t stride1, uint32_t S, uint32_t *badidx, hipStream_t s) {
    return with_tile(d.tile, [&](auto klog) {
        return launch_with_lds(k_yao_m1_in<klog()>, m1_grid(d, S), dim3(kYaoThreads), yao_m1_lds_bytes(d.tile, d.piece_bytes), s, d, T,
                               lt, W, lw, keys_out, m1, stride1, S, badidx);
    });
}

hipError_t launch_yao_m1_verdict(uint32_t S, const uint32_t *badidx, uint32_t *verdict, uint32_t *kept, hipStream_t s) {
    return launch_kernel(k_yao_m1_verdict, dim3((S + kYaoThreads - 1) / kYaoThreads), dim3(kYaoThreads), s, S, badidx, verdict, kept);
}

hipError_t launch_yao_m2_out(const YaoGeom &g, const uint4 *W, const Layout &lw, const uint32_t *out_slots, const uint32_t *kept,
                             uint8_t *m2, size_t stride2, uint32_t *verdict, hipStream_t s) {
    const uint32_t S = (uint32_t)g.S, ny = (g.nout + kM2Tile - 1) / kM2Tile;
    return launch_kernel(k_yao_m2_out, dim3((S + kM2Tile - 1) / kM2Tile, ny < 65535u ? ny : 65535u), dim3(kYaoThreads), s, g.nout, S,
                         W, lw, out_slots, kept, m2, stride2, verdict);
}

hipError_t launch_yao_m2_decode(const YaoGeom &g, const uint4 *W, const Layout &lw, const uint32_t *out_slots, const uint4 *R,
                                const uint8_t *m2, size_t stride2, uint8_t *m3, size_t stride3, uint32_t *len3, uint8_t *bits_out,
                                uint32_t *verdict, hipStream_t s) {
    const uint32_t S = (uint32_t)g.S, per = kYaoThreads / 64;
    return launch_kernel(k_yao_m2_decode, dim3((S + per - 1) / per), dim3(kYaoThreads), s, g.nout, S, W, lw, out_slots, R, m2, stride2,
                         m3, stride3, len3, bits_out, verdict);
}

hipError_t launch_yao_m3_parse(const YaoGeom &g, const uint8_t *m3, size_t stride3, uint8_t *bits_out, uint32_t *verdict,
                               hipStream_t s) {
    const size_t n = g.S * g.bits_bytes();
    return launch_kernel(k_yao_m3_parse, dim3((unsigned)((n + kYaoThreads - 1) / kYaoThreads)), dim3(kYaoThreads), s, g.nout,
                         (uint32_t)g.S, m3, stride3, bits_out, verdict);
}

}  // namespace gc
