// stream_batch_kernels.hip — the kernels around the keyed batch pass of a session-batched streaming step (stream_batch.h):
// the movers between the per-handle wire store [wire id][bstride] and a step's batch, and the serialiser / ingester of the
// stream wire format (circuit/stream_garble.go:391-446) for S byte streams at once.
#include "stream_batch.h"

namespace gcsb {

using gc::Layout;

namespace {

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
// ot.Label <-> its 16 big-endian bytes loaded as a uint4 of little-endian words (its own inverse)
__device__ __forceinline__ uint4 label_be(uint4 v) { return make_uint4(bswap32(v.y), bswap32(v.x), bswap32(v.w), bswap32(v.z)); }

__global__ __launch_bounds__(kThreads) void k_sb_rnd_form(uint4 *__restrict__ rnd, const uint4 *__restrict__ R, uint32_t S,
                                                          uint32_t n1) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)S * n1) return;
    const uint32_t s = (uint32_t)(i / n1), j = (uint32_t)(i % n1);
    rnd[i] = label_be(j == 0 ? R[s] : rnd[i]);
}

__global__ __launch_bounds__(kThreads) void k_sb_init_store(const uint4 *__restrict__ rnd, const uint32_t *__restrict__ ids,
                                                            uint32_t n, uint4 *__restrict__ store, uint32_t bstride,
                                                            uint4 *__restrict__ R, uint32_t S) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)S * (n + 1)) return;
    const uint32_t s = (uint32_t)(i / (n + 1)), j = (uint32_t)(i % (n + 1));
    uint4 v = label_be(rnd[i]);
    if (j == 0) {
        v.y |= 0x80000000u;  // R.SetS(true) (stream_garble.go:60)
        R[s] = v;
    } else if (ids[j - 1] != 0xffffffffu) {
        store[(size_t)ids[j - 1] * bstride + s] = v;
    }
}

// lanes along the sessions: one row of the level-layout store is one coalesced run
__global__ __launch_bounds__(kThreads) void k_sb_rows(const uint4 *__restrict__ src, Layout sl, const uint32_t *__restrict__ srow,
                                                      uint4 *__restrict__ dst, Layout dl, const uint32_t *__restrict__ drow,
                                                      uint32_t n, uint32_t S) {
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    for (uint32_t j = blockIdx.y; j < n; j += gridDim.y) {
        const uint32_t sr = srow ? srow[j] : j, dr = drow ? drow[j] : j;
        if (sr != 0xffffffffu && dr != 0xffffffffu) dst[dl.at(dr, s)] = src[sl.at(sr, s)];
    }
}

// The piece [lo, lo + nb) of one session's bytes lives in LDS at stage + sh, sh = the low four bits of its global address, so
// that everything but the two ragged ends moves as whole, aligned 16-byte lines.  (Byte accesses to global memory with every
// lane in another cache line cost the one-session serialiser 30 us per 4 000 gates: stream_serialise.cpp.)
__device__ __forceinline__ void piece_out(const uint8_t *stage, uint8_t *dst, uint32_t sh, uint32_t nb) {
    const uint32_t head = min(nb, (16u - sh) & 15u);
    const uint32_t body = (nb - head) >> 4, tail = (nb - head) & 15u;
    if (threadIdx.x < head) dst[threadIdx.x] = stage[sh + threadIdx.x];
    const uint4 *src16 = (const uint4 *)(stage + sh + head);
    uint4 *dst16 = (uint4 *)(dst + head);
    for (uint32_t k = threadIdx.x; k < body; k += kThreads) dst16[k] = src16[k];
    if (threadIdx.x < tail) dst[head + 16u * body + threadIdx.x] = stage[sh + head + 16u * body + threadIdx.x];
}
__device__ __forceinline__ void piece_in(uint8_t *stage, const uint8_t *src, uint32_t sh, uint32_t nb) {
    const uint32_t head = min(nb, (16u - sh) & 15u);
    const uint32_t body = (nb - head) >> 4, tail = (nb - head) & 15u;
    if (threadIdx.x < head) stage[sh + threadIdx.x] = src[threadIdx.x];
    uint4 *dst16 = (uint4 *)(stage + sh + head);
    const uint4 *src16 = (const uint4 *)(src + head);
    for (uint32_t k = threadIdx.x; k < body; k += kThreads) dst16[k] = src16[k];
    if (threadIdx.x < tail) stage[sh + head + 16u * body + threadIdx.x] = src[head + 16u * body + threadIdx.x];
}

// room for the piece, its shift, and the 15 bytes by which a row that starts in the piece may reach beyond it
constexpr uint32_t kStageBytes = kPieceBytes + 48;

// session s's rows into the piece [lo, hi) at stage + sh, from row r0 on: every row that has a byte in the piece — a row across
// a piece boundary is written by both pieces, each its own bytes
__device__ __forceinline__ void piece_rows(uint8_t *stage, uint32_t sh, const StepDev &d, const uint4 *__restrict__ T, const Layout &lt,
                                           uint32_t s, uint32_t r0, uint32_t lo, uint32_t hi) {
    for (uint32_t r = r0 + threadIdx.x; r < d.nrows; r += kThreads) {
        const uint32_t off = d.row_off[r];
        if (off >= hi) break;
        const uint4 v = label_be(T[lt.at(r, s)]);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t at = off + k;
            if (at >= lo && at < hi) stage[sh + at - lo] = (uint8_t)(w4[k >> 2] >> (8 * (k & 3)));
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_sb_serialise(StepDev d, const uint4 *__restrict__ T, Layout lt,
                                                           uint8_t *__restrict__ out, size_t stride) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const uint32_t p = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = p * kPieceBytes, hi = min(lo + kPieceBytes, d.nbytes), nb = hi - lo;
    uint8_t *dst = out + (size_t)s * stride + lo;
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15u);
    // the skeleton of the piece (the same for every session), a word per lane
    const uint32_t *sk = (const uint32_t *)(d.skel + lo);
    for (uint32_t k = threadIdx.x; 4 * k < nb; k += kThreads) {
        const uint32_t w = sk[k];
        uint8_t *q = stage + sh + 4 * k;
        q[0] = (uint8_t)w, q[1] = (uint8_t)(w >> 8), q[2] = (uint8_t)(w >> 16), q[3] = (uint8_t)(w >> 24);
    }
    __syncthreads();
    piece_rows(stage, sh, d, T, lt, s, d.piece_row[p], lo, hi);
    __syncthreads();
    piece_out(stage, dst, sh, nb);
}

// Bytes [b0, b1) of the step instead of all of them (a segment of a step that is split over windows: gc_stream_batch_out_create_split),
// at out + s * stride + (byte - b0).  Piece p is [b0 + p * kPieceBytes, ...) of the step, so its first byte is at no particular
// alignment in the skeleton (read as the aligned words around it) and its first row is not piece_row[]'s: it is found between
// the table's entries for the two aligned pieces that the first byte lies between.
__global__ __launch_bounds__(kThreads) void k_sb_serialise_range(StepDev d, const uint4 *__restrict__ T, Layout lt,
                                                                 uint8_t *__restrict__ out, size_t stride, uint32_t b0, uint32_t b1) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const uint32_t p = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = b0 + p * kPieceBytes, hi = min(lo + kPieceBytes, b1), nb = hi - lo;
    uint8_t *dst = out + (size_t)s * stride + (lo - b0);
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15u);
    // the skeleton: the words [lo - a, ...) with the a bytes in front of the piece left out (behind it the stage has room, as above)
    const uint32_t a = lo & 3u;
    const uint32_t *sk = (const uint32_t *)(d.skel + (lo - a));
    for (uint32_t k = threadIdx.x; 4 * k < nb + a; k += kThreads) {
        const uint32_t w = sk[k];
        uint8_t *q = stage + sh + 4 * k - a;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            if (4 * k + j >= a) q[j] = (uint8_t)(w >> (8 * j));
    }
    // the first row that ends behind lo (row_off + 16 > lo; row_off ascends): rows [r0, r1) end in the aligned piece that holds lo,
    // at most 256 of them (16 bytes each), so every lane looks at one and the barrier counts those that end at or before lo — a count per
    // wave in the last 16 bytes of the stage, which a serialiser never fills (the piece ends at or before byte 15 + 4096 + 3)
    static_assert(kThreads == 256 && kStageBytes >= 15 + kPieceBytes + 3 + 16 + 12, "four wave counts behind the piece");
    uint32_t *cnt = (uint32_t *)(stage + kStageBytes - 16);
    const uint32_t ap = lo / kPieceBytes;
    uint32_t r0 = d.piece_row[ap], r1 = ap + 1 < d.npieces ? d.piece_row[ap + 1] : d.nrows;
    if (r1 - r0 <= kThreads) {  // (uniform)
        const uint32_t r = r0 + threadIdx.x;
        const unsigned long long before = __ballot(r < r1 && d.row_off[r] + 16u <= lo);
        if ((threadIdx.x & 63u) == 0) cnt[threadIdx.x >> 6] = (uint32_t)__popcll(before);
        __syncthreads();
        r0 += cnt[0] + cnt[1] + cnt[2] + cnt[3];
    } else {  // (rows that overlap: no step_skeleton makes them; the same answer by bisection)
        while (r0 < r1) {
            const uint32_t mid = (r0 + r1) >> 1;
            if (d.row_off[mid] + 16u > lo) r1 = mid;
            else r0 = mid + 1;
        }
        __syncthreads();
    }
    piece_rows(stage, sh, d, T, lt, s, r0, lo, hi);
    __syncthreads();
    piece_out(stage, dst, sh, nb);
}

__global__ __launch_bounds__(kThreads) void k_sb_ingest(StepDev d, uint4 *__restrict__ T, Layout lt, const uint8_t *__restrict__ in,
                                                        size_t stride, uint32_t *__restrict__ bad) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const uint32_t p = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = p * kPieceBytes, hi = min(lo + kPieceBytes, d.nbytes), nb = hi - lo;
    const uint32_t ext = min(hi + 15u, d.nbytes) - lo;  // with the tail of a row that starts before hi (all inside the block)
    const uint8_t *src = in + (size_t)s * stride + lo;
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15u);
    piece_in(stage, src, sh, ext);
    __syncthreads();
    // rows that START in the piece go to the table array (every offset is the skeleton's: nothing here depends on the bytes)
    const uint32_t r0 = d.piece_row[p];
    for (uint32_t r = r0 + threadIdx.x; r < d.nrows; r += kThreads) {
        const uint32_t off = d.row_off[r];
        if (off >= hi) break;
        if (off < lo) continue;
        const uint8_t *q = stage + sh + (off - lo);
        uint32_t w4[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            w4[k] = (uint32_t)q[4 * k] | ((uint32_t)q[4 * k + 1] << 8) | ((uint32_t)q[4 * k + 2] << 16) | ((uint32_t)q[4 * k + 3] << 24);
        T[lt.at(r, s)] = label_be(make_uint4(w4[0], w4[1], w4[2], w4[3]));
    }
    __syncthreads();
    // ... and every row byte of the piece becomes zero, as in the skeleton: what is left to compare is structure
    for (uint32_t r = r0 + threadIdx.x; r < d.nrows; r += kThreads) {
        const uint32_t off = d.row_off[r];
        if (off >= hi) break;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t at = off + k;
            if (at >= lo && at < hi) stage[sh + at - lo] = 0;
        }
    }
    __syncthreads();
    const uint32_t *sk = (const uint32_t *)(d.skel + lo);
    uint32_t diff = 0;
    for (uint32_t k = threadIdx.x; 4 * k < nb; k += kThreads) {
        const uint8_t *q = stage + sh + 4 * k;
        const uint32_t have = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        uint32_t x = have ^ sk[k];
        if (nb - 4 * k < 4) x &= (1u << (8 * (nb - 4 * k))) - 1u;  // (the last word of the step may reach past its bytes)
        diff += ((x & 0xffu) != 0) + ((x & 0xff00u) != 0) + ((x & 0xff0000u) != 0) + ((x & 0xff000000u) != 0);
    }
    for (int o = 32; o > 0; o >>= 1) diff += __shfl_down(diff, o, 64);
    if ((threadIdx.x & 63) == 0 && diff) atomicAdd(bad + s, diff);
}

// ---- inputs and results (gc_stream_batch_select_labels_dev / _decode_dev) ----------------------------------------------------
// The store is [wire id][bstride], the callers' arrays are [session][n].  A tile of kIoIds ids x kIoSessions sessions is read
// with the lanes along the sessions (512 contiguous bytes of a store row), turned in LDS as k_gather turns its tile, and used
// with the lanes along the ids: a wave owns one session's 64 consecutive entries, 1 KiB of labels or 64 bytes of bits.  The
// tiles along the ids are swept (gridDim.x is capped), so any n runs.
__device__ __forceinline__ void io_tile_in(uint4 (*tile)[kIoSessions + 1], const uint4 *__restrict__ store, uint32_t bstride,
                                           const uint32_t *__restrict__ ids, uint32_t n, uint32_t S, uint32_t j0, uint32_t i0) {
    const uint32_t tx = threadIdx.x & (kIoSessions - 1), ty = threadIdx.x / kIoSessions;
    const uint32_t i = i0 + tx;
    for (uint32_t r = ty; r < kIoIds; r += kThreads / kIoSessions) {
        const uint32_t j = j0 + r;
        if (j < n && i < S) tile[r][tx] = store[(size_t)ids[j] * bstride + i];
    }
}

__global__ __launch_bounds__(kThreads) void k_sb_select(const uint4 *__restrict__ store, uint32_t bstride,
                                                        const uint32_t *__restrict__ ids, uint32_t n, const uint4 *__restrict__ R,
                                                        const uint8_t *__restrict__ bits, uint4 *__restrict__ out, uint32_t S) {
    __shared__ uint4 tile[kIoIds][kIoSessions + 1];
    const uint32_t i0 = blockIdx.y * kIoSessions, ntiles = (n + kIoIds - 1) / kIoIds;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t j0 = t * kIoIds, j = j0 + lane;
        io_tile_in(tile, store, bstride, ids, n, S, j0, i0);
        __syncthreads();
        for (uint32_t r = wave; r < kIoSessions; r += kThreads / 64) {
            const uint32_t i = i0 + r;
            if (j < n && i < S) {
                const size_t at = (size_t)i * n + j;
                const uint32_t m = bits[at] ? 0xffffffffu : 0u;
                const uint4 v = tile[lane][r], rr = R[i];
                out[at] = make_uint4(v.x ^ (rr.x & m), v.y ^ (rr.y & m), v.z ^ (rr.z & m), v.w ^ (rr.w & m));
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_sb_decode(const uint4 *__restrict__ store, uint32_t bstride,
                                                        const uint32_t *__restrict__ ids, uint32_t n, const uint4 *__restrict__ R,
                                                        const uint4 *__restrict__ labels, uint8_t *__restrict__ bits_out,
                                                        uint32_t *__restrict__ bad, uint32_t S) {
    __shared__ uint4 tile[kIoIds][kIoSessions + 1];
    const uint32_t i0 = blockIdx.y * kIoSessions, ntiles = (n + kIoIds - 1) / kIoIds;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t j0 = t * kIoIds, j = j0 + lane;
        io_tile_in(tile, store, bstride, ids, n, S, j0, i0);
        __syncthreads();
        for (uint32_t r = wave; r < kIoSessions; r += kThreads / 64) {  // (uniform per wave: one session at a time)
            const uint32_t i = i0 + r;
            uint32_t unknown = 0;
            if (j < n && i < S) {
                const size_t at = (size_t)i * n + j;
                const uint4 l0 = tile[lane][r], rr = R[i], lab = labels[at];
                const uint4 d = make_uint4(lab.x ^ l0.x, lab.y ^ l0.y, lab.z ^ l0.z, lab.w ^ l0.w);
                uint8_t bit = 0xff;  // BitFromLabel's "unknown label" (streamer.go:563-579)
                if ((d.x | d.y | d.z | d.w) == 0) bit = 0;
                else if (((d.x ^ rr.x) | (d.y ^ rr.y) | (d.z ^ rr.z) | (d.w ^ rr.w)) == 0) bit = 1;
                bits_out[at] = bit;
                unknown = bit == 0xff;
            }
            for (int o = 32; o > 0; o >>= 1) unknown += __shfl_down(unknown, o, 64);
            if (lane == 0 && unknown) atomicAdd(bad + i, unknown);
        }
        __syncthreads();
    }
}

// the evaluator's result labels (gc_stream_eval_batch_return_labels_dev): the same tile and the same turn as k_sb_select, with
// nothing to add to the label — no R and no bits
__global__ __launch_bounds__(kThreads) void k_sb_return(const uint4 *__restrict__ store, uint32_t bstride,
                                                        const uint32_t *__restrict__ ids, uint32_t n, uint4 *__restrict__ out,
                                                        uint32_t S) {
    __shared__ uint4 tile[kIoIds][kIoSessions + 1];
    const uint32_t i0 = blockIdx.y * kIoSessions, ntiles = (n + kIoIds - 1) / kIoIds;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t j0 = t * kIoIds, j = j0 + lane;
        io_tile_in(tile, store, bstride, ids, n, S, j0, i0);
        __syncthreads();
        for (uint32_t r = wave; r < kIoSessions; r += kThreads / 64) {
            const uint32_t i = i0 + r;
            if (j < n && i < S) out[(size_t)i * n + j] = tile[lane][r];
        }
        __syncthreads();
    }
}

// ---- the framing of a fed chunk (gc_stream_eval_batch_in_feed) ---------------------------------------------------------------
// The 20 header bytes of message m of session s against the reference session's, for every (message, session) pair of a chunk:
// a wave owns one session and its lanes the messages, so that a session's count is one sum over a wave.  off[m] comes from
// the reference session's bytes (the host walked them); no byte of any session is used as an index.  The honest path has no
// atomic: a wave that saw no difference adds nothing.
__global__ __launch_bounds__(kThreads) void k_sb_frames(const uint8_t *__restrict__ buf, size_t pitch, const uint32_t *__restrict__ off,
                                                        uint32_t nmsg, uint32_t S, uint32_t ref, uint32_t *__restrict__ bad) {
    const uint32_t lane = threadIdx.x & 63, s = blockIdx.y * (kThreads / 64) + (threadIdx.x >> 6);
    if (s >= S) return;  // (uniform per wave)
    const uint8_t *mine = buf + (size_t)s * pitch, *theirs = buf + (size_t)ref * pitch;
    uint32_t diff = 0;
    for (uint32_t m = blockIdx.x * 64 + lane; m < nmsg; m += gridDim.x * 64) {
        const uint32_t at = off[m];
#pragma unroll
        for (uint32_t k = 0; k < kFrameBytes; k++) diff += mine[at + k] != theirs[at + k];
    }
    if (__ballot(diff != 0) == 0) return;
    for (int o = 32; o > 0; o >>= 1) diff += __shfl_down(diff, o, 64);
    if (lane == 0) atomicAdd(bad + s, diff);
}

}  // namespace

void launch_select(const uint4 *store, uint32_t bstride, const uint32_t *ids, uint32_t n, const uint4 *R, const uint8_t *bits,
                   uint4 *out, uint32_t S, hipStream_t s) {
    if (n == 0 || S == 0) return;
    const uint32_t ntiles = (n + kIoIds - 1) / kIoIds;
    hipLaunchKernelGGL(k_sb_select, dim3(ntiles < kIoMaxTiles ? ntiles : kIoMaxTiles, (S + kIoSessions - 1) / kIoSessions),
                       dim3(kThreads), 0, s, store, bstride, ids, n, R, bits, out, S);
}

void launch_decode_labels(const uint4 *store, uint32_t bstride, const uint32_t *ids, uint32_t n, const uint4 *R, const uint4 *labels,
                          uint8_t *bits_out, uint32_t *bad, uint32_t S, hipStream_t s) {
    if (n == 0 || S == 0) return;
    const uint32_t ntiles = (n + kIoIds - 1) / kIoIds;
    hipLaunchKernelGGL(k_sb_decode, dim3(ntiles < kIoMaxTiles ? ntiles : kIoMaxTiles, (S + kIoSessions - 1) / kIoSessions),
                       dim3(kThreads), 0, s, store, bstride, ids, n, R, labels, bits_out, bad, S);
}

void launch_return_labels(const uint4 *store, uint32_t bstride, const uint32_t *ids, uint32_t n, uint4 *out, uint32_t S, hipStream_t s) {
    if (n == 0 || S == 0) return;
    const uint32_t ntiles = (n + kIoIds - 1) / kIoIds;
    hipLaunchKernelGGL(k_sb_return, dim3(ntiles < kIoMaxTiles ? ntiles : kIoMaxTiles, (S + kIoSessions - 1) / kIoSessions),
                       dim3(kThreads), 0, s, store, bstride, ids, n, out, S);
}

void launch_frames(const uint8_t *buf, size_t pitch, const uint32_t *off, uint32_t nmsg, uint32_t S, uint32_t ref, uint32_t *bad,
                   hipStream_t s) {
    if (nmsg == 0 || S == 0) return;
    const uint32_t nx = (nmsg + 63) / 64;
    hipLaunchKernelGGL(k_sb_frames, dim3(nx < kIoMaxTiles ? nx : kIoMaxTiles, (S + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads),
                       0, s, buf, pitch, off, nmsg, S, ref, bad);
}

void launch_rnd_form(uint4 *rnd, const uint4 *R, uint32_t S, uint32_t n1, hipStream_t s) {
    const size_t n = (size_t)S * n1;
    hipLaunchKernelGGL(k_sb_rnd_form, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, rnd, R, S, n1);
}

void launch_init_store(const uint4 *rnd, const uint32_t *ids, uint32_t n, uint4 *store, uint32_t bstride, uint4 *R, uint32_t S,
                       hipStream_t s) {
    const size_t tot = (size_t)S * (n + 1);
    hipLaunchKernelGGL(k_sb_init_store, dim3((uint32_t)((tot + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, rnd, ids, n, store,
                       bstride, R, S);
}

void launch_rows(const uint4 *src, const Layout &sl, const uint32_t *srow, uint4 *dst, const Layout &dl, const uint32_t *drow,
                 uint32_t n, uint32_t S, hipStream_t s) {
    if (n == 0 || S == 0) return;
    hipLaunchKernelGGL(k_sb_rows, dim3((S + kThreads - 1) / kThreads, n < 65535u ? n : 65535u), dim3(kThreads), 0, s, src, sl, srow, dst, dl,
                       drow, n, S);
}

void launch_serialise(const StepDev &d, const uint4 *T, const Layout &lt, uint8_t *out, size_t stride, uint32_t S, hipStream_t s) {
    if (d.npieces == 0 || S == 0) return;
    hipLaunchKernelGGL(k_sb_serialise, dim3(d.npieces, S), dim3(kThreads), 0, s, d, T, lt, out, stride);
}

void launch_serialise_range(const StepDev &d, const uint4 *T, const Layout &lt, uint8_t *out, size_t stride, uint32_t S, uint32_t b0,
                            uint32_t b1, hipStream_t s) {
    if (b0 >= b1 || b1 > d.nbytes || S == 0) return;
    hipLaunchKernelGGL(k_sb_serialise_range, dim3((b1 - b0 + kPieceBytes - 1) / kPieceBytes, S), dim3(kThreads), 0, s, d, T, lt, out,
                       stride, b0, b1);
}

void launch_ingest(const StepDev &d, uint4 *T, const Layout &lt, const uint8_t *in, size_t stride, uint32_t S, uint32_t *bad,
                   hipStream_t s) {
    if (d.npieces == 0 || S == 0) return;
    hipLaunchKernelGGL(k_sb_ingest, dim3(d.npieces, S), dim3(kThreads), 0, s, d, T, lt, in, stride, bad);
}

}  // namespace gcsb
