// rand_cursor_kernels.hip — CDNA4 kernels of the per-session cursors of the device random streams (gc_rand_*_cur*;
// rand_ctr.h defines the streams, rand_int.h crand.Int on them).  The position of stream s is cur[s] in device
// memory: the kernels read it and advance it, so sessions may diverge and a replayed graph goes on where the array stands.
//
//   k_rand_cur_fill     bytes [cur[s], cur[s] + n) of every stream into the caller's slots.  The launch shape of k_rand_fill
//                       (rand_kernels.hip): persistent 1024-lane workgroups around the dual table, a unit = a wave's run of 64
//                       blocks of one stream, round keys wave-uniform.  The cover is per stream, so head and first block
//                       differ per stream and the block count by at most one: units are sized from the largest cover a
//                       cursor can give, lanes past their stream's cover do nothing, and the aligned / bytewise decision is
//                       per slot.  Several waves of several workgroups serve one stream and all of them read cur[s]:
//                       nothing in this launch writes it.  Lane 0 of the grid resets the status block.
//   k_rand_cur_advance  behind the fill, one lane per session: cur[s] += n, or the session counted in the status block.
//   k_rand_cur_scalars  `count` crand.Int draws per session.  A wave owns a session (only it reads and writes cur[s]).  It
//                       encrypts a run of 64 blocks, one per lane, into its 1 KiB slab of LDS beside the dual table, and the
//                       lanes then gather one candidate each from the slab, 64 candidates a chunk: a ballot is the accept
//                       mask, rand_int_slot the output index, rand_int_walk_step the end of the walk.  A slab holds
//                       (1024 - off) / k whole candidates; the next slab starts at the block of the first candidate behind
//                       them.  The walk runs twice, as rand_int_walk does: the first pass writes nothing and finds out
//                       whether the bound holds, so that a bad session's outputs stay untouched.  Every loop is bounded by
//                       rand_int_cap(count).
//   k_rand_status_reset the status block {0, ~0} in front of k_rand_cur_scalars.
#include <algorithm>

#include "aes_device.h"
#include "kernels.h"
#include "rand_int.h"

namespace gc {

namespace {

constexpr int kRandWaves = kRandThreads / 64;  // waves of a workgroup
constexpr uint32_t kSlabBytes = 16 * kRandRun;  // of a wave: its run of blocks as the stream's bytes
constexpr size_t kScalarsLds = kTeDualBytes + kRandWaves * kSlabBytes;

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    return ((uint64_t)hi << 32) | lo;
}

// status: {bad sessions, lowest bad session}
__device__ __forceinline__ void report_bad(uint64_t *status, uint64_t s) {
    atomicAdd((unsigned long long *)status, 1ull);
    atomicMin((unsigned long long *)status + 1, (unsigned long long)s);
}

// The wave's round keys: the first words scalar, the last NV in VGPRs (with all 60 words of AES-256 in SGPRs the loop's own
// scalars spill).  vz is a zero the compiler cannot see through: the words behind it come by vector loads and never pass
// through SGPRs, which a readfirstlane of all of them would at its peak.
template <int NR, int NV = 16>
__device__ __forceinline__ void wave_keys(uint32_t (&rk)[4 * (NR + 1)], const uint32_t *__restrict__ g_rk, uint32_t vz) {
    constexpr int NS = 4 * (NR + 1) - NV;
    const uint32_t *vp = g_rk + vz;  // one vector address; the words behind it are its constant offsets
#pragma unroll
    for (int i = 0; i < 4 * (NR + 1); i++) rk[i] = i < NS ? (uint32_t)__builtin_amdgcn_readfirstlane(g_rk[i]) : vp[i];
}

// block `blk` of the stream as it lies in memory: x holds bytes 0..3, byte 0 lowest
template <int NR>
__device__ __forceinline__ uint4 stream_block(const RandCtr &iv, uint64_t blk, const uint32_t (&rk)[4 * (NR + 1)],
                                              const uint32_t *te, uint32_t lo0) {
    const RandCtr c = rand_ctr_add(iv, blk);
    uint32_t st[1][4] = {{(uint32_t)(c.hi >> 32), (uint32_t)c.hi, (uint32_t)(c.lo >> 32), (uint32_t)c.lo}};
    aes_encrypt_dual<NR, 1>(st, rk, te, lo0);
    __builtin_amdgcn_sched_barrier(0);  // addresses are worked out behind the rounds, not kept alive across them
    return make_uint4(__builtin_bswap32(st[0][0]), __builtin_bswap32(st[0][1]), __builtin_bswap32(st[0][2]),
                      __builtin_bswap32(st[0][3]));
}

template <int NR>
__global__ __launch_bounds__(kRandThreads) void k_rand_cur_fill(const uint32_t *__restrict__ rk_all, const RandCtr *__restrict__ ivs,
                                                                uint64_t S, const uint64_t *__restrict__ cur, uint64_t n,
                                                                uint8_t *out, uint64_t stride, uint64_t *status,
                                                                const uint32_t *__restrict__ g_te0) {
    constexpr int NW = 4 * (NR + 1);
    extern __shared__ uint4 smem[];
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // k_rand_cur_advance, behind this launch, fills it
        status[0] = 0;
        status[1] = ~0ull;
    }
    const uint32_t lo0 = te_lane_off(), lane = threadIdx.x & 63u;
    const uint64_t ups = rand_units(rand_cover(15, n).nblocks), units = S * ups;  // the largest cover of n bytes
    const uint64_t nwaves = (uint64_t)gridDim.x * kRandWaves;
    uint64_t u = (uint64_t)blockIdx.x * kRandWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= units) return;
    const uint64_t qn = nwaves / ups, rn = nwaves - qn * ups;
    uint64_t s = uniform64(u / ups), r = uniform64(u - (u / ups) * ups);
    uint32_t vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    while (s < S) {
        uint32_t rk[NW];
        wave_keys<NR>(rk, rk_all + s * NW, vz);
        const RandCtr iv{uniform64(ivs[s].hi), uniform64(ivs[s].lo)};
        const uint64_t pos = uniform64(cur[s]);
        const bool good = rand_range_ok(pos, n);  // a bad session's slot stays as it is
        const RandCover cov = rand_cover(pos, n);
        uint8_t *slot = out + s * stride;
        const bool aligned = (((uintptr_t)slot - cov.head) & 15u) == 0;  // every whole block of the slot, or none
        const uint64_t at_s = s;
        do {
            const uint64_t k = r * kRandRun + lane;
            if (good && k < cov.nblocks) {
                uint4 w = stream_block<NR>(iv, cov.first + k, rk, (const uint32_t *)smem, lo0);
                const RandPiece p = rand_piece(cov, n, k);
                if (aligned && p.from == 0 && p.to == 16) {
                    *(uint4 *)(slot + p.at) = w;
                } else {
                    uint8_t *dst = slot + p.at - p.from;  // where byte 0 of the block would go
#pragma unroll 1
                    for (uint32_t b = 0; b < p.to; b++) {
                        if (b >= p.from) dst[b] = (uint8_t)w.x;
                        w.x = __builtin_amdgcn_alignbit(w.y, w.x, 8);
                        w.y = __builtin_amdgcn_alignbit(w.z, w.y, 8);
                        w.z = __builtin_amdgcn_alignbit(w.w, w.z, 8);
                        w.w >>= 8;
                    }
                }
            }
            s += qn;
            r += rn;
            if (r >= ups) {
                r -= ups;
                s++;
            }
        } while (s == at_s);
    }
}

__global__ __launch_bounds__(kRandExpandThreads) void k_rand_cur_advance(uint64_t *__restrict__ cur, uint64_t S, uint64_t n,
                                                                         uint64_t *status) {
    for (uint64_t s = (uint64_t)blockIdx.x * kRandExpandThreads + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kRandExpandThreads) {
        const uint64_t pos = cur[s];
        if (rand_range_ok(pos, n)) cur[s] = pos + n;
        else report_bad(status, s);
    }
}

// cur[s] = pos for every s
__global__ __launch_bounds__(kRandExpandThreads) void k_rand_cur_set(uint64_t *__restrict__ cur, uint64_t S, uint64_t pos) {
    for (uint64_t s = (uint64_t)blockIdx.x * kRandExpandThreads + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kRandExpandThreads)
        cur[s] = pos;
}

__global__ void k_rand_status_reset(uint64_t *status) {
    status[0] = 0;
    status[1] = ~0ull;
}

// out: [S][count][32], scalars big-endian
template <int NR>
__global__ __launch_bounds__(kRandThreads) void k_rand_cur_scalars(const uint32_t *__restrict__ rk_all, const RandCtr *__restrict__ ivs,
                                                                   uint64_t S, uint64_t *cur, RandIntShape sh, uint64_t count,
                                                                   uint8_t *out, uint64_t *status, const uint32_t *__restrict__ g_te0) {
    constexpr int NW = 4 * (NR + 1);
    extern __shared__ uint4 smem[];
    load_te_dual((uint32_t *)smem, g_te0);
    __syncthreads();
    const uint32_t lo0 = te_lane_off(), lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *slab = (uint8_t *)smem + kTeDualBytes + wave * kSlabBytes;
    const uint64_t cap = rand_int_cap(count);
    const bool words = ((uintptr_t)out & 15u) == 0;  // scalars are 32 bytes: all of them on 16-byte boundaries, or none
    uint32_t vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    // the modulus in VGPRs, for the same reason as the last round keys: the walk's own scalars need the SGPRs
    RandIntShape vsh = sh;
    vsh.mask ^= vz;
#pragma unroll
    for (int i = 0; i < 8; i++) vsh.max[i] ^= vz;
    for (uint64_t s = (uint64_t)blockIdx.x * kRandWaves + wave; s < S; s += (uint64_t)gridDim.x * kRandWaves) {
        uint32_t rk[NW];
        wave_keys<NR, NW - 20>(rk, rk_all + s * NW, vz);  // five rounds' keys scalar: the walk's scalars take the rest
        const RandCtr iv{uniform64(ivs[s].hi), uniform64(ivs[s].lo)};
        const uint64_t pos = uniform64(cur[s]);
        bool bad = !rand_int_range_ok(sh, pos, count);
        RandIntWalk w;
        for (int pass = 0; pass < 2 && !bad; pass++) {  // pass 0 writes nothing (rand_int_walk)
            w = RandIntWalk{};
            bool done = false;
            while (!done && w.consumed < cap) {
                const RandPos p = rand_pos_split(pos + w.consumed * sh.k);  // of the slab's first candidate
                *(uint4 *)(slab + 16 * lane) = stream_block<NR>(iv, p.block + lane, rk, (const uint32_t *)smem, lo0);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const uint64_t left = cap - w.consumed;
                const uint32_t fit = (kSlabBytes - p.off) / sh.k;  // >= 31
                const uint32_t m = left < fit ? (uint32_t)left : fit;
                for (uint32_t j0 = 0; j0 < m && !done; j0 += kRandIntChunk) {
                    const uint32_t nc = m - j0 < kRandIntChunk ? m - j0 : kRandIntChunk;
                    bool ok = false;
                    uint32_t v[8];
                    if (lane < nc) {
                        const uint8_t *src = slab + p.off + (j0 + lane) * sh.k;  // ends inside the slab: j0 + lane < fit
                        rand_int_candidate(vsh, [&](int32_t i) { return (uint32_t)src[i]; }, v);  // i < 0: LDS in front, masked
                        ok = rand_int_accept(vsh, v);
                    }
                    const uint64_t accept = __builtin_amdgcn_ballot_w64(ok);
                    if (pass == 1 && ok) {
                        const uint64_t slot = rand_int_slot(w, accept, lane);
                        if (slot < count) {
                            uint8_t *dst = out + (s * count + slot) * 32;
                            if (words) {
                                ((uint4 *)dst)[0] = make_uint4(__builtin_bswap32(v[0]), __builtin_bswap32(v[1]), __builtin_bswap32(v[2]),
                                                               __builtin_bswap32(v[3]));
                                ((uint4 *)dst)[1] = make_uint4(__builtin_bswap32(v[4]), __builtin_bswap32(v[5]), __builtin_bswap32(v[6]),
                                                               __builtin_bswap32(v[7]));
                            } else {
#pragma unroll
                                for (int q = 0; q < 32; q++) dst[q] = (uint8_t)(v[q >> 2] >> (8 * (3 - (q & 3))));
                            }
                        }
                    }
                    done = rand_int_walk_step(w, count, accept, nc);
                }
                __builtin_amdgcn_wave_barrier();  // the slab is read out before the next run overwrites it
            }
            bad = !done;
        }
        if (lane == 0) {
            if (bad) report_bad(status, s);
            else cur[s] = pos + w.consumed * sh.k;
        }
    }
}

unsigned lane_grid(size_t S) {
    return (unsigned)std::min<uint64_t>(kRandExpandGrid, ((uint64_t)S + kRandExpandThreads - 1) / kRandExpandThreads);
}

}  // namespace

hipError_t launch_rand_cur_set(uint64_t *d_cur, size_t S, uint64_t pos, hipStream_t s) {
    return launch_kernel(k_rand_cur_set, lane_grid(S), kRandExpandThreads, s, d_cur, (uint64_t)S, pos);
}

hipError_t launch_rand_cur_fill(int rounds, const uint32_t *d_rk, const RandCtr *d_iv, size_t S, uint64_t *d_cur, uint64_t n,
                                uint8_t *d_out, size_t stride, uint64_t *d_status, const uint32_t *te0, hipStream_t s) {
    const uint64_t units = (uint64_t)S * rand_units(rand_cover(15, n).nblocks);
    const unsigned grid = (unsigned)std::min<uint64_t>(kRandGrid, (units + kRandWaves - 1) / kRandWaves);
    hipError_t e = with_rounds(rounds, [&](auto nr) {
        return launch_with_lds(k_rand_cur_fill<decltype(nr)::value>, grid, kRandThreads, kTeDualBytes, s, d_rk, d_iv, (uint64_t)S,
                               (const uint64_t *)d_cur, n, d_out, (uint64_t)stride, d_status, te0);
    });
    if (e != hipSuccess) return e;
    return launch_kernel(k_rand_cur_advance, lane_grid(S), kRandExpandThreads, s, d_cur, (uint64_t)S, n, d_status);
}

hipError_t launch_rand_cur_scalars(int rounds, const uint32_t *d_rk, const RandCtr *d_iv, size_t S, uint64_t *d_cur,
                                   const RandIntShape &shape, uint64_t count, uint8_t *d_out, uint64_t *d_status,
                                   const uint32_t *te0, hipStream_t s) {
    hipError_t e = launch_kernel(k_rand_status_reset, 1, 1, s, d_status);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)std::min<uint64_t>(kRandGrid, ((uint64_t)S + kRandWaves - 1) / kRandWaves);
    return with_rounds(rounds, [&](auto nr) {
        return launch_with_lds(k_rand_cur_scalars<decltype(nr)::value>, grid, kRandThreads, kScalarsLds, s, d_rk, d_iv, (uint64_t)S,
                               d_cur, shape, count, d_out, d_status, te0);
    });
}

}  // namespace gc
