// gmw_kernels.hip — device side of the GMW party engine (gmw_engine.cpp): one launch per exchange round.
//
// Shares live instance-bit-sliced: slots[s][j] holds wire slot s of instances 64 j .. 64 j + 63, one instance per bit, so a
// free gate is one u64 op for 64 instances.  Messages, triples, inputs and outputs are gate-packed ([words][batch], bit k =
// gate / wire 64 w + k of one instance: the Go bit vectors).  A wave64 converts between the two with a 64 x 64 bit transpose
// (six __shfl_xor butterfly stages): lane l holds row l and gets back row l of the transpose.
//
// A step is one workgroup per instance word j (grid split as in split_grid.h past 2^24 workgroups).  It closes the pending
// AND level (z fold), walks the round's free gates sub-round by sub-round with workgroup barriers, and opens the next AND
// level.  A slot written in the launch is read back by other waves of the same workgroup after a barrier: its stores and
// loads are agent-scope accesses that go past the L1 (as store_get / store_put of the fused kernels), and every wave waits
// for its stores before the barrier.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gmw.h"
#include "split_grid.h"

namespace gc {

namespace {

constexpr uint32_t kGmwThreads = 256;
constexpr uint32_t kGmwWaves = kGmwThreads / 64;

__device__ __forceinline__ uint64_t slot_get(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void slot_put(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// every wave's stores are acknowledged, then the workgroup meets
__device__ __forceinline__ void wg_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// 64 x 64 bit transpose across the wave: lane l passes row l, gets back column l (bit i = bit l of row i).  Six butterfly
// stages; stage s swaps the off-diagonal s x s blocks between lanes l and l ^ s.
__device__ __forceinline__ uint64_t wave_transpose(uint64_t row, uint32_t lane) {
    constexpr uint64_t kMask[6] = {0x00000000FFFFFFFFull, 0x0000FFFF0000FFFFull, 0x00FF00FF00FF00FFull,
                                   0x0F0F0F0F0F0F0F0Full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const uint32_t s = 32u >> i;
        const uint64_t m = kMask[i];
        const uint64_t other = __shfl_xor(row, (int)s);
        row = (lane & s) ? (row & ~m) | ((other >> s) & m) : (row & m) | ((other & m) << s);
    }
    return row;
}

__device__ __forceinline__ uint32_t block_index() { return blockIdx.y * gridDim.x + blockIdx.x; }

__global__ void __launch_bounds__(kGmwThreads) k_gmw_inputs(uint64_t *__restrict__ slots, const uint64_t *__restrict__ in,
                                                            uint32_t ninputs, uint32_t batch, uint32_t bw) {
    const uint32_t j = block_index();
    if (j >= bw) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inst = 64 * j + lane;
    const uint32_t nq = (ninputs + 63) / 64;
    for (uint32_t q = wave; q < nq; q += kGmwWaves) {
        const uint64_t row = inst < batch ? in[(size_t)q * batch + inst] : 0;  // wires 64 q .. of instance `inst`
        const uint64_t col = wave_transpose(row, lane);                         // wire 64 q + lane of 64 instances
        const uint32_t w = 64 * q + lane;
        if (w < ninputs) slots[(size_t)w * bw + j] = col;
    }
}

__global__ void __launch_bounds__(kGmwThreads) k_gmw_step(GmwStepArgs a) {
    const uint32_t j = block_index();
    if (j >= a.bw) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inst = 64 * j + lane;
    const bool live = inst < a.batch;
    const uint64_t p0 = a.party0 ? ~0ull : 0ull;
    uint64_t *const S = a.slots;
    const size_t bw = a.bw, batch = a.batch;

    // (1) close the pending AND level: z = c ^ d&b ^ e&a (^ d&e on party 0)   network.go:735-756
    if (a.close_n) {
        for (uint32_t k = wave; k < a.close_w; k += kGmwWaves) {
            uint64_t z = 0;
            if (live) {
                const size_t di = (size_t)k * batch + inst, ei = (size_t)(a.close_w + k) * batch + inst;
                uint64_t d = a.own_prev[di], e = a.own_prev[ei];
                const size_t msg = (size_t)2 * a.close_w * batch;
                for (uint32_t p = 0; p < a.npeers; p++) {
                    d ^= a.peers[p * msg + di];
                    e ^= a.peers[p * msg + ei];
                }
                const size_t t = (size_t)(a.close_W + k) * batch + inst;
                z = a.tc[t] ^ (d & a.tb[t]) ^ (e & a.ta[t]) ^ (d & e & p0);
            }
            const uint64_t col = wave_transpose(z, lane);  // AND gate 64 k + lane of 64 instances
            const uint32_t g = 64 * k + lane;
            if (g < a.close_n) slot_put(S + (size_t)a.close_out[g] * bw + j, col);
        }
        wg_sync();
    }

    // (2) the round's free gates, one sub-round per barrier   network.go:578-612
    for (uint32_t s = 0; s < a.nsub; s++) {
        const uint32_t end = a.sub[s + 1];
        for (uint32_t i = a.sub[s] + threadIdx.x; i < end; i += kGmwThreads) {
            const GmwGate g = a.gates[i];
            const uint64_t x = slot_get(S + (size_t)g.in0 * bw + j);
            uint64_t v;
            if (g.op == GC_INV) {
                v = x ^ p0;
            } else {
                v = x ^ slot_get(S + (size_t)g.in1 * bw + j);
                if (g.op == GC_XNOR) v ^= p0;
            }
            slot_put(S + (size_t)g.out * bw + j, v);
        }
        wg_sync();
    }

    // (3) open the round's AND level: d = x ^ a, e = y ^ b, padding gates read 0   network.go:695-721
    for (uint32_t k = wave; k < a.and_w; k += kGmwWaves) {
        const uint32_t g = 64 * k + lane;
        uint64_t x = 0, y = 0;
        if (g < a.and_n) {
            x = slot_get(S + (size_t)a.and_in[g] * bw + j);
            y = slot_get(S + (size_t)a.and_in[a.and_n + g] * bw + j);
        }
        const uint64_t X = wave_transpose(x, lane), Y = wave_transpose(y, lane);  // ANDs 64 k .. of instance `inst`
        if (live) {
            const size_t t = (size_t)(a.and_W + k) * batch + inst;
            const uint64_t d = X ^ a.ta[t], e = Y ^ a.tb[t];
            const size_t di = (size_t)k * batch + inst, ei = (size_t)(a.and_w + k) * batch + inst;
            a.own_next[di] = d;
            a.own_next[ei] = e;
            a.msg_out[di] = d;
            a.msg_out[ei] = e;
        }
    }

    // (4) last round: this party's output shares, gate-packed   network.go:622-624
    const uint32_t nq = (a.nout + 63) / 64;
    for (uint32_t q = wave; q < nq; q += kGmwWaves) {
        const uint32_t o = 64 * q + lane;
        const uint64_t v = o < a.nout ? slot_get(S + (size_t)a.out_slots[o] * bw + j) : 0;
        const uint64_t row = wave_transpose(v, lane);
        if (live) a.out[(size_t)q * batch + inst] = row;
    }
}

// the local words of tripleBatch (triples.go:312-315, 340-349, 362-364, 387-389)
__global__ void __launch_bounds__(256) k_gmw_fold(int kind, uint64_t dmask, const uint64_t *x, const uint64_t *y,
                                                   const uint64_t *z, uint64_t *c, size_t words) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
        switch (kind) {
        case 0: c[i] = x[i] & y[i]; break;             // c = a & b
        case 1: c[i] = x[i] ^ dmask; break;            // u = a ^ (D0 ? ~0 : 0)
        case 2: c[i] ^= x[i] ^ (y[i] & z[i]); break;   // c ^= s ^ (u & v)
        default: c[i] ^= x[i]; break;                  // c ^= r
        }
    }
}

dim3 word_grid(uint32_t bw) {
    if (bw <= kSplitMaxX) return dim3(bw, 1, 1);
    return dim3(kSplitRowBlocks, (bw + kSplitRowBlocks - 1) / kSplitRowBlocks, 1);
}

}  // namespace

hipError_t gmw_launch_inputs(hipStream_t s, uint64_t *slots, const uint64_t *in, uint32_t ninputs, uint32_t batch, uint32_t bw) {
    if (!bw) return hipSuccess;
    hipLaunchKernelGGL(k_gmw_inputs, word_grid(bw), dim3(kGmwThreads), 0, s, slots, in, ninputs, batch, bw);
    return hipGetLastError();
}

hipError_t gmw_launch_step(hipStream_t s, const GmwStepArgs &a) {
    if (!a.bw) return hipSuccess;
    hipLaunchKernelGGL(k_gmw_step, word_grid(a.bw), dim3(kGmwThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t gmw_launch_fold(hipStream_t s, int kind, uint32_t delta_bit, const uint64_t *x, const uint64_t *y, const uint64_t *z,
                           uint64_t *c, size_t words) {
    if (!words) return hipSuccess;
    const size_t blocks = std::min<size_t>((words + 255) / 256, 65536);
    hipLaunchKernelGGL(k_gmw_fold, dim3((uint32_t)blocks), dim3(256), 0, s, kind, delta_bit ? ~0ull : 0ull, x, y, z, c, words);
    return hipGetLastError();
}

}  // namespace gc
