// mad_rate_ubench.hip — the card's own 32 x 32 -> 64 bit multiply-add rate (developer tool, in the manner of
// issue_rate_ubench.hip).  The limb products of the P-256 arithmetic (mpc_amd/csrc/vole_mod.h: vole_mont_mul) are
// v_mad_u64_u32; scripts/bench_co.py divides the products the Chou-Orlandi kernels need by this rate, measured in the same
// run, to say what share of the multiplier they use.
//
// Every lane runs 8 independent chains of v_mad_u64_u32, 64 instructions per loop iteration; 1 024 workgroups of 256 threads
// (four waves per SIMD on 256 CUs).  Timing: a host clock around launches that end in hipDeviceSynchronize, windows of at
// least 0.2 s after a warm-up, median of 5.  Output: one JSON line.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HIPCHECK(x)                                                  \
    do {                                                             \
        hipError_t e__ = (x);                                        \
        if (e__ != hipSuccess) {                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__)); \
            exit(1);                                                 \
        }                                                            \
    } while (0)

#define MAD(A) "v_mad_u64_u32 " A ", vcc, %8, %9, " A "\n"
#define REP8(X) X X X X X X X X

__global__ __launch_bounds__(256) void k_mad(uint64_t *out, int iters) {
    uint64_t a0 = threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, a6 = a0 * 17, a7 = a0 * 19;
    const uint32_t b = blockIdx.x * 77u + threadIdx.x + 1u, c = b * 31u + 5u;
    for (int it = 0; it < iters; it++) {
        asm volatile(REP8(MAD("%0") MAD("%1") MAD("%2") MAD("%3") MAD("%4") MAD("%5") MAD("%6") MAD("%7"))
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                     : "v"(b), "v"(c)
                     : "vcc");
    }
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}

static double seconds(uint64_t *d_out, int grid, int iters, int launches) {
    HIPCHECK(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < launches; i++) hipLaunchKernelGGL(k_mad, dim3(grid), dim3(256), 0, 0, d_out, iters);
    HIPCHECK(hipDeviceSynchronize());
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int main() {
    const int grid = 1024, iters = 4000;
    uint64_t *d_out;
    HIPCHECK(hipMalloc(&d_out, (size_t)grid * 256 * 8));
    for (int i = 0; i < 3; i++) seconds(d_out, grid, iters, 1);  // warm-up: code object, clocks
    const double one = std::max(seconds(d_out, grid, iters, 1), 1e-6);
    const int launches = std::max(1, (int)(0.2 / one) + 1);
    std::vector<double> rates;
    for (int r = 0; r < 5; r++) {
        const double s = seconds(d_out, grid, iters, launches);
        rates.push_back((double)grid * 256 * iters * 64.0 * launches / s);
    }
    std::sort(rates.begin(), rates.end());
    printf("{\"bench\": \"mad_u64_u32_rate\", \"lane_mads_per_s\": %.4e, \"min\": %.4e, \"max\": %.4e, \"launches_per_window\": %d, "
           "\"window_s\": %.3f}\n",
           rates[2], rates[0], rates[4], launches, one * launches);
    HIPCHECK(hipFree(d_out));
    return 0;
}
