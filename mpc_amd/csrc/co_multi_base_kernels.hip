// co_multi_base_kernels.hip — the receiver's decrypt of S Chou-Orlandi sessions from per-session fixed-base window tables
// that are BUILT ON THE DEVICE (gcengine.h: gc_co_multi_base_*; co_multi_table.h has the lane bodies and the why).
//
//   k_co_multi_tab_bases    one lane = one session: checks A_s, writes the session's good flag, walks the 252 dependent
//                           doublings once and stores the Jacobian base 2^(4i) * A_s of every window (6 KiB per session)
//   k_co_multi_tab_rows     one lane = one (session, window): the 15 entries of the window from its base, one inversion,
//                           affine Montgomery x, y into the table; Z and prefix products through a 64-byte workspace slot
//   k_co_multi_decrypt_tab  k_co_decrypt_tab (co_base_kernels.hip) with the table of the lane's session, s = i / per
//
// A session's table starts at entry s * 960 and equals co_tab_build<kCoTabWidthA>(A_s) byte for byte.  A bad session (an A_s
// that is not a point of the curve) has no table: its flag is zero, the build writes nothing for it, and the decrypt reads the
// flag BEFORE any table access, gives its OTs zero labels and counts it once, by the lane of its OT 0, as k_co_multi_decrypt
// does.
//
// The two build kernels have no grid-stride loop: each launch's grid is sized to its lanes and the lanes past the end return.
// The rows kernel runs per chunk of kCoMultiTabChunk sessions, so its Z / prefix workspace is that of one chunk whatever S is.
// All index arithmetic is size_t.  No LDS, no scratch; nothing is indexed by a register.
#include <algorithm>

#include "co_lane.h"
#include "co_multi_table.h"
#include "kernels.h"

namespace gc {

namespace {

constexpr size_t kWindows = co_tab_windows(kCoTabWidthA);
constexpr size_t kEntries = co_tab_entries(kCoTabWidthA);

__global__ __launch_bounds__(kCoMultiTabBaseThreads) void k_co_multi_tab_bases(const uint4 *__restrict__ A_all, size_t S,
                                                                               uint32_t *__restrict__ good,
                                                                               CoTabBase *__restrict__ bases) {
    const size_t s = (size_t)blockIdx.x * kCoMultiTabBaseThreads + threadIdx.x;
    if (s >= S) return;
    const bool ok =
        co_multi_tab_bases<kCoTabWidthA>(load_be_fe(A_all + 4 * s), load_be_fe(A_all + 4 * s + 2), s, bases, LimbMem());
    good[s] = ok ? 1u : 0u;
}

// sessions s0 .. s0 + count - 1; zs: the workspace of ONE chunk, indexed from s0
__global__ __launch_bounds__(kCoMultiTabRowThreads) void k_co_multi_tab_rows(const uint32_t *__restrict__ good,
                                                                             const CoTabBase *__restrict__ bases, size_t s0,
                                                                             size_t count, CoTabEntry *tabs, CoTabZ *zs) {
    co_multi_tab_rows_lane<kCoTabWidthA>((size_t)blockIdx.x * kCoMultiTabRowThreads + threadIdx.x, s0, count, good, bases, tabs,
                                         zs, LimbMem());
}

__global__ __launch_bounds__(kCoMultiTabThreads) void k_co_multi_decrypt_tab(const CoTabEntry *__restrict__ tabs,
                                                                             const uint32_t *__restrict__ good,
                                                                             const uint4 *__restrict__ scalars,
                                                                             const uint8_t *__restrict__ choice,
                                                                             const uint4 *__restrict__ ct, size_t n, size_t per,
                                                                             uint64_t id0, uint4 *__restrict__ labels_out,
                                                                             unsigned long long *status) {
    for (size_t i = (size_t)blockIdx.x * kCoMultiTabThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoMultiTabThreads) {
        const size_t s = i / per, j = i - s * per;
        if (!good[s]) {  // before any table access: a bad session has no table
            co_bad_session(status, s, j == 0);
            store_zero(labels_out + i, 1);
            continue;
        }
        co_decrypt_tail(pt_mul_tab<kCoTabWidthA>(load_be_fe(scalars + 2 * i), tabs + s * kEntries, TabLoad()), id0 + j, ct,
                        choice, i, labels_out);
    }
}

}  // namespace

void launch_co_multi_tab_bases(const uint4 *A, size_t S, uint32_t *good, CoTabBase *bases, hipStream_t s) {
    if (S == 0) return;
    const size_t grid = (S + kCoMultiTabBaseThreads - 1) / kCoMultiTabBaseThreads;
    hipLaunchKernelGGL(k_co_multi_tab_bases, dim3((unsigned)grid), dim3(kCoMultiTabBaseThreads), 0, s, A, S, good, bases);
}

void launch_co_multi_tab_rows(const uint32_t *good, const CoTabBase *bases, size_t s0, size_t count, CoTabEntry *tabs,
                              CoTabZ *zs, hipStream_t s) {
    if (count == 0) return;
    const size_t grid = (count * kWindows + kCoMultiTabRowThreads - 1) / kCoMultiTabRowThreads;
    hipLaunchKernelGGL(k_co_multi_tab_rows, dim3((unsigned)grid), dim3(kCoMultiTabRowThreads), 0, s, good, bases, s0, count, tabs,
                       zs);
}

void launch_co_multi_decrypt_tab(const CoTabEntry *tabs, const uint32_t *good, const uint4 *scalars, const uint8_t *choice,
                                 const uint4 *ct, size_t S, size_t per, uint64_t id0, uint4 *labels_out,
                                 unsigned long long *status, hipStream_t s) {
    const size_t n = S * per;
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>(kCoMultiTabGrid, (n + kCoMultiTabThreads - 1) / kCoMultiTabThreads);
    hipLaunchKernelGGL(k_co_multi_decrypt_tab, dim3(grid), dim3(kCoMultiTabThreads), 0, s, tabs, good, scalars, choice, ct, n, per,
                       id0, labels_out, status);
}

}  // namespace gc
