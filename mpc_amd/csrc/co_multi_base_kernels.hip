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

#include "co_multi_table.h"
#include "co_sha256.h"
#include "kernels.h"

namespace gc {

namespace {

constexpr size_t kWindows = co_tab_windows(kCoTabWidthA);
constexpr size_t kEntries = co_tab_entries(kCoTabWidthA);

// 32 big-endian bytes as two 16-byte loads -> limbs
__device__ __forceinline__ Fe load_be_fe(const uint4 *p) {
    const uint4 a = p[0], b = p[1];
    const uint32_t w[kVoleLimbs] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    Fe f;
    vole_from_be_words(w, f.v);
    return f;
}
__device__ __forceinline__ uint4 bswap4(const uint4 v) {
    return make_uint4(__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w));
}

// eight limbs as two 16-byte loads or stores
struct LimbMem {
    __device__ __forceinline__ Fe ld(const uint32_t *p) const {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
        const uint4 a = q[0], b = q[1];
        return Fe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
    }
    __device__ __forceinline__ void st(uint32_t *p, const Fe &f) const {
        uint4 *q = reinterpret_cast<uint4 *>(p);
        q[0] = make_uint4(f.v[0], f.v[1], f.v[2], f.v[3]);
        q[1] = make_uint4(f.v[4], f.v[5], f.v[6], f.v[7]);
    }
};

// one table entry as four 16-byte loads
struct TabLoad {
    __device__ __forceinline__ CoTabEntry operator()(const CoTabEntry *e) const {
        const uint4 *p = reinterpret_cast<const uint4 *>(e);
        const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
        return CoTabEntry{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}};
    }
};

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
            if (j == 0) {
                atomicAdd(status + 2, 1ull);
                atomicMin(status + 3, (unsigned long long)s);
            }
            labels_out[i] = make_uint4(0u, 0u, 0u, 0u);
            continue;
        }
        const Jac sp = pt_mul_tab<kCoTabWidthA>(load_be_fe(scalars + 2 * i), tabs + s * kEntries, TabLoad());
        Fe x, y;
        pt_to_affine(sp, fe_inv(sp.z), x, y);
        uint32_t m[4];
        co_derive_mask(x, y, id0 + j, m);
        const uint4 c = bswap4(ct[2 * i + (choice[i] ? 1 : 0)]);
        // SetData: D0 = BE64(bytes 0..7), D1 = BE64(bytes 8..15)
        labels_out[i] = make_uint4(m[1] ^ c.y, m[0] ^ c.x, m[3] ^ c.w, m[2] ^ c.z);
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
