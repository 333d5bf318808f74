// co_base_kernels.hip — the receiver loops of the Chou-Orlandi base OT (co_kernels.hip: k_co_choices, k_co_decrypt) with the
// scalar multiplication taken from a fixed-base window table (co_table.h) instead of the double-and-add ladder.
//
//   k_co_choices_tab   B_i = b_i * G from G's table (width kCoTabWidthG), + A when the choice is set
//   k_co_decrypt_tab   label_i = SetData(deriveMask(b_i * A, id)[:16] ^ (choice_i ? ct1 : ct0)), b_i * A from A's table
//
// Byte for byte the outputs of the ladder kernels, which stay the yardstick.  One lane = one OT, grid-stride over 64-bit
// indices, a capped grid; the tail behind the multiplication (one inversion, affine output or co_derive_mask) is theirs.
// The ladder's cost is its dependent chain, 256 doublings and 256 issued additions per OT; here it is one plain mixed
// addition per window (pt_mul_tab says why the plain one is exact) and no doubling.  The table is read from global memory
// through L2: the entry of the next window is requested before the addition of the current one, so the gather (four 16-byte
// loads per lane, at most 2^w - 1 distinct entries per wave) waits under about 11 Montgomery products.  The table index is a
// digit of the secret scalar, as the AES tables are indexed by secret bytes; the ladder calls remain for callers who mind.
#include <algorithm>

#include "co_lane.h"
#include "kernels.h"

namespace gc {

namespace {

__global__ __launch_bounds__(kCoTabThreads) void k_co_choices_tab(const CoTabEntry *__restrict__ g_tab, Aff A,
                                                                  const uint4 *__restrict__ scalars,
                                                                  const uint8_t *__restrict__ choice, size_t n,
                                                                  uint4 *__restrict__ points_out) {
    for (size_t i = (size_t)blockIdx.x * kCoTabThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoTabThreads) {
        Jac b = pt_mul_tab<kCoTabWidthG>(load_be_fe(scalars + 2 * i), g_tab, TabLoad());
        Aff add = A;
        add.inf = choice[i] ? 0u : 1u;  // + A, or + infinity: b * G = +-A can be steered, so this addition stays the complete one
        b = pt_madd<true>(b, add);
        Fe x, y;
        pt_to_affine(b, fe_inv(b.z), x, y);
        store_be_fe(points_out + 4 * i, x);
        store_be_fe(points_out + 4 * i + 2, y);
    }
}

__global__ __launch_bounds__(kCoTabThreads) void k_co_decrypt_tab(const CoTabEntry *__restrict__ a_tab,
                                                                  const uint4 *__restrict__ scalars,
                                                                  const uint8_t *__restrict__ choice,
                                                                  const uint4 *__restrict__ ct, size_t n, uint64_t id0,
                                                                  uint4 *__restrict__ labels_out) {
    for (size_t i = (size_t)blockIdx.x * kCoTabThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoTabThreads) {
        co_decrypt_tail(pt_mul_tab<kCoTabWidthA>(load_be_fe(scalars + 2 * i), a_tab, TabLoad()), id0 + i, ct, choice, i,
                        labels_out);
    }
}

unsigned co_tab_grid(size_t n) { return (unsigned)std::min<size_t>(kCoTabGrid, (n + kCoTabThreads - 1) / kCoTabThreads); }

}  // namespace

void launch_co_choices_tab(const CoTabEntry *g_tab, const Aff &a, const uint4 *scalars, const uint8_t *choice, size_t n,
                           uint4 *points_out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_choices_tab, dim3(co_tab_grid(n)), dim3(kCoTabThreads), 0, s, g_tab, a, scalars, choice, n,
                       points_out);
}

void launch_co_decrypt_tab(const CoTabEntry *a_tab, const uint4 *scalars, const uint8_t *choice, const uint4 *ct, size_t n,
                           uint64_t id0, uint4 *labels_out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_decrypt_tab, dim3(co_tab_grid(n)), dim3(kCoTabThreads), 0, s, a_tab, scalars, choice, ct, n, id0,
                       labels_out);
}

}  // namespace gc
