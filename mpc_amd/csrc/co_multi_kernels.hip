// co_multi_kernels.hip — the Chou-Orlandi base OT for S independent sessions in one launch (gcengine.h: gc_co_multi_*).
// The loops of co_kernels.hip and co_base_kernels.hip with the session constants read per lane instead of passed by value:
//
//   k_co_multi_setup     one lane = one SESSION: A_s = a_s * G and AaInv_s = -(a_s^2 mod N) * G from G's table (co_multi.h)
//   k_co_multi_encrypt   k_co_encrypt with a_s and AaInv_s of the lane's session
//   k_co_multi_choices   k_co_choices_tab (b_i * G from G's table) with A_s of the lane's session
//   k_co_multi_decrypt   k_co_decrypt (the ladder) with A_s of the lane's session
//
// Layout: session-major, OT j of session s is element i = s * per + j, s = i / per, and its id is id0 + j (Go numbers every
// session from 0).  One lane = one OT, grid-stride over 64-bit indices, 256-thread workgroups, a capped grid; nothing is
// indexed by a register.  A session's constants are loaded and CHECKED by every lane of it (pt_on_curve, 6 products next to
// the thousands of a scalar multiplication): a bad session (a_s = 0 mod N, an AaInv_s or A_s that is not a point of the
// curve) gets zero bytes in all its outputs and is counted once, by the lane of its OT 0; its OTs are not counted as bad
// points.
//
// What diverges in a wave.  In k_co_encrypt the walk over the bits of a is uniform; here it is pt_mul with the lane's scalar,
// as the receiver ladders always were: the addition runs under the execution mask and is skipped when no lane of the wave
// has the bit set.  A wave that sits in one session (per a multiple of 64) therefore skips the additions of a_s's zero bits
// as k_co_encrypt does; a wave that spans sessions issues an addition wherever any of them has the bit.  AaInv_s is loaded
// behind the ladder, so that it does not sit in registers through it.
#include <algorithm>

#include "co_lane.h"
#include "co_multi.h"
#include "kernels.h"

namespace gc {

namespace {

__global__ __launch_bounds__(kCoMultiThreads) void k_co_multi_setup(VoleMod modn, const CoTabEntry *__restrict__ g_tab,
                                                                    const uint4 *__restrict__ a, size_t S,
                                                                    uint4 *__restrict__ A_out, uint4 *__restrict__ AaInv_out,
                                                                    unsigned long long *status) {
    for (size_t s = (size_t)blockIdx.x * kCoMultiThreads + threadIdx.x; s < S; s += (size_t)gridDim.x * kCoMultiThreads) {
        Fe ax, ay, tx, ty;
        if (!co_multi_setup_session<kCoTabWidthG>(load_be_fe(a + 2 * s), modn, g_tab, TabLoad(), ax, ay, tx, ty))
            co_bad_session(status, s, true);  // (the outputs are zero)
        store_be_fe(A_out + 4 * s, ax);
        store_be_fe(A_out + 4 * s + 2, ay);
        store_be_fe(AaInv_out + 4 * s, tx);
        store_be_fe(AaInv_out + 4 * s + 2, ty);
    }
}

__global__ __launch_bounds__(kCoMultiThreads) void k_co_multi_encrypt(const uint4 *__restrict__ a_all,
                                                                      const uint4 *__restrict__ ainv_all,
                                                                      const uint4 *__restrict__ points,
                                                                      const uint4 *__restrict__ wires, size_t n, size_t per,
                                                                      uint64_t id0, uint4 *__restrict__ ct,
                                                                      unsigned long long *status) {
    // The pointers that are used behind the ladder alone would wait through it in scalar registers, next to the carry masks
    // of the limb arithmetic (a pair of scalar registers each): that ran the kernel out of them (two spilled).  Held in
    // vector registers instead, as k_co_decrypt holds A.
    asm volatile("" : "+v"(ainv_all), "+v"(wires), "+v"(ct), "+v"(status));
    for (size_t i = (size_t)blockIdx.x * kCoMultiThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoMultiThreads) {
        const size_t s = i / per, j = i - s * per;
        const Fe a = sc_reduce(load_be_fe(a_all + 2 * s));
        Aff b, ainv;
        const bool b_ok = pt_on_curve(load_be_fe(points + 4 * i), load_be_fe(points + 4 * i + 2), b);
        if (!b_ok || fe_is_zero(a)) {
            // no ladder for this lane: whether the session or the point is to blame is decided here (a bad session wins)
            if (fe_is_zero(a) || !pt_on_curve(load_be_fe(ainv_all + 4 * s), load_be_fe(ainv_all + 4 * s + 2), ainv)) {
                co_bad_session(status, s, j == 0);
            } else {
                co_bad_point(status, i);
            }
            store_zero(ct + 2 * i, 2);
            continue;
        }
        const Jac sp = pt_mul(a, b);
        if (!pt_on_curve(load_be_fe(ainv_all + 4 * s), load_be_fe(ainv_all + 4 * s + 2), ainv)) {
            co_bad_session(status, s, j == 0);
            store_zero(ct + 2 * i, 2);
            continue;
        }
        co_encrypt_tail(sp, ainv, id0 + j, wires, i, ct);
    }
}

__global__ __launch_bounds__(kCoMultiThreads) void k_co_multi_choices(const CoTabEntry *__restrict__ g_tab,
                                                                      const uint4 *__restrict__ A_all,
                                                                      const uint4 *__restrict__ scalars,
                                                                      const uint8_t *__restrict__ choice, size_t n, size_t per,
                                                                      uint4 *__restrict__ points_out,
                                                                      unsigned long long *status) {
    for (size_t i = (size_t)blockIdx.x * kCoMultiThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoMultiThreads) {
        const size_t s = i / per, j = i - s * per;
        Jac b = pt_mul_tab<kCoTabWidthG>(load_be_fe(scalars + 2 * i), g_tab, TabLoad());
        Aff add;
        if (!pt_on_curve(load_be_fe(A_all + 4 * s), load_be_fe(A_all + 4 * s + 2), add)) {  // ensureOnCurve(Ax, Ay)
            co_bad_session(status, s, j == 0);
            store_zero(points_out + 4 * i, 4);
            continue;
        }
        add.inf = choice[i] ? 0u : 1u;  // + A_s, or + infinity: b * G = +-A_s can be steered, so this addition stays the complete one
        b = pt_madd<true>(b, add);
        Fe x, y;
        pt_to_affine(b, fe_inv(b.z), x, y);
        store_be_fe(points_out + 4 * i, x);
        store_be_fe(points_out + 4 * i + 2, y);
    }
}

__global__ __launch_bounds__(kCoMultiThreads) void k_co_multi_decrypt(const uint4 *__restrict__ A_all,
                                                                      const uint4 *__restrict__ scalars,
                                                                      const uint8_t *__restrict__ choice,
                                                                      const uint4 *__restrict__ ct, size_t n, size_t per,
                                                                      uint64_t id0, uint4 *__restrict__ labels_out,
                                                                      unsigned long long *status) {
    for (size_t i = (size_t)blockIdx.x * kCoMultiThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoMultiThreads) {
        const size_t s = i / per, j = i - s * per;
        Aff A;
        if (!pt_on_curve(load_be_fe(A_all + 4 * s), load_be_fe(A_all + 4 * s + 2), A)) {  // ensureOnCurve(Ax, Ay)
            co_bad_session(status, s, j == 0);
            store_zero(labels_out + i, 1);
            continue;
        }
        co_decrypt_tail(pt_mul(sc_reduce(load_be_fe(scalars + 2 * i)), A), id0 + j, ct, choice, i, labels_out);
    }
}

unsigned co_multi_grid(size_t n) {
    return (unsigned)std::min<size_t>(kCoMultiGrid, (n + kCoMultiThreads - 1) / kCoMultiThreads);
}

}  // namespace

void launch_co_multi_setup(const VoleMod &modn, const CoTabEntry *g_tab, const uint4 *a, size_t S, uint4 *A_out,
                           uint4 *AaInv_out, unsigned long long *status, hipStream_t s) {
    if (S == 0) return;
    hipLaunchKernelGGL(k_co_multi_setup, dim3(co_multi_grid(S)), dim3(kCoMultiThreads), 0, s, modn, g_tab, a, S, A_out,
                       AaInv_out, status);
}

void launch_co_multi_encrypt(const uint4 *a, const uint4 *ainv, const uint4 *points, const uint4 *wires, size_t S, size_t per,
                             uint64_t id0, uint4 *ct, unsigned long long *status, hipStream_t s) {
    const size_t n = S * per;
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_multi_encrypt, dim3(co_multi_grid(n)), dim3(kCoMultiThreads), 0, s, a, ainv, points, wires, n, per,
                       id0, ct, status);
}

void launch_co_multi_choices(const CoTabEntry *g_tab, const uint4 *A, const uint4 *scalars, const uint8_t *choice, size_t S,
                             size_t per, uint4 *points_out, unsigned long long *status, hipStream_t s) {
    const size_t n = S * per;
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_multi_choices, dim3(co_multi_grid(n)), dim3(kCoMultiThreads), 0, s, g_tab, A, scalars, choice, n,
                       per, points_out, status);
}

void launch_co_multi_decrypt(const uint4 *A, const uint4 *scalars, const uint8_t *choice, const uint4 *ct, size_t S,
                             size_t per, uint64_t id0, uint4 *labels_out, unsigned long long *status, hipStream_t s) {
    const size_t n = S * per;
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_multi_decrypt, dim3(co_multi_grid(n)), dim3(kCoMultiThreads), 0, s, A, scalars, choice, ct, n, per,
                       id0, labels_out, status);
}

}  // namespace gc
