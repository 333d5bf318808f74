// co_kernels.hip — CDNA4 kernels of the Chou-Orlandi base OT on P-256 (ot/co.go, ot/co_helpers.go): the three per-OT loops.
//
//   k_co_encrypt   EncryptCOCiphertexts (co_helpers.go:118-134): IsOnCurve(B_i), S = a * B_i, T = S + AaInv,
//                  ct0 = deriveMask(S, id)[:16] ^ GetData(L0), ct1 = deriveMask(T, id)[:16] ^ GetData(L1)
//   k_co_choices   BuildCOChoices (:150-166): B_i = b_i * G, + A when the choice is set
//   k_co_decrypt   DecryptCOCiphertexts (:202-216): label_i = SetData(deriveMask(b_i * A, id)[:16] ^ (choice_i ? ct1 : ct0))
//
// One lane = one OT, grid-stride over 64-bit indices, 256-thread workgroups, a capped grid.  The curve arithmetic is p256.h,
// the hash co_sha256.h, and what a lane does behind its multiplication (byte order, status, the encrypt and decrypt tails) is co_lane.h, shared with the table
// and the multi-session kernels; nothing is indexed by a register, so nothing lives in scratch.  Points cross the boundary
// as gc_p256_point (x, y: 32 bytes big-endian each; 64 zero bytes = infinity), scalars as 32 bytes big-endian, any value
// below 2^256, taken mod N.
//
// In k_co_encrypt the scalar a is a kernel argument: the walk over its bits (pt_mul) is uniform control flow, every lane of
// the grid doubles and adds in step.  In the receiver kernels the base is uniform (G, A) and the scalar is the lane's, so the
// lanes of a wave add on different steps (about half of them on each): the addition runs under the execution mask.
// The sender shares ONE inversion between S and T (Montgomery's trick: 1 / (Zs * Zt)); T at infinity (B = A, a hostile
// receiver's choice) stands in with Z = 1 and hashes as two empty coordinates, as crypto/elliptic's (0, 0) does in Go.
#include <algorithm>

#include "co_lane.h"
#include "kernels.h"

namespace gc {

namespace {

// status[0] += bad points, status[1] = min(lowest bad index)
__global__ __launch_bounds__(kCoThreads) void k_co_encrypt(CoSender ses, const uint4 *__restrict__ points,
                                                           const uint4 *__restrict__ wires, size_t n, uint64_t id0,
                                                           uint4 *__restrict__ ct, unsigned long long *status) {
    for (size_t i = (size_t)blockIdx.x * kCoThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoThreads) {
        Aff b;
        if (!pt_on_curve(load_be_fe(points + 4 * i), load_be_fe(points + 4 * i + 2), b)) {
            co_bad_point(status, i);
            store_zero(ct + 2 * i, 2);
            continue;
        }
        Fe a;
#pragma unroll
        for (int j = 0; j < kVoleLimbs; j++) a.v[j] = ses.a[j];
        co_encrypt_tail(pt_mul(a, b), ses.ainv, id0 + i, wires, i, ct);
    }
}

__global__ __launch_bounds__(kCoThreads) void k_co_choices(CoBase base, const uint4 *__restrict__ scalars,
                                                           const uint8_t *__restrict__ choice, size_t n,
                                                           uint4 *__restrict__ points_out) {
    for (size_t i = (size_t)blockIdx.x * kCoThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoThreads) {
        Jac b = pt_mul(sc_reduce(load_be_fe(scalars + 2 * i)), base.g);
        Aff add = base.a;
        add.inf = choice[i] ? 0u : 1u;  // + A, or + infinity: b * G = +-A is possible, so the addition is the complete one
        b = pt_madd<true>(b, add);
        Fe x, y;
        pt_to_affine(b, fe_inv(b.z), x, y);
        store_be_fe(points_out + 4 * i, x);
        store_be_fe(points_out + 4 * i + 2, y);
    }
}

__global__ __launch_bounds__(kCoThreads) void k_co_decrypt(Aff A, const uint4 *__restrict__ scalars,
                                                           const uint8_t *__restrict__ choice, const uint4 *__restrict__ ct,
                                                           size_t n, uint64_t id0, uint4 *__restrict__ labels_out) {
    // A is uniform and would sit in 16 scalar registers through the whole ladder, next to the carry masks of the limb
    // arithmetic (a pair of scalar registers each): that ran the kernel out of them.  Held in vector registers instead.
#pragma unroll
    for (int j = 0; j < kVoleLimbs; j++) asm volatile("" : "+v"(A.x.v[j]), "+v"(A.y.v[j]));
    for (size_t i = (size_t)blockIdx.x * kCoThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kCoThreads) {
        co_decrypt_tail(pt_mul(sc_reduce(load_be_fe(scalars + 2 * i)), A), id0 + i, ct, choice, i, labels_out);
    }
}

unsigned co_grid(size_t n) { return (unsigned)std::min<size_t>(kCoGrid, (n + kCoThreads - 1) / kCoThreads); }

}  // namespace

void launch_co_encrypt(const CoSender &ses, const uint4 *points, const uint4 *wires, size_t n, uint64_t id0, uint4 *ct,
                       unsigned long long *status, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_encrypt, dim3(co_grid(n)), dim3(kCoThreads), 0, s, ses, points, wires, n, id0, ct, status);
}

void launch_co_choices(const CoBase &base, const uint4 *scalars, const uint8_t *choice, size_t n, uint4 *points_out,
                       hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_choices, dim3(co_grid(n)), dim3(kCoThreads), 0, s, base, scalars, choice, n, points_out);
}

void launch_co_decrypt(const CoBase &base, const uint4 *scalars, const uint8_t *choice, const uint4 *ct, size_t n, uint64_t id0,
                       uint4 *labels_out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_co_decrypt, dim3(co_grid(n)), dim3(kCoThreads), 0, s, base.a, scalars, choice, ct, n, id0, labels_out);
}

}  // namespace gc
