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

#include "co_multi.h"
#include "co_sha256.h"
#include "kernels.h"

namespace gc {

namespace {

// 32 big-endian bytes as two 16-byte loads <-> limbs
__device__ __forceinline__ Fe load_be_fe(const uint4 *p) {
    const uint4 a = p[0], b = p[1];
    const uint32_t w[kVoleLimbs] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    Fe f;
    vole_from_be_words(w, f.v);
    return f;
}
__device__ __forceinline__ void store_be_fe(uint4 *p, const Fe &f) {
    uint32_t w[kVoleLimbs];
    vole_to_be_words(f.v, w);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
__device__ __forceinline__ void store_zero(uint4 *p, int n16) {
#pragma unroll
    for (int j = 0; j < n16; j++) p[j] = make_uint4(0u, 0u, 0u, 0u);
}

// GetData(label) = BE64(D0) || BE64(D1) (label.go:105-108) as four big-endian words, and back (SetData)
__device__ __forceinline__ uint4 label_be_words(const uint4 l) { return make_uint4(l.y, l.x, l.w, l.z); }
__device__ __forceinline__ uint4 bswap4(const uint4 v) {
    return make_uint4(__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w));
}

// one table entry as four 16-byte loads
struct TabLoad {
    __device__ __forceinline__ CoTabEntry operator()(const CoTabEntry *e) const {
        const uint4 *p = reinterpret_cast<const uint4 *>(e);
        const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
        return CoTabEntry{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}};
    }
};

// status[2] += 1 and status[3] = min(s), by the lane of the session's OT 0 alone
__device__ __forceinline__ void bad_session(unsigned long long *status, size_t s, bool first) {
    if (first) {
        atomicAdd(status + 2, 1ull);
        atomicMin(status + 3, (unsigned long long)s);
    }
}

__global__ __launch_bounds__(kCoMultiThreads) void k_co_multi_setup(VoleMod modn, const CoTabEntry *__restrict__ g_tab,
                                                                    const uint4 *__restrict__ a, size_t S,
                                                                    uint4 *__restrict__ A_out, uint4 *__restrict__ AaInv_out,
                                                                    unsigned long long *status) {
    for (size_t s = (size_t)blockIdx.x * kCoMultiThreads + threadIdx.x; s < S; s += (size_t)gridDim.x * kCoMultiThreads) {
        Fe ax, ay, tx, ty;
        if (!co_multi_setup_session<kCoTabWidthG>(load_be_fe(a + 2 * s), modn, g_tab, TabLoad(), ax, ay, tx, ty))
            bad_session(status, s, true);  // (the outputs are zero)
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
                bad_session(status, s, j == 0);
            } else {
                atomicAdd(status, 1ull);
                atomicMin(status + 1, (unsigned long long)i);
            }
            store_zero(ct + 2 * i, 2);
            continue;
        }
        const Jac sp = pt_mul(a, b);
        if (!pt_on_curve(load_be_fe(ainv_all + 4 * s), load_be_fe(ainv_all + 4 * s + 2), ainv)) {
            bad_session(status, s, j == 0);
            store_zero(ct + 2 * i, 2);
            continue;
        }
        const Jac t = pt_madd<true>(sp, ainv);
        // 1 / Zs and 1 / Zt from one inversion; a Z of zero (infinity) stands in as 1 and is selected away in pt_to_affine
        const Fe zs = fe_select(pt_is_inf(sp), fe_one(), sp.z), zt = fe_select(pt_is_inf(t), fe_one(), t.z);
        const Fe inv = fe_inv(fe_mul(zs, zt));
        Fe sx, sy, tx, ty;
        pt_to_affine(sp, fe_mul(inv, zt), sx, sy);
        pt_to_affine(t, fe_mul(inv, zs), tx, ty);
        uint32_t m0[4] = {0u, 0u, 0u, 0u}, m1[4] = {0u, 0u, 0u, 0u};
        GC_P256_NOUNROLL
        for (int h = 0; h < 2; h++) {  // one copy of the hash in the code
            uint32_t m[4];
            co_derive_mask(fe_select(h != 0, tx, sx), fe_select(h != 0, ty, sy), id0 + j, m);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                m0[q] = h ? m0[q] : m[q];
                m1[q] = m[q];
            }
        }
        const uint4 l0 = label_be_words(wires[2 * i]), l1 = label_be_words(wires[2 * i + 1]);
        ct[2 * i] = bswap4(make_uint4(m0[0] ^ l0.x, m0[1] ^ l0.y, m0[2] ^ l0.z, m0[3] ^ l0.w));
        ct[2 * i + 1] = bswap4(make_uint4(m1[0] ^ l1.x, m1[1] ^ l1.y, m1[2] ^ l1.z, m1[3] ^ l1.w));
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
            bad_session(status, s, j == 0);
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
            bad_session(status, s, j == 0);
            store_zero(labels_out + i, 1);
            continue;
        }
        const Jac sp = pt_mul(sc_reduce(load_be_fe(scalars + 2 * i)), A);
        Fe x, y;
        pt_to_affine(sp, fe_inv(sp.z), x, y);
        uint32_t m[4];
        co_derive_mask(x, y, id0 + j, m);
        const uint4 c = bswap4(ct[2 * i + (choice[i] ? 1 : 0)]);
        // SetData: D0 = BE64(bytes 0..7), D1 = BE64(bytes 8..15)
        labels_out[i] = make_uint4(m[1] ^ c.y, m[0] ^ c.x, m[3] ^ c.w, m[2] ^ c.z);
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
