// co_lane.h — what one lane of a Chou-Orlandi kernel does besides its scalar multiplication, once for the four kernel files
// (co_kernels.hip, co_base_kernels.hip, co_multi_kernels.hip, co_multi_base_kernels.hip): the byte order of the boundary, the
// memory access of the window tables, the status block, and the two tails that lead from the product point to the bytes
// of the protocol (ot/co_helpers.go): the sender's encrypt and the receiver's decrypt.  A kernel keeps its loop and its way
// to the session constants and to the product (by value or per lane, ladder or table) and ends in a tail.  The three choices
// kernels keep their five lines behind the product (the complete addition of A, one inversion, two stores) in place: behind a
// function boundary of any shape the complete addition compiled to other code (k_co_multi_choices 210 -> 216 VGPRs, every
// choices kernel 0.3 - 0.6 % slower on the card), in place the three kernels are instruction for instruction what they
// were.  Device code only: the headers that are also compiled for the host (co_table.h, co_multi.h, co_multi_table.h) do
// not depend on this one.  Nothing is indexed by a register.
//
// i is the lane's element in every array of the call (session-major in the multi kernels), id the OT's own number in its
// session: id0 + i for one session, id0 + j in the multi kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "co_sha256.h"
#include "co_table.h"

namespace gc {

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

// eight limbs as two 16-byte loads or stores (the MEM of co_multi_table.h)
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

// one table entry as four 16-byte loads (the LOAD of co_table.h)
struct TabLoad {
    __device__ __forceinline__ CoTabEntry operator()(const CoTabEntry *e) const {
        const uint4 *p = reinterpret_cast<const uint4 *>(e);
        const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
        return CoTabEntry{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}};
    }
};

// The status block.  A point of the peer's that is not on the curve: status[0] += 1, status[1] = min(i)
__device__ __forceinline__ void co_bad_point(unsigned long long *status, size_t i) {
    atomicAdd(status, 1ull);
    atomicMin(status + 1, (unsigned long long)i);
}
// A bad session is counted once, by the lane of its OT 0 alone (first): status[2] += 1, status[3] = min(s)
__device__ __forceinline__ void co_bad_session(unsigned long long *status, size_t s, bool first) {
    if (first) {
        atomicAdd(status + 2, 1ull);
        atomicMin(status + 3, (unsigned long long)s);
    }
}

// The sender's tail (EncryptCOCiphertexts, co_helpers.go:118-134): S = a * B_i, T = S + AaInv,
// ct0 = deriveMask(S, id)[:16] ^ GetData(L0), ct1 = deriveMask(T, id)[:16] ^ GetData(L1).
// ONE inversion serves S and T (Montgomery's trick: 1 / (Zs * Zt)).  T at infinity (B = A, a hostile receiver's choice)
// stands in with Z = 1 and hashes as two empty coordinates, as crypto/elliptic's (0, 0) does in Go.
__device__ __forceinline__ void co_encrypt_tail(const Jac &s, const Aff &ainv, uint64_t id, const uint4 *wires, size_t i,
                                                uint4 *ct) {
    const Jac t = pt_madd<true>(s, ainv);
    // 1 / Zs and 1 / Zt from one inversion; a Z of zero (infinity) stands in as 1 and is selected away in pt_to_affine
    const Fe zs = fe_select(pt_is_inf(s), fe_one(), s.z), zt = fe_select(pt_is_inf(t), fe_one(), t.z);
    const Fe inv = fe_inv(fe_mul(zs, zt));
    Fe sx, sy, tx, ty;
    pt_to_affine(s, fe_mul(inv, zt), sx, sy);
    pt_to_affine(t, fe_mul(inv, zs), tx, ty);
    uint32_t m0[4] = {0u, 0u, 0u, 0u}, m1[4] = {0u, 0u, 0u, 0u};
    GC_P256_NOUNROLL
    for (int h = 0; h < 2; h++) {  // one copy of the hash in the code
        uint32_t m[4];
        co_derive_mask(fe_select(h != 0, tx, sx), fe_select(h != 0, ty, sy), id, m);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            m0[j] = h ? m0[j] : m[j];
            m1[j] = m[j];
        }
    }
    const uint4 l0 = label_be_words(wires[2 * i]), l1 = label_be_words(wires[2 * i + 1]);
    ct[2 * i] = bswap4(make_uint4(m0[0] ^ l0.x, m0[1] ^ l0.y, m0[2] ^ l0.z, m0[3] ^ l0.w));
    ct[2 * i + 1] = bswap4(make_uint4(m1[0] ^ l1.x, m1[1] ^ l1.y, m1[2] ^ l1.z, m1[3] ^ l1.w));
}

// The receiver's tail (DecryptCOCiphertexts, co_helpers.go:202-216): s = b_i * A,
// label_i = SetData(deriveMask(s, id)[:16] ^ (choice_i ? ct1 : ct0))
__device__ __forceinline__ void co_decrypt_tail(const Jac &s, uint64_t id, const uint4 *ct, const uint8_t *choice, size_t i,
                                                uint4 *labels_out) {
    Fe x, y;
    pt_to_affine(s, fe_inv(s.z), x, y);
    uint32_t m[4];
    co_derive_mask(x, y, id, m);
    const uint4 c = bswap4(ct[2 * i + (choice[i] ? 1 : 0)]);
    // SetData: D0 = BE64(bytes 0..7), D1 = BE64(bytes 8..15)
    labels_out[i] = make_uint4(m[1] ^ c.y, m[0] ^ c.x, m[3] ^ c.w, m[2] ^ c.z);
}

}  // namespace gc
