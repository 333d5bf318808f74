// p256.h — NIST P-256 field and point arithmetic for the Chou-Orlandi base OT (co_kernels.hip, co_engine.cpp) and their host
// checks.  Plain C++ with no HIP types, as vole_mod.h on which it builds, so that a host-only test can compile it with g++
// (tests/test_p256_host.py).  The reference does this work with crypto/elliptic on math/big affine points
// (ot/co_helpers.go:87-88, :122-123, :157-159, :203: ScalarBaseMult, ScalarMult, Add, IsOnCurve).
//
// Field elements (Fe) are eight 32-bit limbs, least significant first, below p and in Montgomery form (x * 2^256 mod p):
// every product is vole_mont_mul with the constants of p (p256_field(): n0 = 1; the compiler folds the sparse limbs of p into
// the unrolled reduction).  Points are Jacobian (X, Y, Z) with x = X / Z^2, y = Y / Z^3; Z = 0 is the point at infinity.
//   pt_dbl       dbl-2001-b (a = -3), 3M + 5S; keeps infinity (Z3 = (Y + Z)^2 - Y^2 - Z^2 = 0)
//   pt_madd      Jacobian + affine, 8M + 3S.  Either operand at infinity gives the other; equal x with opposite y gives
//                Z3 = Z1 * H = 0, infinity, by itself.  COMPLETE: equal points take the doubling path (a branch that no lane
//                takes unless it must).  Without COMPLETE that one case is the caller's to exclude: the ladder below does.
//   pt_mul       left-to-right double-and-add over the 256 bits of a scalar k < N on a point of order N.  At every addition
//                the accumulator is 2j * P with 2j + 1 <= k < N, so 2j = +-1 mod N cannot be: the plain pt_madd is exact.
//   fe_inv       x^(p - 2) by a fixed chain, 255 squarings and 12 products; 0 gives 0
//   pt_on_curve  0 <= x, y < p and y^2 = x^3 - 3x + b: an encoding >= p is refused, not reduced, and so is (0, 0)
//   sc_reduce    a scalar below 2^256 mod N by one conditional subtraction (N > 2^255)
#pragma once

#include "vole_mod.h"

// Everything here is inlined into its kernel: a call would pass the operands through memory (scratch on the device).
#if defined(__clang__)
#define GC_P256_NOUNROLL _Pragma("clang loop unroll(disable)")
#define GC_P256_FN GC_VOLE_HD inline __attribute__((always_inline))
#define GC_P256_FLAT [[clang::always_inline]]
#else
#define GC_P256_NOUNROLL
#define GC_P256_FN GC_VOLE_HD inline
#define GC_P256_FLAT
#endif

namespace gc {

struct Fe {
    uint32_t v[kVoleLimbs];
};
struct Jac {
    Fe x, y, z;
};
// affine, Montgomery form; inf != 0: the point at infinity (x, y ignored)
struct Aff {
    Fe x, y;
    uint32_t inf;
};

// the constants of p = 2^256 - 2^224 + 2^192 + 2^96 - 1 (checked against vole_mod_init by the host test)
GC_P256_FN VoleMod p256_field() {
    const VoleMod m = {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 1u, 0xffffffffu},
                       {3u, 0u, 0xffffffffu, 0xfffffffbu, 0xfffffffeu, 0xffffffffu, 0xfffffffdu, 4u},
                       1u};
    return m;
}
GC_P256_FN Fe fe_zero() { return Fe{{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}}; }
GC_P256_FN Fe fe_plain_one() { return Fe{{1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}}; }
// 1 in Montgomery form: 2^256 mod p
GC_P256_FN Fe fe_one() { return Fe{{1u, 0u, 0u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffffeu, 0u}}; }
// plain values
GC_P256_FN Fe p256_b() {
    return Fe{{0x27d2604bu, 0x3bce3c3eu, 0xcc53b0f6u, 0x651d06b0u, 0x769886bcu, 0xb3ebbd55u, 0xaa3a93e7u, 0x5ac635d8u}};
}
GC_P256_FN Fe p256_gx() {
    return Fe{{0xd898c296u, 0xf4a13945u, 0x2deb33a0u, 0x77037d81u, 0x63a440f2u, 0xf8bce6e5u, 0xe12c4247u, 0x6b17d1f2u}};
}
GC_P256_FN Fe p256_gy() {
    return Fe{{0x37bf51f5u, 0xcbb64068u, 0x6b315eceu, 0x2bce3357u, 0x7c0f9e16u, 0x8ee7eb4au, 0xfe1a7f9bu, 0x4fe342e2u}};
}
GC_P256_FN Fe p256_n() {
    return Fe{{0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0u, 0xffffffffu}};
}

GC_P256_FN Fe fe_mul(const Fe &a, const Fe &b) {
    const VoleMod m = p256_field();
    Fe r;
    GC_P256_FLAT vole_mont_mul(a.v, b.v, m, r.v);
    return r;
}
GC_P256_FN Fe fe_sqr(const Fe &a) { return fe_mul(a, a); }
GC_P256_FN Fe fe_add(const Fe &a, const Fe &b) {
    const VoleMod m = p256_field();
    Fe r;
    GC_P256_FLAT vole_add_mod(a.v, b.v, m, r.v);
    return r;
}
// (a - b) mod p, a, b < p
GC_P256_FN Fe fe_sub(const Fe &a, const Fe &b) {
    const VoleMod m = p256_field();
    uint32_t d[kVoleLimbs];
    uint64_t borrow = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) {
        const uint64_t s = (uint64_t)a.v[j] - b.v[j] - borrow;
        d[j] = (uint32_t)s;
        borrow = (s >> 32) & 1;
    }
    const uint32_t mask = 0u - (uint32_t)borrow;  // a < b: add p back
    Fe r;
    uint64_t c = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) {
        const uint64_t s = (uint64_t)d[j] + (m.p[j] & mask) + c;
        r.v[j] = (uint32_t)s;
        c = s >> 32;
    }
    return r;
}
GC_P256_FN Fe fe_neg(const Fe &a) { return fe_sub(fe_zero(), a); }
GC_P256_FN bool fe_is_zero(const Fe &a) {
    uint32_t o = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) o |= a.v[j];
    return o == 0;
}
GC_P256_FN bool fe_eq(const Fe &a, const Fe &b) {
    uint32_t o = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) o |= a.v[j] ^ b.v[j];
    return o == 0;
}
// c ? a : b
GC_P256_FN Fe fe_select(bool c, const Fe &a, const Fe &b) {
    Fe r;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) r.v[j] = c ? a.v[j] : b.v[j];
    return r;
}
// plain value < p  <->  Montgomery form
GC_P256_FN Fe fe_to_mont(const Fe &a) {
    const VoleMod m = p256_field();
    Fe r2, r;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) r2.v[j] = m.r2[j];
    GC_P256_FLAT vole_mont_mul(a.v, r2.v, m, r.v);
    return r;
}
GC_P256_FN Fe fe_from_mont(const Fe &a) { return fe_mul(a, fe_plain_one()); }
// a plain value is below p
GC_P256_FN bool fe_below_p(const Fe &a) {
    const VoleMod m = p256_field();
    uint64_t borrow = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) borrow = (((uint64_t)a.v[j] - m.p[j] - borrow) >> 32) & 1;
    return borrow != 0;
}

GC_P256_FN Fe fe_sqr_n(Fe a, int n) {
    GC_P256_NOUNROLL
    for (int i = 0; i < n; i++) a = fe_sqr(a);
    return a;
}
// a^(p - 2): p - 2 = ffffffff 00000001 00000000 00000000 00000000 ffffffff ffffffff fffffffd
GC_P256_FN Fe fe_inv(const Fe &a) {
    const Fe x2 = fe_mul(fe_sqr(a), a);            // 2^2 - 1
    const Fe x3 = fe_mul(fe_sqr(x2), a);           // 2^3 - 1
    const Fe x6 = fe_mul(fe_sqr_n(x3, 3), x3);     // 2^6 - 1
    const Fe x12 = fe_mul(fe_sqr_n(x6, 6), x6);    // 2^12 - 1
    const Fe x15 = fe_mul(fe_sqr_n(x12, 3), x3);   // 2^15 - 1
    const Fe x30 = fe_mul(fe_sqr_n(x15, 15), x15); // 2^30 - 1
    const Fe x32 = fe_mul(fe_sqr_n(x30, 2), x2);   // 2^32 - 1
    Fe t = fe_mul(fe_sqr_n(x32, 32), a);           // ffffffff 00000001
    t = fe_mul(fe_sqr_n(t, 128), x32);             // ... 00000000 00000000 00000000 ffffffff
    t = fe_mul(fe_sqr_n(t, 32), x32);              // ... ffffffff
    t = fe_mul(fe_sqr_n(t, 30), x30);              // ... 3fffffff
    return fe_mul(fe_sqr_n(t, 2), a);              // ... fffffffd
}

GC_P256_FN Jac pt_infinity() { return Jac{fe_one(), fe_one(), fe_zero()}; }
GC_P256_FN bool pt_is_inf(const Jac &p) { return fe_is_zero(p.z); }
GC_P256_FN Jac pt_select(bool c, const Jac &a, const Jac &b) {
    return Jac{fe_select(c, a.x, b.x), fe_select(c, a.y, b.y), fe_select(c, a.z, b.z)};
}
GC_P256_FN Jac pt_from_aff(const Aff &q) {
    return Jac{q.x, q.y, q.inf ? fe_zero() : fe_one()};
}

GC_P256_FN Jac pt_dbl(const Jac &p) {
    const Fe delta = fe_sqr(p.z), gamma = fe_sqr(p.y), beta = fe_mul(p.x, gamma);
    const Fe t = fe_mul(fe_sub(p.x, delta), fe_add(p.x, delta));
    const Fe alpha = fe_add(fe_add(t, t), t);
    const Fe beta2 = fe_add(beta, beta), beta4 = fe_add(beta2, beta2);
    Jac r;
    r.x = fe_sub(fe_sqr(alpha), fe_add(beta4, beta4));
    r.z = fe_sub(fe_sub(fe_sqr(fe_add(p.y, p.z)), gamma), delta);
    const Fe g2 = fe_sqr(gamma), g4 = fe_add(g2, g2), g8 = fe_add(g4, g4);
    r.y = fe_sub(fe_mul(alpha, fe_sub(beta4, r.x)), fe_add(g8, g8));
    return r;
}

template <bool COMPLETE>
GC_P256_FN Jac pt_madd(const Jac &p, const Aff &q) {
    const Fe z1z1 = fe_sqr(p.z);
    const Fe u2 = fe_mul(q.x, z1z1), s2 = fe_mul(q.y, fe_mul(p.z, z1z1));
    const Fe h = fe_sub(u2, p.x), r = fe_sub(s2, p.y);
    const Fe hh = fe_sqr(h), hhh = fe_mul(h, hh), v = fe_mul(p.x, hh);
    Jac o;
    o.x = fe_sub(fe_sub(fe_sqr(r), hhh), fe_add(v, v));
    o.y = fe_sub(fe_mul(r, fe_sub(v, o.x)), fe_mul(p.y, hhh));
    o.z = fe_mul(p.z, h);
    const bool p_inf = pt_is_inf(p), q_inf = q.inf != 0;
    if (COMPLETE) {
        if (!p_inf && !q_inf && fe_is_zero(h) && fe_is_zero(r)) o = pt_dbl(p);
    }
    o = pt_select(p_inf, pt_from_aff(q), o);
    return pt_select(q_inf, p, o);
}

// k * q for a scalar k < N (limbs, least significant first) and a point q of order N (or infinity)
GC_P256_FN Jac pt_mul(const Fe &k, const Aff &q) {
    Fe s = k;
    Jac acc = pt_infinity();
    GC_P256_NOUNROLL
    for (int i = 0; i < 256; i++) {
        acc = pt_dbl(acc);
        if (s.v[kVoleLimbs - 1] >> 31) acc = pt_madd<false>(acc, q);
        GC_VOLE_UNROLL
        for (int j = kVoleLimbs - 1; j > 0; j--) s.v[j] = (s.v[j] << 1) | (s.v[j - 1] >> 31);
        s.v[0] <<= 1;
    }
    return acc;
}

// (X, Y, Z), 1 / Z -> plain affine coordinates; infinity -> (0, 0), crypto/elliptic's encoding
GC_P256_FN void pt_to_affine(const Jac &p, const Fe &zinv, Fe &x, Fe &y) {
    const Fe zi2 = fe_sqr(zinv);
    const bool inf = pt_is_inf(p);
    x = fe_select(inf, fe_zero(), fe_from_mont(fe_mul(p.x, zi2)));
    y = fe_select(inf, fe_zero(), fe_from_mont(fe_mul(p.y, fe_mul(zi2, zinv))));
}

// plain coordinates (any values below 2^256) -> the point in Montgomery form; false: not an affine point of the curve
GC_P256_FN bool pt_on_curve(const Fe &x, const Fe &y, Aff &q) {
    const bool in_range = fe_below_p(x) && fe_below_p(y);
    q.x = fe_to_mont(x);  // (a value >= p is reduced by the product; the point is refused all the same)
    q.y = fe_to_mont(y);
    q.inf = 0;
    const Fe x3 = fe_mul(fe_sqr(q.x), q.x);
    const Fe rhs = fe_add(fe_sub(x3, fe_add(fe_add(q.x, q.x), q.x)), fe_to_mont(p256_b()));
    return in_range && fe_eq(fe_sqr(q.y), rhs);
}

// any scalar below 2^256 mod N
GC_P256_FN Fe sc_reduce(const Fe &k) {
    const Fe n = p256_n();
    Fe r;
    GC_P256_FLAT vole_cond_sub(k.v, 0, n.v, r.v);
    return r;
}

}  // namespace gc
