// vole_mod.h — 256-bit arithmetic mod an odd p (3 <= p < 2^256) for the VOLE kernels (vole_kernels.hip) and their host
// checks.  Plain C++ with no HIP types, so that a host-only test can compile it with g++ (tests/test_vole_mod.py).
//
// Values are eight 32-bit limbs, least significant first.  Every operation is Montgomery arithmetic with R = 2^256, one
// code path for every supported modulus, tiny ones included:
//   n0 = -p^-1 mod 2^32, r2 = R^2 mod p          (vole_mod_init, host)
//   REDC(a * b) = a * b * R^-1 mod p             (vole_mont_mul: a < 2^256, b < p -> the CIOS sum stays below 2p, so one
//                                                 conditional subtraction ends it)
//   v mod p     = REDC(REDC(v * r2) * 1)         (vole_reduce, any v < 2^256; for p >= 2^255, v < 2p: one conditional
//                                                 subtraction instead)
//   x * y mod p = REDC(x * REDC(y * r2))         (vole_mul_mod, any x, y < 2^256)
// The reference does the same work with math/big (vole/vole.go:58-97, 182-187): Mod, Mul then Mod, Add then Mod.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GC_VOLE_HD __host__ __device__
#else
#define GC_VOLE_HD
#endif
#if defined(__clang__)
#define GC_VOLE_UNROLL _Pragma("unroll")
#else
#define GC_VOLE_UNROLL
#endif

namespace gc {

constexpr int kVoleLimbs = 8;

// the constants of one modulus; passed to the kernels by value, so they are uniform across the grid
struct VoleMod {
    uint32_t p[kVoleLimbs];
    uint32_t r2[kVoleLimbs];
    uint32_t n0;
};

// big-endian 32 bytes <-> limbs.  The word form takes the eight 32-bit words as a little-endian load of the 32 bytes
// delivers them (word i = bytes 4i..4i+3), which is how the kernels read and write them.
GC_VOLE_HD inline void vole_from_be_words(const uint32_t (&w)[kVoleLimbs], uint32_t (&v)[kVoleLimbs]) {
    for (int i = 0; i < kVoleLimbs; i++) v[kVoleLimbs - 1 - i] = __builtin_bswap32(w[i]);
}
GC_VOLE_HD inline void vole_to_be_words(const uint32_t (&v)[kVoleLimbs], uint32_t (&w)[kVoleLimbs]) {
    for (int i = 0; i < kVoleLimbs; i++) w[i] = __builtin_bswap32(v[kVoleLimbs - 1 - i]);
}
GC_VOLE_HD inline void vole_load_be(const uint8_t *b, uint32_t (&v)[kVoleLimbs]) {
    for (int i = 0; i < kVoleLimbs; i++)
        v[kVoleLimbs - 1 - i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) |
                                b[4 * i + 3];
}
GC_VOLE_HD inline void vole_store_be(const uint32_t (&v)[kVoleLimbs], uint8_t *b) {
    for (int i = 0; i < kVoleLimbs; i++) {
        const uint32_t x = v[kVoleLimbs - 1 - i];
        b[4 * i] = (uint8_t)(x >> 24);
        b[4 * i + 1] = (uint8_t)(x >> 16);
        b[4 * i + 2] = (uint8_t)(x >> 8);
        b[4 * i + 3] = (uint8_t)x;
    }
}

// v = t - p when hi (a 257th bit of t) is set or t >= p, else v = t; branch-free (selects only)
GC_VOLE_HD inline void vole_cond_sub(const uint32_t (&t)[kVoleLimbs], uint32_t hi, const uint32_t (&p)[kVoleLimbs],
                                     uint32_t (&v)[kVoleLimbs]) {
    uint32_t d[kVoleLimbs];
    uint64_t borrow = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) {
        const uint64_t s = (uint64_t)t[j] - p[j] - borrow;
        d[j] = (uint32_t)s;
        borrow = (s >> 32) & 1;
    }
    const bool take = hi != 0 || borrow == 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) v[j] = take ? d[j] : t[j];
}

// out = a * b * 2^-256 mod p (CIOS), a < 2^256, b < p; out may alias neither input
GC_VOLE_HD inline void vole_mont_mul(const uint32_t (&a)[kVoleLimbs], const uint32_t (&b)[kVoleLimbs], const VoleMod &m,
                                     uint32_t (&out)[kVoleLimbs]) {
    uint32_t t[kVoleLimbs], t8 = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) t[j] = 0;
    GC_VOLE_UNROLL
    for (int i = 0; i < kVoleLimbs; i++) {
        // t += a * b[i]   (t < a + p < 2^257 on entry, so t + a * b[i] < 2^289: t8 and the carry c9 hold it)
        uint64_t c = 0;
        GC_VOLE_UNROLL
        for (int j = 0; j < kVoleLimbs; j++) {
            const uint64_t s = (uint64_t)a[j] * b[i] + t[j] + c;
            t[j] = (uint32_t)s;
            c = s >> 32;
        }
        const uint64_t s8 = (uint64_t)t8 + c;
        t8 = (uint32_t)s8;
        const uint32_t c9 = (uint32_t)(s8 >> 32);
        // t = (t + q * p) / 2^32 with q = t[0] * n0 mod 2^32: the low limb cancels
        const uint32_t q = t[0] * m.n0;
        c = ((uint64_t)q * m.p[0] + t[0]) >> 32;
        GC_VOLE_UNROLL
        for (int j = 1; j < kVoleLimbs; j++) {
            const uint64_t s = (uint64_t)q * m.p[j] + t[j] + c;
            t[j - 1] = (uint32_t)s;
            c = s >> 32;
        }
        const uint64_t s7 = (uint64_t)t8 + c;
        t[kVoleLimbs - 1] = (uint32_t)s7;
        t8 = c9 + (uint32_t)(s7 >> 32);
    }
    vole_cond_sub(t, t8, m.p, out);  // t < 2p
}

// out = v mod p, any v < 2^256
GC_VOLE_HD inline void vole_reduce(const uint32_t (&v)[kVoleLimbs], const VoleMod &m, uint32_t (&out)[kVoleLimbs]) {
    if (m.p[kVoleLimbs - 1] >> 31) {  // p >= 2^255: v < 2^256 <= 2p; p is uniform on the device, so is the branch
        vole_cond_sub(v, 0, m.p, out);
        return;
    }
    uint32_t vr[kVoleLimbs], one[kVoleLimbs] = {1, 0, 0, 0, 0, 0, 0, 0};
    vole_mont_mul(v, m.r2, m, vr);   // v * R mod p
    vole_mont_mul(vr, one, m, out);  // v mod p
}

// out = x * y mod p, any x, y < 2^256
GC_VOLE_HD inline void vole_mul_mod(const uint32_t (&x)[kVoleLimbs], const uint32_t (&y)[kVoleLimbs], const VoleMod &m,
                                    uint32_t (&out)[kVoleLimbs]) {
    uint32_t yr[kVoleLimbs];
    vole_mont_mul(y, m.r2, m, yr);  // y * R mod p
    vole_mont_mul(x, yr, m, out);   // x * y mod p
}

// out = (a + b) mod p, a, b < p; out may alias a or b
GC_VOLE_HD inline void vole_add_mod(const uint32_t (&a)[kVoleLimbs], const uint32_t (&b)[kVoleLimbs], const VoleMod &m,
                                    uint32_t (&out)[kVoleLimbs]) {
    uint32_t s[kVoleLimbs];
    uint64_t c = 0;
    GC_VOLE_UNROLL
    for (int j = 0; j < kVoleLimbs; j++) {
        const uint64_t x = (uint64_t)a[j] + b[j] + c;
        s[j] = (uint32_t)x;
        c = x >> 32;
    }
    vole_cond_sub(s, (uint32_t)c, m.p, out);  // a + b < 2p
}

// The constants of the modulus p (32 bytes, big-endian).  false: p is even or p < 3 — not supported (GC_E_ARG).
inline bool vole_mod_init(const uint8_t *p_be, VoleMod *m) {
    vole_load_be(p_be, m->p);
    bool above2 = false;
    for (int j = 1; j < kVoleLimbs; j++) above2 |= m->p[j] != 0;
    above2 |= m->p[0] >= 3;
    if (!(m->p[0] & 1) || !above2) return false;
    // p0^-1 mod 2^32 by Newton's iteration (each step doubles the correct low bits; p0 * p0 = 1 mod 8 to start)
    uint32_t inv = m->p[0];
    for (int k = 0; k < 5; k++) inv *= 2u - m->p[0] * inv;
    m->n0 = 0u - inv;
    // r2 = 2^512 mod p: double 1 512 times mod p (each step: x < p -> 2x < 2p, one conditional subtraction)
    uint32_t x[kVoleLimbs] = {1, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 512; k++) {
        uint32_t d[kVoleLimbs];
        uint32_t c = 0;
        for (int j = 0; j < kVoleLimbs; j++) {
            d[j] = (x[j] << 1) | c;
            c = x[j] >> 31;
        }
        vole_cond_sub(d, c, m->p, x);
    }
    for (int j = 0; j < kVoleLimbs; j++) m->r2[j] = x[j];
    return true;
}

}  // namespace gc
