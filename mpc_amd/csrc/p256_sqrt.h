// p256_sqrt.h — the square root mod p and the decompression of a P-256 point, for the Round 2 decode of sha2pc (sha2pc.h,
// sha2pc_kernels.hip) and its host check (tests/test_sha2pc_sqrt_host.py).  Plain C++ on p256.h, host and device as that
// header is.  The reference decompresses every choice point with elliptic.UnmarshalCompressed (sha2pc/encoding.go:505-543).
//
//   fe_sqrt        p = 3 mod 4, so a square t has the root t^((p + 1) / 4).  (p + 1) / 4 = 2^254 - 2^222 + 2^190 + 2^94: 32 one
//                  bits, 31 zeros, a one, 95 zeros, a one, 94 zeros — a fixed chain of 253 squarings and 7 products whatever
//                  t is.  The candidate is accepted only when its square is t: a non-residue gives false.
//   pt_decompress  X (plain, any value below 2^256) and the parity of y -> plain (x, y).  X >= p is refused, not reduced;
//                  x^3 - 3x + b a non-residue is refused; of the two roots the one whose PLAIN value has the parity asked
//                  for is taken (the other one is p - y; y = 0 stays 0, as y.Neg(y).Mod(y, p) leaves it).
#pragma once

#include "p256.h"

namespace gc {

// Montgomery form in, Montgomery form out; false: t is no square (y is then some value, not to be used)
GC_P256_FN bool fe_sqrt(const Fe &t, Fe &y) {
    const Fe x2 = fe_mul(fe_sqr(t), t);             // 2^2 - 1
    const Fe x4 = fe_mul(fe_sqr_n(x2, 2), x2);      // 2^4 - 1
    const Fe x8 = fe_mul(fe_sqr_n(x4, 4), x4);      // 2^8 - 1
    const Fe x16 = fe_mul(fe_sqr_n(x8, 8), x8);     // 2^16 - 1
    const Fe x32 = fe_mul(fe_sqr_n(x16, 16), x16);  // 2^32 - 1
    Fe r = fe_mul(fe_sqr_n(x32, 32), t);            // ffffffff 00000001
    r = fe_mul(fe_sqr_n(r, 96), t);                 // ... 00000000 00000000 00000001
    y = fe_sqr_n(r, 94);                            // ... << 94
    return fe_eq(fe_sqr(y), t);
}

// false: (X, odd) is no point of the curve; x and y are then zero
GC_P256_FN bool pt_decompress(const Fe &X, bool odd, Fe &x, Fe &y) {
    const Fe xm = fe_to_mont(X);  // (a value >= p is reduced by the product; the point is refused all the same)
    const Fe x3 = fe_mul(fe_sqr(xm), xm);
    const Fe rhs = fe_add(fe_sub(x3, fe_add(fe_add(xm, xm), xm)), fe_to_mont(p256_b()));
    Fe ym;
    const bool in_range = fe_below_p(X);
    const bool ok = fe_sqrt(rhs, ym) && in_range;
    const Fe yp = fe_from_mont(ym);
    const Fe yn = fe_neg(yp);
    y = fe_select(ok, fe_select(((yp.v[0] & 1u) != 0) == odd, yp, yn), fe_zero());
    x = fe_select(ok, X, fe_zero());
    return ok;
}

}  // namespace gc
