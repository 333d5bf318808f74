// co_multi.h — the sender's setup of ONE Chou-Orlandi session (GenerateCOSenderSetup, ot/co_helpers.go:77-101) from G's
// fixed-base window table, for k_co_multi_setup (co_multi_kernels.hip: one lane per session) and its host check
// (tests/test_co_multi_host.py).  Plain C++ on top of co_table.h, compiled by hipcc for host and device and by g++ for the
// test.
//
//     A = a * G        AaInv = -(a * A) = (x, p - y) of (a^2 mod N) * G
//
// Both products have G as their base, so both are sums of table entries (pt_mul_tab: 32 plain additions each at w = 8, no
// doubling) where gc_co_sender_setup walks two ladders.  a^2 mod N is two Montgomery products with the constants of N
// (vole_mul_mod: a * a * R^-1, then * R^2 * R^-1).  N is prime, so a^2 != 0 when a != 0: neither point is infinity for a
// good session.  The plain-addition argument of co_table.h asks only that the digits are those of a k < N, which holds
// for a mod N and for a^2 mod N alike.  ONE inversion serves both affine conversions (Montgomery's trick on the two Z).
#pragma once

#include "co_table.h"

namespace gc {

// a: the session's scalar as passed, any value below 2^256 (limbs, least significant first); modn: vole_mod_init of N.
// Plain affine coordinates out.  false: a = 0 mod N, a bad session; the four outputs are zero then.
template <int W, class LOAD>
GC_P256_FN bool co_multi_setup_session(const Fe &a, const VoleMod &modn, const CoTabEntry *g_tab, LOAD load, Fe &ax, Fe &ay,
                                       Fe &tx, Fe &ty) {
    const Fe k = sc_reduce(a);
    Fe k2;
    GC_P256_FLAT vole_mul_mod(k.v, k.v, modn, k2.v);
    Jac pa = pt_infinity(), paa = pt_infinity();
    GC_P256_NOUNROLL
    for (int h = 0; h < 2; h++) {  // one copy of the table walk in the code
        const Jac r = pt_mul_tab<W>(fe_select(h != 0, k2, k), g_tab, load);
        pa = pt_select(h != 0, pa, r);
        paa = r;
    }
    const Fe za = fe_select(pt_is_inf(pa), fe_one(), pa.z), zaa = fe_select(pt_is_inf(paa), fe_one(), paa.z);
    const Fe inv = fe_inv(fe_mul(za, zaa));
    Fe y;
    pt_to_affine(pa, fe_mul(inv, zaa), ax, ay);
    pt_to_affine(paa, fe_mul(inv, za), tx, y);
    ty = fe_neg(y);  // p - y (co_helpers.go:90-91); y != 0 on a curve of odd order, and infinity's 0 stays 0
    return !fe_is_zero(k);
}

}  // namespace gc
