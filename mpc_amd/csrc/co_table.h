// co_table.h — fixed-base window tables for the receiver side of the Chou-Orlandi base OT (co_base_kernels.hip,
// co_engine.cpp: gc_co_base_*) and their host check (tests/test_co_table_host.py).  Plain C++ on top of p256.h, compiled by
// hipcc for host and device and by g++ for the test.
//
// The receiver multiplies a base that is the same for every OT of a session (G, then the sender's A) by a scalar of its
// own per OT.  For a width w the table of a base P of order N is
//     T[i][d - 1] = d * 2^(w * i) * P        window i = 0 .. ceil(256 / w) - 1, digit d = 1 .. 2^w - 1
// so that k * P is the sum of one entry per window, picked by the w-bit digits of k, without a single doubling: 64 mixed
// additions at w = 4 (704 products) where the ladder of pt_mul issues 256 doublings and 256 additions (4 864).
//
// An entry is an affine point in Montgomery form: x then y, 16 words, 64 bytes, 16-byte aligned (four 16-byte loads per
// lane).  There is no row for the digit 0: a zero digit reads the entry of digit 1 (a valid address, so the loads of a wave
// never diverge) and adds it with inf = 1, which pt_madd selects away.  No entry is the point at infinity: P has prime order
// N, and N divides neither a power of two nor a d below 2^w < N.
//
// Why the PLAIN addition (pt_madd<false>) is exact here.  pt_mul_tab reduces the scalar mod N first, so the digits are
// those of a k < N.  Walk the windows in either order.  Before the step of window j the accumulator is s * P and the entry
// is t * P with t = d * 2^(w * j), d != 0, where s is the sum of the other digits taken so far.  Low to high (the order
// used): s < 2^(w * j) <= t, so s != t.  High to low: s is a multiple of 2^(w * (j + 1)) > t, or zero.  In both orders
// s + t <= k < N with s, t >= 0, so s = -t mod N needs s + t = 0 or N: neither.  Hence the accumulator never meets the
// entry or its negative, and the only special cases left are an accumulator at infinity (s = 0) and a zero digit, both of
// which pt_madd's selects handle.  Digits of an UNREDUCED scalar k >= N would break the bound s + t < N: the reduction
// comes first.  The host test counts the additions that meet h = 0 with both operands finite (GC_CO_TABLE_COUNT): none.
// The table is unsigned; a signed-digit table of half the size would need its own argument here.
#pragma once

#include "p256.h"

#if defined(GC_CO_TABLE_BUILD)
#include <vector>
#endif

namespace gc {

struct alignas(16) CoTabEntry {
    uint32_t x[kVoleLimbs], y[kVoleLimbs];
};

constexpr int co_tab_windows(int w) { return (256 + w - 1) / w; }
constexpr int co_tab_digits(int w) { return (1 << w) - 1; }
constexpr size_t co_tab_entries(int w) { return (size_t)co_tab_windows(w) * co_tab_digits(w); }

#if defined(GC_CO_TABLE_COUNT) && !defined(__HIP_DEVICE_COMPILE__)
// host test only: plain additions of pt_mul_tab that met h = 0 (equal x) with both operands finite
inline unsigned long long &co_tab_exceptional() {
    static unsigned long long n = 0;
    return n;
}
#endif

// entry (window i, digit d) of a table of width W; d = 0 reads the entry of digit 1.  LOAD(const CoTabEntry *) -> CoTabEntry
// is the memory access: four 16-byte loads on the device, a copy on the host.
template <int W, class LOAD>
GC_P256_FN CoTabEntry co_tab_fetch(const CoTabEntry *tab, int i, uint32_t d, LOAD load) {
    const uint32_t at = (uint32_t)i * (uint32_t)co_tab_digits(W) + (d ? d - 1u : 0u);
    return load(tab + at);
}

// k * P from P's table of width W, for any k below 2^256 (limbs, least significant first): k mod N first, then one plain
// mixed addition per window, low window first.  The digit is the low W bits of a scalar that is shifted as a whole each
// step (indexing a limb by the loop counter would put the scalar in scratch); the loop is not unrolled (64 additions would
// be a megabyte of code).  The entry of the next window is fetched before the addition of this one, so the gather sits
// under the 11 products of an addition; the fetch behind the last window is that window's digit-1 entry again and is dropped.
template <int W, class LOAD>
GC_P256_FN Jac pt_mul_tab(const Fe &k, const CoTabEntry *tab, LOAD load) {
    static_assert(W >= 1 && W <= 16, "window width");
    constexpr int kWindows = co_tab_windows(W);
    constexpr uint32_t kMask = (1u << W) - 1u;
    Fe s = sc_reduce(k);
    Jac acc = pt_infinity();
    uint32_t d = s.v[0] & kMask;
    CoTabEntry cur = co_tab_fetch<W>(tab, 0, d, load);
    GC_P256_NOUNROLL
    for (int i = 0; i < kWindows; i++) {
        GC_VOLE_UNROLL
        for (int j = 0; j < kVoleLimbs - 1; j++) s.v[j] = (s.v[j] >> W) | (s.v[j + 1] << (32 - W));
        s.v[kVoleLimbs - 1] >>= W;
        const uint32_t dn = s.v[0] & kMask;
        const CoTabEntry nxt = co_tab_fetch<W>(tab, i + 1 < kWindows ? i + 1 : kWindows - 1, dn, load);
        Aff q;
        GC_VOLE_UNROLL
        for (int j = 0; j < kVoleLimbs; j++) {
            q.x.v[j] = cur.x[j];
            q.y.v[j] = cur.y[j];
        }
        q.inf = d == 0 ? 1u : 0u;
#if defined(GC_CO_TABLE_COUNT) && !defined(__HIP_DEVICE_COMPILE__)
        if (!q.inf && !pt_is_inf(acc) && fe_eq(fe_mul(q.x, fe_sqr(acc.z)), acc.x)) co_tab_exceptional()++;
#endif
        acc = pt_madd<false>(acc, q);
        cur = nxt;
        d = dn;
    }
    return acc;
}

// Jacobian + Jacobian, 12M + 4S, for distinct finite points that are not each other's negative (the table builds only:
// co_tab_build below on the host, co_multi_table.h on the device)
GC_P256_FN Jac pt_add_distinct(const Jac &p, const Jac &q) {
    const Fe z1z1 = fe_sqr(p.z), z2z2 = fe_sqr(q.z);
    const Fe u1 = fe_mul(p.x, z2z2), u2 = fe_mul(q.x, z1z1);
    const Fe s1 = fe_mul(p.y, fe_mul(q.z, z2z2)), s2 = fe_mul(q.y, fe_mul(p.z, z1z1));
    const Fe h = fe_sub(u2, u1), r = fe_sub(s2, s1);
    const Fe hh = fe_sqr(h), hhh = fe_mul(h, hh), v = fe_mul(u1, hh);
    Jac o;
    o.x = fe_sub(fe_sub(fe_sqr(r), hhh), fe_add(v, v));
    o.y = fe_sub(fe_mul(r, fe_sub(v, o.x)), fe_mul(s1, hhh));
    o.z = fe_mul(fe_mul(p.z, q.z), h);
    return o;
}

// ---- host only: building a table.  Compiled only where GC_CO_TABLE_BUILD is defined before the first include
// (co_engine.cpp, the host test), so the kernels' translation units see the half above alone. ----
#if defined(GC_CO_TABLE_BUILD)

// The table of a finite point P of order N, on the host: every entry in Jacobian coordinates (window i + 1 starts from W
// doublings of window i's first entry; d * B = (d - 1) * B + B, a doubling at d = 2 and distinct points beyond, since
// 1 < d < N), then ONE inversion for all of them (Montgomery's trick: prefix products of the Z, the inverse of the last,
// and back down).  A lone wave on the device would walk the same 252 dependent doublings in about 2 ms.
template <int W>
inline void co_tab_build(const Aff &P, CoTabEntry *out) {
    constexpr int kWindows = co_tab_windows(W), kDigits = co_tab_digits(W);
    const size_t n = co_tab_entries(W);
    std::vector<Jac> pts(n);
    Jac base = pt_from_aff(P);
    for (int i = 0; i < kWindows; i++) {
        Jac *row = pts.data() + (size_t)i * kDigits;
        row[0] = base;
        for (int d = 2; d <= kDigits; d++) row[d - 1] = d == 2 ? pt_dbl(base) : pt_add_distinct(row[d - 2], base);
        if (i + 1 < kWindows)
            for (int j = 0; j < W; j++) base = pt_dbl(base);
    }
    std::vector<Fe> prefix(n);
    Fe run = fe_one();
    for (size_t e = 0; e < n; e++) {
        prefix[e] = run;  // product of the Z before e
        run = fe_mul(run, pts[e].z);
    }
    Fe inv = fe_inv(run);
    for (size_t e = n; e-- > 0;) {
        const Fe zi = fe_mul(inv, prefix[e]);
        inv = fe_mul(inv, pts[e].z);
        const Fe zi2 = fe_sqr(zi);
        const Fe x = fe_mul(pts[e].x, zi2), y = fe_mul(pts[e].y, fe_mul(zi2, zi));
        for (int j = 0; j < kVoleLimbs; j++) {
            out[e].x[j] = x.v[j];
            out[e].y[j] = y.v[j];
        }
    }
}

#endif  // GC_CO_TABLE_BUILD

}  // namespace gc
