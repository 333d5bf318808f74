// co_multi_table.h — building the fixed-base window table of a point A_s (co_table.h) where it is used, in device memory,
// one table per session of a multi-session Chou-Orlandi receiver (gcengine.h: gc_co_multi_base_*).  The two lane bodies of
// co_multi_base_kernels.hip and their host check (tests/test_co_multi_table_host.py).  Plain C++ on top of co_table.h,
// compiled by hipcc for host and device and by g++ for the test.
//
// The table of a session is co_tab_build<W>(A_s), byte for byte: T[i][d - 1] = d * 2^(W * i) * A_s as affine Montgomery
// coordinates.  Field elements are fully reduced, so the affine coordinates of a point are unique whatever route the Jacobian
// arithmetic took: the host builder inverts once for all entries, a lane here once for its window, and the bytes agree.
//
// The work is split where its shape changes:
//   co_multi_tab_bases   one lane = one SESSION.  Checks A_s (pt_on_curve) and walks the W * (windows - 1) dependent doublings
//                        once, leaving the Jacobian base 2^(W * i) * A_s of every window in a workspace (CoTabBase, 96 bytes).
//   co_multi_tab_row     one lane = one (session, WINDOW).  Forward: d * B = (d - 1) * B + B, a doubling at d = 2 and
//                        pt_add_distinct beyond (the host builder's recurrence, valid for the same reason: 1 < d < N and B
//                        of order N).  X and Y of an entry go to its final slot in the table, its Z and the product of the
//                        Z before it to a workspace slot (CoTabZ, 64 bytes).  Then ONE inversion and a pass back down
//                        (Montgomery's trick) that overwrites the slots with affine x, y.  A lane reads back only what it
//                        wrote itself.
// Nothing but the base, the current entry and the running product lives across a step, and nothing is indexed by a register:
// the loops are not unrolled and address memory by their counter.
//
// MEM is the memory access: Fe ld(const uint32_t *) and void st(uint32_t *, const Fe &) on eight words, 16-byte aligned (two
// 16-byte loads or stores on the device, a copy on the host).
#pragma once

#include "co_table.h"

namespace gc {

// workspace of the build: a window's base in Jacobian coordinates, and an entry's Z next to the product of the Z before it
struct alignas(16) CoTabBase {
    uint32_t x[kVoleLimbs], y[kVoleLimbs], z[kVoleLimbs];
};
struct alignas(16) CoTabZ {
    uint32_t z[kVoleLimbs], prefix[kVoleLimbs];
};

// Lane s of the bases launch.  x, y: A_s as passed, plain values below 2^256.  false: not a point of the curve, a bad session;
// nothing is written then.  bases: [S][co_tab_windows(W)], the slots of every session.
template <int W, class MEM>
GC_P256_FN bool co_multi_tab_bases(const Fe &x, const Fe &y, size_t s, CoTabBase *bases, MEM mem) {
    constexpr int kSteps = W * (co_tab_windows(W) - 1);
    Aff a;
    if (!pt_on_curve(x, y, a)) return false;
    CoTabBase *out = bases + s * (size_t)co_tab_windows(W);
    Jac b = pt_from_aff(a);
    GC_P256_NOUNROLL
    for (int t = 0; t <= kSteps; t++) {  // one copy of the doubling in the code
        if (t % W == 0) {
            CoTabBase *o = out + t / W;
            mem.st(o->x, b.x);
            mem.st(o->y, b.y);
            mem.st(o->z, b.z);
        }
        if (t < kSteps) b = pt_dbl(b);
    }
    return true;
}

// base: this window's slot of co_multi_tab_bases; row: the co_tab_digits(W) entries of this window in the session's table;
// zs: as many workspace slots, this lane's own
template <int W, class MEM>
GC_P256_FN void co_multi_tab_row(const CoTabBase *base, CoTabEntry *row, CoTabZ *zs, MEM mem) {
    constexpr int kDigits = co_tab_digits(W);
    const Jac b = Jac{mem.ld(base->x), mem.ld(base->y), mem.ld(base->z)};
    Jac cur = b;
    Fe run = fe_one();
    GC_P256_NOUNROLL
    for (int d = 1; d <= kDigits; d++) {
        mem.st(row[d - 1].x, cur.x);
        mem.st(row[d - 1].y, cur.y);
        mem.st(zs[d - 1].z, cur.z);
        mem.st(zs[d - 1].prefix, run);  // the product of the Z before d
        run = fe_mul(run, cur.z);
        if (d < kDigits) cur = d == 1 ? pt_dbl(b) : pt_add_distinct(cur, b);
    }
    Fe inv = fe_inv(run);
    GC_P256_NOUNROLL
    for (int d = kDigits; d >= 1; d--) {
        const Fe zi = fe_mul(inv, mem.ld(zs[d - 1].prefix));
        inv = fe_mul(inv, mem.ld(zs[d - 1].z));
        const Fe zi2 = fe_sqr(zi);
        const Fe x = fe_mul(mem.ld(row[d - 1].x), zi2), y = fe_mul(mem.ld(row[d - 1].y), fe_mul(zi2, zi));
        mem.st(row[d - 1].x, x);
        mem.st(row[d - 1].y, y);
    }
}

// Lane l of a rows launch over the sessions s0 .. s0 + count - 1: window l % windows of session s0 + l / windows.  Lanes past
// the end and lanes of a bad session (good[s] = 0: no bases were stored) do nothing.  bases and tabs hold every session of
// the handle, tabs at 960 entries per session for W = 4; zs is the workspace of this launch alone, indexed from s0.
template <int W, class MEM>
GC_P256_FN void co_multi_tab_rows_lane(size_t l, size_t s0, size_t count, const uint32_t *good, const CoTabBase *bases,
                                       CoTabEntry *tabs, CoTabZ *zs, MEM mem) {
    constexpr size_t kWindows = co_tab_windows(W), kDigits = co_tab_digits(W), kEntries = co_tab_entries(W);
    if (l >= count * kWindows) return;
    const size_t c = l / kWindows, w = l - c * kWindows, s = s0 + c;
    if (!good[s]) return;
    co_multi_tab_row<W>(bases + s * kWindows + w, tabs + s * kEntries + w * kDigits, zs + c * kEntries + w * kDigits, mem);
}

}  // namespace gc
