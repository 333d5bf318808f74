// rand_int.h — crand.Int on the random streams of rand_ctr.h (gc_rand_scalars_cur*), defined once.
//
// Go's crypto/rand.Int(reader, max) draws uniformly from [0, max) by rejection (crypto/rand/util.go): with
// bitlen = BitLen(max - 1), k = ceil(bitlen / 8) and b = bitlen % 8 (8 when that is 0), a candidate is the next k bytes of
// the reader, the first byte cut to its low b bits, read big-endian; a candidate < max is the answer, any other is thrown
// away and the next k bytes are tried.  A rejected candidate consumes exactly k bytes like an accepted one, so candidate j of
// a session sits at byte cursor + j k whatever was drawn before it, and `count` successive draws are the first `count`
// accepted candidates: a compaction, not a dependent chain.  Since max > 2^(bitlen - 1) a candidate is accepted with
// probability above 1/2, and the walk looks at no more than rand_int_cap(count) candidates (the contract's bound; it fails
// with probability below 2^-90).
// This header holds the shape of a modulus, the candidate and its test, the bound, the range test of a cursor and the walk
// in chunks of kRandIntChunk candidates; the engine's argument checks, the kernel (one lane per candidate of a chunk, the
// accept bits a ballot) and the host walk of tests/test_rand_int_host.py use it and nothing restates it.  Plain C++ as
// rand_ctr.h.
#pragma once

#include "rand_ctr.h"

#if defined(__HIPCC__)
#define GC_RAND_UNROLL _Pragma("unroll")
#else
#define GC_RAND_UNROLL
#endif

namespace gc {

// a modulus 2 <= max < 2^256 as the draw sees it; scalars are eight big-endian limbs, limb 0 the most significant
struct RandIntShape {
    uint32_t k;       // bytes of a candidate, 1 .. 32
    uint32_t mask;    // of a candidate's first byte
    uint32_t max[8];
};

// max: 32 bytes big-endian.  false for max = 0 (Go panics) and max = 1 (Go reads nothing): there is no shape
GC_RAND_FN bool rand_int_shape(const uint8_t *max, RandIntShape &sh) {
    uint32_t m1[8];  // max - 1
    uint32_t borrow = 1, any_high = 0;
    for (int i = 7; i >= 0; i--) {
        const uint8_t *b = max + 4 * i;
        sh.max[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        m1[i] = sh.max[i] - borrow;
        borrow = sh.max[i] < borrow ? 1u : 0u;
        if (i < 7) any_high |= sh.max[i];
    }
    if (!any_high && sh.max[7] < 2) return false;
    uint32_t bitlen = 0;
    for (int i = 0; i < 8 && !bitlen; i++)
        if (m1[i]) bitlen = 32u * (uint32_t)(8 - i) - (uint32_t)__builtin_clz(m1[i]);
    const uint32_t b = bitlen % 8 ? bitlen % 8 : 8;
    sh.k = (bitlen + 7) / 8;
    sh.mask = (1u << b) - 1;
    return true;
}

// the candidates a session may look at for `count` draws: 4 count + 256 (saturating)
GC_RAND_FN uint64_t rand_int_cap(uint64_t count) { return count > (UINT64_MAX - 256) / 4 ? UINT64_MAX : 4 * count + 256; }

// A cursor from which `count` draws cannot leave the stream's 2^64 - 1 bytes.  Conservative: it asks for room for all
// rand_int_cap(count) candidates, of which the draws will almost surely consume about half at most.
GC_RAND_FN bool rand_int_range_ok(const RandIntShape &sh, uint64_t pos, uint64_t count) {
    const uint64_t cap = rand_int_cap(count);
    return cap <= UINT64_MAX / sh.k && rand_range_ok(pos, sh.k * cap);
}

// the bits of limb i that a candidate may have set: none left of its first byte, `mask` in that byte, all behind it
GC_RAND_FN uint32_t rand_int_limb_mask(const RandIntShape &sh, uint32_t i) {
    const uint32_t pad = 32 - sh.k, first = pad >> 2;
    return i < first ? 0u : i > first ? ~0u : ((sh.mask << 24) | 0xffffffu) >> (8 * (pad & 3));
}

// The candidate whose byte i (of k) is byte_at(i): masked, zero-padded on the left.  Fixed trip count, fixed limb indices and
// no branch, so the limbs stay in registers and a byte's address is the candidate's plus a constant: byte_at is also asked
// for i = -1 .. k - 32, the bytes of the padding, and may answer those with anything: the limb masks clear them.
template <class ByteAt>
GC_RAND_FN void rand_int_candidate(const RandIntShape &sh, ByteAt byte_at, uint32_t (&v)[8]) {
    const int32_t pad = 32 - (int32_t)sh.k;
    GC_RAND_UNROLL
    for (int32_t i = 0; i < 8; i++) {
        uint32_t limb = 0;
        GC_RAND_UNROLL
        for (int32_t q = 4 * i; q < 4 * i + 4; q++) limb = (limb << 8) | ((uint32_t)byte_at(q - pad) & 0xffu);
        v[i] = limb & rand_int_limb_mask(sh, (uint32_t)i);
    }
}

GC_RAND_FN bool rand_int_accept(const RandIntShape &sh, const uint32_t (&v)[8]) {
    bool lt = false, eq = true;
    GC_RAND_UNROLL
    for (int i = 0; i < 8; i++) {
        lt = lt || (eq && v[i] < sh.max[i]);
        eq = eq && v[i] == sh.max[i];
    }
    return lt;
}

// The walk: candidates are looked at in chunks of at most kRandIntChunk; bit j of `accept` says that candidate
// consumed + j was accepted.  That candidate supplies output rand_int_slot(w, accept, j) where that is below count.
constexpr uint32_t kRandIntChunk = 64;
struct RandIntWalk {
    uint64_t accepted = 0;  // outputs supplied by the chunks before this one
    uint64_t consumed = 0;  // candidates of the chunks before this one
};
GC_RAND_FN uint64_t rand_int_slot(const RandIntWalk &w, uint64_t accept, uint32_t j) {
    return w.accepted + (uint64_t)__builtin_popcountll(accept & ((1ull << j) - 1));
}
// Behind a chunk of n candidates.  true: the chunk held the count-th accepted candidate and the walk ends right behind THAT
// candidate, not behind the chunk.  accepted < count on entry.
GC_RAND_FN bool rand_int_walk_step(RandIntWalk &w, uint64_t count, uint64_t accept, uint32_t n) {
    const uint64_t need = count - w.accepted, have = (uint64_t)__builtin_popcountll(accept);
    if (have < need) {
        w.accepted += have;
        w.consumed += n;
        return false;
    }
    for (uint64_t i = 1; i < need; i++) accept &= accept - 1;  // drop the need - 1 accepted candidates before it
    w.accepted = count;
    w.consumed += (uint64_t)__builtin_ctzll(accept) + 1;
    return true;
}

// `count` draws over an abstract byte source: byte_at(p) is byte p behind the cursor, emit(i, v) takes scalar i.  A first
// pass finds out whether the first rand_int_cap(count) candidates hold `count` accepted ones, and only then a second pass
// emits: a walk that fails (false, `consumed` = the bound) has emitted nothing.  On success `consumed` candidates, k bytes
// each, are what the cursor advances by.
template <class ByteAt, class Emit>
GC_RAND_FN bool rand_int_walk(const RandIntShape &sh, uint64_t count, ByteAt byte_at, Emit emit, uint64_t &consumed) {
    const uint64_t cap = rand_int_cap(count);
    consumed = 0;
    if (count == 0) return true;
    for (int pass = 0; pass < 2; pass++) {
        RandIntWalk w;
        bool done = false;
        while (!done && w.consumed < cap) {
            const uint32_t n = cap - w.consumed < kRandIntChunk ? (uint32_t)(cap - w.consumed) : kRandIntChunk;
            uint64_t accept = 0;
            for (uint32_t j = 0; j < n; j++) {
                const uint64_t at = (w.consumed + j) * sh.k;
                uint32_t v[8];
                rand_int_candidate(sh, [&](int32_t i) { return i < 0 ? 0u : (uint32_t)byte_at(at + (uint64_t)i); }, v);
                if (!rand_int_accept(sh, v)) continue;
                if (pass == 1 && rand_int_slot(w, accept, j) < count) emit(rand_int_slot(w, accept, j), v);
                accept |= 1ull << j;
            }
            done = rand_int_walk_step(w, count, accept, n);
        }
        consumed = w.consumed;
        if (!done) return false;
    }
    return true;
}

}  // namespace gc
