// co_sha256.h — deriveMask of the Chou-Orlandi OT (ot/co_helpers.go:222-235): SHA-256(x.Bytes() || y.Bytes() || BE64(id)) for
// one lane, with no indexed memory: the message is put together in registers.  Plain C++ as p256.h, so the host test hashes
// with the same code (tests/test_p256_host.py).
//
// big.Int.Bytes() is minimal-length, so a coordinate with leading zero bytes is hashed short and the point at infinity
// (0, 0) as two empty strings: the message has 8 to 72 bytes, one or two blocks, its length differs from lane to lane.  It is
// built from the fixed-width 72 bytes x32 || y32 || id8 by two left shifts that drop the zero bytes — first y32 || id8 by the
// leading zero bytes of y, then x32 || (that) by those of x — each a barrel shifter over words (conditional moves by 8, 4, 2,
// 1 words, then a funnel shift by 0..3 bytes), so every register index is a constant.  Only the first 16 bytes of the digest
// are used (xor truncates to LabelData, co_helpers.go:238-249), but they need all 64 rounds.
#pragma once

#include "p256.h"

namespace gc {

// leading zero bytes of a 256-bit value (0..32)
GC_P256_FN uint32_t co_leading_zero_bytes(const Fe &a) {
    uint32_t z = 0;
    bool open = true;
    GC_VOLE_UNROLL
    for (int i = kVoleLimbs - 1; i >= 0; i--) {
        const uint32_t w = a.v[i];
        const uint32_t here = w ? (uint32_t)__builtin_clz(w) >> 3 : 4u;
        z += open ? here : 0u;
        open = open && w == 0;
    }
    return z;
}

// w (big-endian words, w[0] first) <<= 32 * STEP when take.  A bit blend, not a conditional: the compiler turns a choice
// between two array elements into a load through a chosen address, and the array would then live in memory.
template <int STEP, int NW>
GC_P256_FN void co_shl_words(uint32_t (&w)[NW], bool take) {
    const uint32_t mask = 0u - (uint32_t)take;
    GC_VOLE_UNROLL
    for (int j = 0; j < NW; j++) {
        const uint32_t from = j + STEP < NW ? w[j + STEP < NW ? j + STEP : 0] : 0u;
        w[j] = (from & mask) | (w[j] & ~mask);
    }
}
// w <<= 8 * nbytes, zeros shifted in; nbytes <= 32
template <int NW>
GC_P256_FN void co_shl_bytes(uint32_t (&w)[NW], uint32_t nbytes) {
    co_shl_words<8>(w, (nbytes & 32u) != 0);
    co_shl_words<4>(w, (nbytes & 16u) != 0);
    co_shl_words<2>(w, (nbytes & 8u) != 0);
    co_shl_words<1>(w, (nbytes & 4u) != 0);
    const uint32_t r = 8u * (nbytes & 3u);
    GC_VOLE_UNROLL
    for (int j = 0; j < NW; j++) {
        const uint32_t next = j + 1 < NW ? w[j + 1 < NW ? j + 1 : 0] : 0u;
        w[j] = (uint32_t)((((uint64_t)w[j] << 32) | next) >> (32u - r));
    }
}

GC_P256_FN uint32_t co_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// one SHA-256 block: w is used up
GC_P256_FN void co_sha256_block(uint32_t (&st)[8], uint32_t (&w)[16]) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u,
        0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u,
        0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u,
        0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
        0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u,
        0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au,
        0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u,
        0xc67178f2u};
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    GC_VOLE_UNROLL
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
            const uint32_t s0 = co_rotr(w15, 7) ^ co_rotr(w15, 18) ^ (w15 >> 3);
            const uint32_t s1 = co_rotr(w2, 17) ^ co_rotr(w2, 19) ^ (w2 >> 10);
            w[i & 15] += s0 + w[(i - 7) & 15] + s1;
        }
        const uint32_t t1 = h + (co_rotr(e, 6) ^ co_rotr(e, 11) ^ co_rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const uint32_t t2 = (co_rotr(a, 2) ^ co_rotr(a, 13) ^ co_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + t2;
    }
    st[0] += a;
    st[1] += b;
    st[2] += c;
    st[3] += d;
    st[4] += e;
    st[5] += f;
    st[6] += g;
    st[7] += h;
}

// SHA-256 of the first len bytes (len <= 72) of the 18 big-endian words m, whose bytes from len on are zero
GC_P256_FN void co_sha256_short(const uint32_t (&m)[18], uint32_t len, uint32_t (&st)[8]) {
    uint32_t M[32];
    GC_VOLE_UNROLL
    for (int j = 0; j < 32; j++) M[j] = j < 18 ? m[j < 18 ? j : 0] : 0u;
    const uint32_t mark = 0x80000000u >> (8u * (len & 3u));
    GC_VOLE_UNROLL
    for (int j = 0; j < 19; j++) M[j] |= (uint32_t)j == (len >> 2) ? mark : 0u;
    const bool two = len > 55;  // 0x80 and the 64-bit length no longer fit the first block
    M[15] = two ? M[15] : 8u * len;
    M[31] = 8u * len;
    st[0] = 0x6a09e667u;
    st[1] = 0xbb67ae85u;
    st[2] = 0x3c6ef372u;
    st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu;
    st[5] = 0x9b05688cu;
    st[6] = 0x1f83d9abu;
    st[7] = 0x5be0cd19u;
    const int nblocks = two ? 2 : 1;
    GC_P256_NOUNROLL
    for (int b = 0; b < nblocks; b++) {
        uint32_t w[16];
        GC_VOLE_UNROLL
        for (int j = 0; j < 16; j++) w[j] = b ? M[16 + j] : M[j];
        co_sha256_block(st, w);
    }
}

// the message of deriveMask for the plain affine point (x, y): words and length
GC_P256_FN uint32_t co_mask_message(const Fe &x, const Fe &y, uint64_t id, uint32_t (&m)[18]) {
    const uint32_t zx = co_leading_zero_bytes(x), zy = co_leading_zero_bytes(y);
    uint32_t t[10];
    GC_VOLE_UNROLL
    for (int j = 0; j < 8; j++) t[j] = y.v[7 - j];
    t[8] = (uint32_t)(id >> 32);
    t[9] = (uint32_t)id;
    co_shl_bytes(t, zy);
    GC_VOLE_UNROLL
    for (int j = 0; j < 8; j++) m[j] = x.v[7 - j];
    GC_VOLE_UNROLL
    for (int j = 0; j < 10; j++) m[8 + j] = t[j];
    co_shl_bytes(m, zx);
    return 72u - zx - zy;
}

// mask[:16] as four big-endian words
GC_P256_FN void co_derive_mask(const Fe &x, const Fe &y, uint64_t id, uint32_t (&out)[4]) {
    uint32_t m[18], st[8];
    const uint32_t len = co_mask_message(x, y, id, m);
    co_sha256_short(m, len, st);
    GC_VOLE_UNROLL
    for (int j = 0; j < 4; j++) out[j] = st[j];
}

}  // namespace gc
