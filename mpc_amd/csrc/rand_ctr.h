// rand_ctr.h — the random streams of gc_rand_* (rand_engine.cpp, rand_kernels.hip), defined once.
//
// Stream s is the keystream of AES-CTR as Go's cipher.NewCTR(aes.NewCipher(seed[s]), iv[s]) gives it over zeros
// (crypto/cipher/ctr.go): block j is AES_seed[s](iv[s] + j), the sum taken on the 16-byte BIG-ENDIAN counter with the carry
// running through all 16 bytes and a silent wrap past 2^128 - 1.  Byte p of the stream is byte p % 16 of block p / 16.
// This header holds that counter addition, the split of a byte position and the cover of a byte range by blocks; the
// engine's argument checks and the kernels use it and nothing restates it.  Plain C++ without HIP types: hipcc compiles it
// for host and device, g++ for the walk of tests/test_rand_ctr_host.py.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GC_RAND_FN __host__ __device__ inline
#else
#define GC_RAND_FN inline
#endif

namespace gc {

// a counter block as two native words: hi = BE64(bytes 0..7), lo = BE64(bytes 8..15)
struct RandCtr {
    uint64_t hi, lo;
};

GC_RAND_FN uint64_t rand_be64(const uint8_t *b) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v = (v << 8) | b[i];
    return v;
}
GC_RAND_FN RandCtr rand_ctr_from_bytes(const uint8_t *iv) { return RandCtr{rand_be64(iv), rand_be64(iv + 8)}; }

// iv + j mod 2^128
GC_RAND_FN RandCtr rand_ctr_add(RandCtr iv, uint64_t j) {
    RandCtr c;
    c.lo = iv.lo + j;
    c.hi = iv.hi + (c.lo < iv.lo ? 1u : 0u);
    return c;
}

// byte position -> (block, offset inside it)
struct RandPos {
    uint64_t block;
    uint32_t off;
};
GC_RAND_FN RandPos rand_pos_split(uint64_t pos) { return RandPos{pos >> 4, (uint32_t)(pos & 15u)}; }

// The blocks that hold bytes [pos, pos + n) of a stream, n > 0 and pos + n <= 2^64 - 1 (rand_range_ok): block first + k for
// k < nblocks.  Block k of the cover holds bytes [16 k - head, 16 k - head + 16) of the range, cut to [0, n).
struct RandCover {
    uint64_t first;    // block of byte pos
    uint64_t nblocks;  // 1 .. 2^60
    uint32_t head;     // pos % 16: bytes of the first block that lie before the range
};
GC_RAND_FN RandCover rand_cover(uint64_t pos, uint64_t n) {
    const RandPos p = rand_pos_split(pos);
    return RandCover{p.block, (n >> 4) + ((p.off + (n & 15u) + 15u) >> 4), p.off};
}
// a position that a stream of at most 2^64 - 1 bytes can reach
GC_RAND_FN bool rand_range_ok(uint64_t pos, uint64_t n) { return n <= UINT64_MAX - pos; }

// What block k of a cover gives to its slot: bytes [from, to) of the block go to slot offset `at` onwards.  A whole block
// (from = 0, to = 16) can be stored in one piece; the ragged first and last block of a range cannot.
struct RandPiece {
    uint64_t at;
    uint32_t from, to;
};
GC_RAND_FN RandPiece rand_piece(const RandCover &c, uint64_t n, uint64_t k) {
    RandPiece p;
    p.from = k == 0 ? c.head : 0u;
    p.at = k == 0 ? 0u : 16 * k - c.head;
    const uint64_t left = n - p.at;  // bytes of the range from this piece on
    const uint32_t room = 16u - p.from;
    p.to = left < room ? p.from + (uint32_t)left : 16u;
    return p;
}

// A unit of kernel work is one wave's run of kRandRun consecutive blocks of one stream (one block per lane): unit u of
// S * rand_units(nblocks) serves stream u / units, cover blocks [64 (u % units), ...).
constexpr uint32_t kRandRun = 64;
GC_RAND_FN uint64_t rand_units(uint64_t nblocks) { return (nblocks + kRandRun - 1) / kRandRun; }

}  // namespace gc
