// yao_m3.h — the result message of circuit.Garbler (gc_yao_*), defined once.
//
// circuit/garbler.go:142-167 sets output i as bit i of a big.Int and sends SendData(result.Bytes()): BE32(n) and n bytes,
// big-endian and minimal, n = ceil(bitlen / 8), n = 0 for a zero result.  circuit/evaluator.go:144-148 reads any n with
// SetBytes, and IO.Split (ioarg.go:51-65) keeps the low nout bits.  The engine's bits array is the sha2pc digest layout:
// output i in bit i % 8 of byte i / 8, nb8 = ceil(nout / 8) bytes, so payload byte k of n is bits byte n - 1 - k.
// The kernels (one lane per byte), the CPU test (tests/cpp/yao_host_check.cpp) and nothing else restate this.  Plain C++.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GC_YAO_FN __host__ __device__ inline
#else
#define GC_YAO_FN inline
#endif

namespace gc {

GC_YAO_FN uint32_t yao_m3_bits_bytes(uint32_t nout) { return (nout + 7u) / 8u; }
// bytes of an M3 slot: the length word and the longest payload an honest garbler sends
GC_YAO_FN uint32_t yao_m3_slot_bytes(uint32_t nout) { return 4u + yao_m3_bits_bytes(nout); }

// n of result.Bytes(): the index of the highest non-zero bits byte, plus one
GC_YAO_FN uint32_t yao_m3_len(const uint8_t *bits, uint32_t nb8) {
    uint32_t n = nb8;
    while (n && !bits[n - 1]) n--;
    return n;
}

// byte k of the message, k < 4 + n
GC_YAO_FN uint8_t yao_m3_byte(const uint8_t *bits, uint32_t n, uint32_t k) {
    return k < 4u ? (uint8_t)(n >> (8u * (3u - k))) : bits[n - 1u - (k - 4u)];
}

// the length word of a received message
GC_YAO_FN uint32_t yao_m3_read_len(const uint8_t *msg) {
    return ((uint32_t)msg[0] << 24) | ((uint32_t)msg[1] << 16) | ((uint32_t)msg[2] << 8) | msg[3];
}

// bits byte j (j < nb8) of a received payload of n bytes: SetBytes, then the bits at index nout and above dropped
GC_YAO_FN uint8_t yao_m3_bits_byte(const uint8_t *payload, uint32_t n, uint32_t nout, uint32_t j) {
    uint8_t v = j < n ? payload[n - 1u - j] : (uint8_t)0;
    if (j == nout / 8u) v &= (uint8_t)((1u << (nout % 8u)) - 1u);  // the partial top byte (no such j when nout % 8 == 0)
    return v;
}

// the whole message into out (yao_m3_slot_bytes(nout) bytes of room); returns its length 4 + n
GC_YAO_FN uint32_t yao_m3_pack(const uint8_t *bits, uint32_t nout, uint8_t *out) {
    const uint32_t n = yao_m3_len(bits, yao_m3_bits_bytes(nout));
    for (uint32_t k = 0; k < 4u + n; k++) out[k] = yao_m3_byte(bits, n, k);
    return 4u + n;
}

// a message in a slot of `room` bytes into bits (nb8 bytes); false when 4 + n > room (nothing written)
GC_YAO_FN bool yao_m3_parse(const uint8_t *msg, uint64_t room, uint32_t nout, uint8_t *bits) {
    const uint32_t n = yao_m3_read_len(msg);
    if (4u + (uint64_t)n > room) return false;
    for (uint32_t j = 0; j < yao_m3_bits_bytes(nout); j++) bits[j] = yao_m3_bits_byte(msg + 4, n, nout, j);
    return true;
}

}  // namespace gc
