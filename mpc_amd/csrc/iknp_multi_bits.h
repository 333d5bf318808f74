// iknp_multi_bits.h — the index arithmetic of bit-COT over the multi-session IKNP handle (gc_iknp_multi_*_bits*,
// iknp_multi_bits_kernels.hip): S sessions of `per` OTs each, session-major, all at the same stream position, W = ceil(per / 64).
// The receiver walks the (session, chunk) items of iknp_multi.h; this header adds where an item's result words and choice
// words lie.  The sender has no items: a lane makes 16 result bytes of one session from column 0 alone.  Plain C++ without HIP
// types: hipcc compiles it for host and device, g++ for the walk of tests/test_iknp_multi_bits_index_host.py.
//
//   result   [S][W] u64: bit i of session s is bit i % 64 of word s * W + i / 64; bits at and behind `per` are zero
//   choices  u64 words: session s reads W words from word s * stride; stride 0 = one vector of W words for every session
//   u        as iknp_multi.h (the sender reads column 0 only: the first byte_rows bytes of a chunk)
//
// Result byte j of a session is byte pos + j of column 0's stream: a full chunk is 64 stream bytes and 64 result bytes, so
// the chunks of a session are contiguous in both (ReceiveBits, iknp.go:554-620; SendBits, :259-310).  The choice vector
// enters u in whole 64-bit words only: a chunk of byte_rows bytes folds in byte_rows / 8 words (:577-592).
#pragma once

#include <cstdint>

#include "iknp_multi.h"

namespace gc {

GC_IKM_FN uint64_t iknp_bits_words(uint64_t per) { return (per + 63) / 64; }
// 0 (shared) or at least a session's W words
GC_IKM_FN bool iknp_bits_stride_ok(uint64_t stride, uint64_t per) { return stride == 0 || stride >= iknp_bits_words(per); }
// words from choices[0] on that a call may read (S >= 1, per >= 1)
GC_IKM_FN uint64_t iknp_bits_choice_span(uint64_t S, uint64_t per, uint64_t stride) {
    return (S - 1) * stride + iknp_bits_words(per);
}
// the bits of word w of a session that hold OTs
GC_IKM_FN uint64_t iknp_bits_word_mask(uint64_t per, uint64_t w) {
    const uint64_t left = per > 64 * w ? per - 64 * w : 0;
    return left >= 64 ? ~0ull : (1ull << left) - 1;
}

// ---- receiver: what item m = iknp_multi_item(it, per, pos) adds to the label call's item ----
struct IknpBitsItem {
    uint64_t result_word;   // first word of result the item writes
    uint32_t result_words;  // ceil(rows / 64): 8, or what is left of the session's W
    uint64_t choice_word;   // first word of choices the item may read
    uint32_t choice_words;  // byte_rows / 8: the whole words that enter u
};

GC_IKM_FN IknpBitsItem iknp_bits_item(const IknpMultiItem &m, uint64_t per, uint64_t stride) {
    IknpBitsItem b;
    b.result_word = m.session * iknp_bits_words(per) + 8 * m.chunk;
    b.result_words = (m.rows + 63) / 64;
    b.choice_word = m.session * stride + 8 * m.chunk;
    b.choice_words = m.byte_rows / 8;
    return b;
}

// ---- sender: lane g of iknp_bits_send_lanes(S, per) makes result bytes [16 l, 16 l + 16) of its session ----
struct IknpBitsLane {
    uint64_t session;
    uint64_t word;        // session-local index of the lane's first result word: 2 l
    uint32_t words;       // result words the lane writes: 2, or 1 at the end of an odd W
    uint32_t nbytes;      // of the lane's 16 bytes, those that hold OTs: 16, or what is left of ceil(per / 8); >= 1
    uint64_t stream_pos;  // byte position of the lane's first byte in column 0's stream
    uint32_t blocks;      // AES-CTR blocks that hold the nbytes bytes: 1 or 2
    uint64_t u_off;       // byte of u that goes with the lane's first byte; the other nbytes - 1 follow it
};

GC_IKM_FN uint64_t iknp_bits_send_session_lanes(uint64_t per) { return (iknp_bits_words(per) + 1) / 2; }
GC_IKM_FN uint64_t iknp_bits_send_lanes(uint64_t S, uint64_t per) { return S * iknp_bits_send_session_lanes(per); }

// u_session / u_chunk: bytes between the sessions and between the chunks of u — iknp_multi_u_bytes(per) and 8192 for the
// message as it is, any other pair for a copy that holds column 0 only
GC_IKM_FN IknpBitsLane iknp_bits_send_lane(uint64_t g, uint64_t per, uint64_t pos, uint64_t u_session, uint64_t u_chunk) {
    const uint64_t lps = iknp_bits_send_session_lanes(per), W = iknp_bits_words(per);
    IknpBitsLane n;
    n.session = g / lps;
    const uint64_t l = g % lps, byte0 = 16 * l, bytes = (per + 7) / 8;
    n.word = 2 * l;
    n.words = (uint32_t)(W - n.word < 2 ? W - n.word : 2);
    n.nbytes = (uint32_t)(bytes - byte0 < 16 ? bytes - byte0 : 16);
    n.stream_pos = pos + byte0;
    n.blocks = iknp_multi_blocks((uint32_t)(pos & 15u), n.nbytes);
    n.u_off = n.session * u_session + (byte0 / 64) * u_chunk + byte0 % 64;
    return n;
}

// the host form's copy of column 0: a session's ceil(per / 8) bytes in a row, rows padded to 16 bytes
GC_IKM_FN uint64_t iknp_bits_col0_row(uint64_t per) { return ((per + 7) / 8 + 15) / 16 * 16; }

}  // namespace gc
