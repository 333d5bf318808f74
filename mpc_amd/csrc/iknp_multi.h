// iknp_multi.h — the work items of the multi-session IKNP extension (gc_iknp_multi_*, iknp_multi_kernels.hip): S sessions
// of `per` OTs each, session-major, all at the same stream position.  An item is one chunk of one session (at most 512 OTs,
// the reference's 8 KiB message: ot/iknp.go:468-511); this header says where an item's bytes lie in the four arrays of a
// call and how many AES blocks one of its columns costs.  Plain C++ without HIP types: hipcc compiles it for host and
// device, g++ for the walk of tests/test_iknp_multi_index_host.py.
//
//   choice  [S][chunks * 64] bytes: packed LSB first, zero-padded to whole chunks; an item reads byte_rows of its 64
//   u       [S][u_bytes(per)] bytes: a session's chunks one after the other, each 128 columns x byte_rows, column-major
//   labels  [S][per] gc_label
//   keys    [S][128] base labels (sender) or label pairs (receiver): column col of session s is element s * 128 + col
//
// Every column stream of every session has given out `pos` bytes before the call, and a chunk takes 64 of them (the last
// one of a session byte_rows), so item (s, c) starts at byte pos + 64 c of its streams whatever s is.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GC_IKM_FN __host__ __device__ inline
#else
#define GC_IKM_FN inline
#endif

namespace gc {

constexpr uint32_t kIknpChunkRows = 512;  // OTs per chunk (iknp.go:58)

struct IknpMultiItem {
    uint64_t session, chunk;
    uint32_t rows;        // OTs of the item: 512, or what is left of the session
    uint32_t byte_rows;   // ceil(rows / 8): bytes of one column of the item
    uint32_t blocks;      // AES-CTR blocks that hold a column's byte_rows bytes from the item's stream position on
    uint64_t stream_pos;  // byte position of the item in every column stream of its session
    uint64_t choice_off;  // bytes
    uint64_t u_off;       // bytes, column 0; column col follows at col * byte_rows
    uint64_t label_off;   // labels
};

GC_IKM_FN uint64_t iknp_multi_chunks(uint64_t per) { return (per + kIknpChunkRows - 1) / kIknpChunkRows; }
// gc_iknp_u_bytes and the stream_advance of ot_engine.cpp for one session
GC_IKM_FN uint64_t iknp_multi_u_bytes(uint64_t per) {
    return (per / kIknpChunkRows) * 8192 + ((per % kIknpChunkRows + 7) / 8) * 128;
}
GC_IKM_FN uint64_t iknp_multi_advance(uint64_t per) { return (per / kIknpChunkRows) * 64 + (per % kIknpChunkRows + 7) / 8; }
GC_IKM_FN uint64_t iknp_multi_choice_bytes(uint64_t per) { return iknp_multi_chunks(per) * 64; }
GC_IKM_FN uint64_t iknp_multi_items(uint64_t S, uint64_t per) { return S * iknp_multi_chunks(per); }
// blocks of a column of byte_rows bytes that starts sh = pos % 16 bytes into a block: 1 .. 5
GC_IKM_FN uint32_t iknp_multi_blocks(uint32_t sh, uint32_t byte_rows) { return (sh + byte_rows + 15) / 16; }

// item `it` of iknp_multi_items(S, per), per > 0
GC_IKM_FN IknpMultiItem iknp_multi_item(uint64_t it, uint64_t per, uint64_t pos) {
    const uint64_t cps = iknp_multi_chunks(per);
    IknpMultiItem m;
    m.session = it / cps;
    m.chunk = it % cps;
    const uint64_t left = per - m.chunk * kIknpChunkRows;
    m.rows = (uint32_t)(left < kIknpChunkRows ? left : kIknpChunkRows);
    m.byte_rows = (m.rows + 7) / 8;
    m.stream_pos = pos + 64 * m.chunk;
    m.blocks = iknp_multi_blocks((uint32_t)(pos & 15u), m.byte_rows);
    m.choice_off = m.session * (cps * 64) + m.chunk * 64;
    m.u_off = m.session * iknp_multi_u_bytes(per) + m.chunk * 8192;
    m.label_off = m.session * per + m.chunk * kIknpChunkRows;
    return m;
}

// Workgroup steps of the kernel: a step serves `per_step` items (8 as sender, 4 as receiver); workgroup b takes steps
// b, b + grid, ...
GC_IKM_FN uint64_t iknp_multi_steps(uint64_t items, uint32_t per_step) { return (items + per_step - 1) / per_step; }

}  // namespace gc
